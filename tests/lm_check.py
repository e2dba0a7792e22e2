"""The step-by-step comparison of a solver chain with the reference chain of tests/oracle_lm.py, shared by
tests/test_gpu_lm_steps.py (arrow system) and tests/test_gpu_lm_coupled_steps.py (full system: priors, odometry, ranks).
A plain module: nothing here runs by itself."""
import numpy as np

from tests import golden_cases as G
from tests import oracle_lm as L

BAR, RHO_MARGIN = L.BAR, L.RHO_MARGIN   # backward error of a step above its rounding floor; margin of every decision
COST_RTOL = 1e-12
RADIUS_RTOL = 1e-8


def reference_chain(route, c, R, a, k=3):
    """the reference chain from the case's initial point; every compared decision is far from the acceptance threshold"""
    ref = L.lm_chain(c, G.layout(c)[2], k, {"initial_trust_region_radius": R, "soft_l1_scale": a})
    for it in ref:
        assert abs(it["rho"] - L.DEFAULTS["min_relative_decrease"]) > RHO_MARGIN, (route, R, it["rho"])
    return ref


def check_iteration(what, c, a, opt, r, s, x, x_prev, radius_prev, worst):
    """iteration k of a solver chain (summary s, parameters x; x_prev / radius_prev after k - 1) against iteration k of
    the reference chain (r): success count exactly, cost beyond its rounding floor, radius, and the step -- a rejected one
    leaves x untouched, an accepted one solves the reference's damped system at the solver's own x_{k-1} to BAR above its
    rounding floor, and held / frozen columns, constant / unobserved poses do not move.
    worst [4]: running maxima of backward error, its floor, cost and radius deviation"""
    assert s["num_successful_steps"] == r["n_success"], (what, s["num_successful_steps"], r["n_success"])
    oc, fl = L.cost(c, x, a, floor=True)
    dc = max(abs(s["final_cost"] - oc) - fl, 0.0) / oc    # beyond the cost's rounding floor (oracle_lm.cost_floor)
    dr = abs(s["final_radius"] - r["radius"]) / r["radius"]
    assert dc <= COST_RTOL, (what, s["final_cost"], oc)
    assert dr <= RADIUS_RTOL, (what, s["final_radius"], r["radius"])
    worst[2], worst[3] = max(worst[2], dc), max(worst[3], dr)
    if not r["success"]:
        assert np.array_equal(x, x_prev), what   # a rejected step (a discarded speculation) leaves no trace
        return
    sy = L.system(c, x_prev, a)
    mu = 1.0 / radius_prev
    own = L.damped_step(sy, mu, opt)
    dg, dp = L.split_step(sy, x)
    # the reference's own step is not clipped by a bound: x_k - x_{k-1} is the step itself
    xg = x_prev[sy["gcols"]] + own["dg"]
    assert np.all((xg >= sy["lb"]) & (xg <= sy["ub"])), what
    assert np.all(dg[own["held"]] == 0.0), (what, "held / frozen columns moved")
    assert np.all(dp[~sy["pose_free"]] == 0.0), (what, "constant / unobserved poses moved")
    # x_k - x_{k-1} carries the rounding of x_k: each block may exceed BAR by its rounding floor (oracle_lm.backward_error)
    excess, be, floor = L.recovered_step_error(sy, mu, x, opt)
    worst[0], worst[1] = max(worst[0], be), max(worst[1], floor)
    assert excess <= BAR, (what, be, floor)


def check_chain(p, route, c, R, a, worst, route_ok):
    """solve(max_num_iterations=k) of problem p for k = 1, 2, 3 from the case's initial point, each against the reference
    chain (check_iteration); route_ok(summary) asserts that the problem's sizes select the route under test"""
    x0 = G.layout(c)[2]
    opt = {"initial_trust_region_radius": R, "soft_l1_scale": a}
    ref = reference_chain(route, c, R, a)
    x_prev, radius_prev = x0, R
    for k in (1, 2, 3):
        p.set_parameters(x0)
        s = p.solve(max_num_iterations=k, initial_trust_region_radius=R, soft_l1_scale=a)
        x = p.get_parameters()
        what = (route, R, k)
        assert s["termination"] == "NO_CONVERGENCE", (what, s["message"])
        route_ok(what, s)
        check_iteration(what, c, a, opt, ref[k - 1], s, x, x_prev, radius_prev, worst)
        x_prev, radius_prev = x, s["final_radius"]
    return ref
