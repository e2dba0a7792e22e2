"""Single Levenberg-Marquardt steps, and chains of two and three, of the HIP solver held to the dense damped-normal-equation
reference of tests/oracle_lm.py on every route of the reduced solve.

The optimum of a least-squares problem does not depend on the solver, so the optimum tests cannot see a wrong damping term,
a dropped W_i coupling or a wrong model change: they cost iterations, not the answer.  Here every case runs
solve(max_num_iterations=k) for k = 1, 2, 3 from the same start and compares, after each k:
  * the step x_k - x_{k-1}: its blockwise backward error in the reference's damped system at the solver's own x_{k-1}
    (mu = 1 / the solver's radius after k - 1 iterations) exceeds the rounding floor of x_k by at most BAR
    (tests/test_oracle_lm.py shows that planted errors of the kinds above land 100x and more above it); held and frozen
    columns, constant and unobserved poses do not move;
  * num_successful_steps exactly, and a rejected step leaves x untouched;
  * final_cost against the oracle's cost at the solver's x_k (1e-12 beyond the cost's rounding floor), final_radius
    against the reference chain (1e-8).
Every accept / reject decision of the reference chain is asserted to be far from min_relative_decrease, so the exact
comparison of the counts is not a coin toss.  Routes are reached on their default trigger where one exists, otherwise
through a debug hook (those cases skip on the production library); every case asserts that its sizes select its route.
The per-image pose refinement (refine_poses, vg_pose_lm.hpp) is held the same way to the 6 x 6 reference oracle_lm.pose_lm."""
import numpy as np
import pytest

from tests import lm_cases as C
from tests import lm_check as K
from tests import oracle_lm as L

pytestmark = pytest.mark.gpu

BAR, RHO_MARGIN = K.BAR, K.RHO_MARGIN   # backward error of a step above its rounding floor; margin of every decision
COST_RTOL = K.COST_RTOL
RADIUS_RTOL = K.RADIUS_RTOL

# (route, case, initial radii, SoftLOne scale, hooks, kernel the sizes select); a route named *_rejected must meet a rejected
# step, *_held a held column.  (The UCM case with radius 1e4 is left out: its second step is clipped by the bound, so
# x_k - x_{k-1} is not the step.)
ROUTES = [
    ("fold_kJ1_eucm", "mono_eucm", (1e4, 1.0, 1e-2), 0.0, {}, "fold kJ=1"),
    ("fold_kJ1_eucm_rejected", "mono_eucm_far", (1e16,), 0.0, {}, "fold kJ=1"),
    ("fold_kJ1_ucm_held", "mono_ucm_bound", (1e16,), 0.0, {}, "fold kJ=1"),
    ("fold_kJ2_g16", "rig_g16", (1e4, 1.0), 0.0, {}, "fold kJ=2"),
    ("fold_kJ2_stereo", "stereo_missing", (1e4, 1.0, 1e-2), 0.0, {}, "fold kJ=2"),
    ("fold_kJ2_g24", "rig_g24", (1e4, 1.0), 0.0, {}, "fold kJ=2"),
    ("no_fold_hook", "stereo_missing", (1e4, 1e-2), 0.0, {"solver_fold_max_groups": 1}, "entries"),
    ("no_fold_mono_16k", "mono_eucm_16k", (1e4,), 0.0, {}, "entries"),
    ("entries_mei_stereo_rejected", "stereo_mei", (1e4, 1.0, 1e16), 0.0, {}, "entries"),
    ("entries_rig4_device", "rig4", (1e4, 1.0), 0.0, {"solver_device_loop": 1}, "entries"),
    ("entries_mei4_device_rejected", "rig_mei4", (1e4, 1e16), 0.0, {"solver_device_loop": 1}, "entries"),
    ("entries_g63_device", "rig_g63", (1e4, 1.0), 0.0, {"solver_device_loop": 1}, "entries"),
    ("reduced_64_g64_device_rejected", "rig_g64", (1e4, 1.0, 1e16), 0.0, {"solver_device_loop": 1}, "reduced 64 threads"),
    ("reduced_256_mei8_device_rejected", "rig_mei8", (1e4, 1e16), 0.0, {"solver_device_loop": 1}, "reduced 256 threads"),
    ("host_rig4_rejected", "rig4", (1e4, 1e16, 1.0), 0.0, {}, "host"),
    ("host_mono_rejected", "mono_eucm_far", (1e16, 1.0), 0.0, {"solver_host_loop": 1}, "host"),
    ("host_260_datasets", "datasets_260", (1e4, 1.0), 0.0, {}, "host"),
    ("constant_camera_and_poses", "stereo_const", (1e4, 1.0), 0.0, {}, "fold kJ=2"),
    ("constant_global_transform", "stereo_const_transform", (1e4,), 0.0, {}, "fold kJ=2"),
    ("soft_l1_stereo", "stereo_missing", (1e4, 1.0), 2.0, {}, "fold kJ=2"),
]

# the library's route thresholds, restated so that a case whose sizes no longer select its route fails instead of silently
# testing another one (vg_lm_solve.hpp: device loop up to 32 global columns and kLmMaxDatasets = 256 datasets;
# vg_lm_device_loop.hpp / vg_solver_device.hpp: fold up to kFoldMaxG = 24 columns and kFoldMaxGroups = 480 back-substitution
# workgroups of 32 poses, kJ = 1 below 16 columns; entry-parallel solve up to kEntrySolveMaxG = 63; 64 threads up to 64)
def expected_route(G, n_poses, n_ds, hooks):
    if hooks.get("solver_host_loop") or n_ds > 256 or (G > 32 and not hooks.get("solver_device_loop")):
        return "host"
    if 0 < G <= 24 and -(-n_poses // 32) <= (hooks.get("solver_fold_max_groups") or 480):
        return "fold kJ=1" if G < 16 else "fold kJ=2"
    if G <= 63:
        return "entries"
    return "reduced 64 threads" if G <= 64 else "reduced 256 threads"


_WORST = {}


@pytest.fixture(scope="module")
def vg():
    import torch

    assert torch.cuda.is_available()
    import visgeom_amd

    return visgeom_amd


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for route, v in sorted(_WORST.items()):
        print("lm steps %-34s worst backward error %.2e (rounding floor %.2e)  cost %.2e  radius %.2e" % ((route,) + tuple(v)))


def _check_chain(vg, route, c, R, a, hooks, kernel):
    def route_ok(what, s):
        assert expected_route(s["num_global_columns"], s["num_pose_blocks"], len(c["datasets"]), hooks) == kernel, \
            (what, s["num_global_columns"], s["num_pose_blocks"])

    p = C.build_product_problem(vg, c)
    try:
        return K.check_chain(p, route, c, R, a, _WORST.setdefault(route, [0.0, 0.0, 0.0, 0.0]), route_ok)
    finally:
        p.close()


@pytest.mark.parametrize("route,name,radii,a,hooks,kernel", ROUTES, ids=[r[0] for r in ROUTES])
def test_lm_steps_equal_the_damped_normal_equations(vg, route, name, radii, a, hooks, kernel):
    from visgeom_amd import capi

    c = C.case(name)
    try:
        for h, v in hooks.items():
            capi.debug_set(h, v)
        refs = [_check_chain(vg, route, c, R, a, hooks, kernel) for R in radii]
    finally:
        if capi.has_debug_hooks():
            for h in hooks:
                capi.debug_set(h, 0)
    if route.endswith("_rejected"):
        assert any(not it["success"] for ref in refs for it in ref), route
    if route.endswith("_held"):
        assert any(it["held"].any() for ref in refs for it in ref), route


# ---- the per-image pose LM (vg_refine_poses): poses, iterations, final_cost and termination of every image after k iterations
POSE_CASES = [   # (model, images, corners per image, SoftLOne scale, initial radius); the first has an image with failed projections
    ("eucm", 96, 96, 25.0, 1e4),
    ("ucm", 65, 65, 25.0, 1e16),
    ("mei", 130, 7, 0.0, 1e4),
    ("eucm", 7, 96, 0.0, 1e16),
    ("mei", 96, 96, 25.0, 1e16),
    ("eucm", 6000, 96, 25.0, 1e16),   # more images than the persistent grid's first round: handed out through its counter
]


def _pose_problem(model, n, N, poison):
    """starts: small offsets (first step accepted), every third image 2.5x farther away (first step rejected at radius
    1e16); poison: image 1 behind an EUCM camera (94 of 96 corners fail to project: 1e15 residuals)"""
    from visgeom_amd import synthetic as S

    d = S.make_mono(model, n, 3)
    idx = np.arange(96)[:N] if N <= 96 else np.arange(96)
    start = d["gt_poses"] + np.random.default_rng(7).uniform(-0.03, 0.03, (n, 6))
    start[::3, 2] *= 2.5
    if poison:
        start[1] = [0.0, 0.0, -1.0, 0.0, 0.0, 0.0]
    return d["gt_intrinsics"] * (1 + 1e-3), d["board"][idx], d["corners"][:, idx], start


@pytest.mark.parametrize("model,n,N,a,R", POSE_CASES, ids=["%s-%d-N%d-a%g-R%g" % c for c in POSE_CASES])
def test_pose_lm_steps_equal_the_per_image_reference(vg, model, n, N, a, R):
    from visgeom_amd.calibration import refine_poses

    intr, board, corners, start = _pose_problem(model, n, N, (model, n, N, a, R) == POSE_CASES[0])
    opt = {"initial_trust_region_radius": R, "soft_l1_scale": a}
    prev = start
    worst = [0.0, 0.0, 0.0]
    rejected_first = accepted_first = 0
    close = set()
    for k in (1, 2, 3):
        poses, it, cost, term = refine_poses(model, intr, board, corners, start, max_num_iterations=k, **opt)
        for b in range(n):
            ref = L.pose_lm(model, intr, board, corners[b], start[b], dict(opt, max_num_iterations=k))
            what = (model, n, N, a, R, k, b)
            # a decision or convergence test of the reference near its threshold is a coin toss, not a finding: such images
            # (a few in a thousand) leave the exact comparison, and are counted.  (Convergence tests with a 1 % margin: what the
            # GPU's ~1e-15 cost error can move is ~1e-9 of them.)
            if any(abs(t["gain"] - 1e-3) <= RHO_MARGIN or any(0.99 < t.get(q, 0.0) < 1.01 for q in ("grad", "param", "func"))
                   for t in ref["trace"]):
                close.add(b)
                continue
            assert it[b] == ref["iterations"] and term[b] == ref["termination"], (what, it[b], term[b], ref)
            r, _ = L._pose_rows(model, intr, board, corners[b], poses[b])
            oc, fl = 0.5 * float(L.soft_l1(r @ r, a)[0]), L.cost_floor(r, corners[b].ravel(), a)
            worst[2] = max(worst[2], max(abs(cost[b] - oc) - fl, 0.0) / oc)
            assert abs(cost[b] - oc) <= COST_RTOL * oc + fl, (what, cost[b], oc, fl)
            last = ref["trace"][-1]
            if ref["iterations"] < k or not last["accepted"]:
                assert np.array_equal(poses[b], prev[b]), what    # no iteration k, or a rejected one: the pose did not move
            else:
                be, floor = L.pose_step_error(model, intr, board, corners[b], prev[b], poses[b], last["mu"], a, opt)
                worst[0], worst[1] = max(worst[0], be), max(worst[1], floor)
                assert be - floor <= BAR, (what, be, floor)
            if k == 1:
                rejected_first += not last["accepted"]
                accepted_first += last["accepted"]
        prev = poses
    print("pose lm %s n=%d N=%d a=%g R=%g: worst backward error %.2e (rounding floor %.2e), cost %.2e; first step rejected %d, "
          "accepted %d, near a threshold %d" % (model, n, N, a, R, worst[0], worst[1], worst[2], rejected_first, accepted_first,
                                                len(close)))
    assert len(close) <= max(1, n // 100), sorted(close)
    assert accepted_first > 0
    if R == 1e16:
        assert rejected_first > 0
