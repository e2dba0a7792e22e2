"""The trust-region rule of the 6-parameter pose solves (visgeom_amd/csrc/vg_lm6.hpp), restated once in numpy for the
restatements that need it: photometric_ref.Localizer.solve_scale and sparse_odom_ref.solve.  Test infrastructure only; written
from reading Ceres' trust-region minimizer with its Levenberg-Marquardt strategy, not a binding of the library's."""
import math

import numpy as np

# Ceres' defaults; the iteration cap is the caller's
FTOL, GTOL, PTOL, RADIUS0, MAX_RADIUS, MIN_RADIUS = 1e-6, 1e-10, 1e-8, 1e4, 1e16, 1e-32
MIN_REL_DECREASE, DIAG_MIN, DIAG_MAX = 1e-3, 1e-6, 1e32
TERM_FUNCTION, TERM_GRADIENT, TERM_PARAMETER, TERM_NO_CONVERGENCE, TERM_RADIUS = 0, 1, 2, 3, 4


def solve(f, x0, max_iterations, ftol=FTOL, gtol=GTOL, ptol=PTOL, radius0=RADIUS0, max_radius=MAX_RADIUS,
          min_radius=MIN_RADIUS, min_rel_decrease=MIN_REL_DECREASE, diag_min=DIAG_MIN, diag_max=DIAG_MAX):
    """the loop on f: x -> (cost, JtJ [6, 6], g [6]) from x0: (x, dict(iterations, initial_cost, final_cost, termination)).
    The tolerances are tested on the candidate before it is taken; a step that cannot be made (no Cholesky factor, a step
    that is not finite) or is refused shrinks the radius by a factor that doubles with every refusal in a row."""
    x = np.asarray(x0, float).copy()
    cost, JtJ, g = f(x)
    rep = {"iterations": 0, "initial_cost": cost, "termination": TERM_NO_CONVERGENCE}
    radius, dec = radius0, 2.
    while rep["iterations"] < max_iterations:
        rep["iterations"] += 1
        mu = 1. / radius
        D = np.clip(np.diag(JtJ), diag_min, diag_max)
        step_ok = True
        try:
            L = np.linalg.cholesky(JtJ + mu * np.diag(D))
            dx = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            step_ok = bool(np.isfinite(dx).all())
        except np.linalg.LinAlgError:
            step_ok = False
        success = False
        if step_ok:
            cost_c, JtJ_c, g_c = f(x + dx)
            model_change = 0.5 * (mu * float(D @ (dx * dx)) - float(g @ dx))
            rho = (cost - cost_c) / model_change if model_change > 0. else -1.
            if np.abs(g).max() <= gtol:
                rep["termination"] = TERM_GRADIENT
                break
            if math.sqrt(float(dx @ dx)) <= ptol * (math.sqrt(float(x @ x)) + ptol):
                rep["termination"] = TERM_PARAMETER
                break
            if model_change > 0. and math.isfinite(cost_c) and abs(cost - cost_c) <= ftol * cost:
                rep["termination"] = TERM_FUNCTION
                break
            success = math.isfinite(cost_c) and rho > min_rel_decrease
        if success:
            x, cost, JtJ, g = x + dx, cost_c, JtJ_c, g_c
            radius = min(radius / max(1. - (2. * rho - 1.) ** 3, 1. / 3.), max_radius)
            dec = 2.
        else:
            radius /= dec
            dec *= 2.
            if radius < min_radius:
                rep["termination"] = TERM_RADIUS
                break
    rep["final_cost"] = cost
    return x, rep
