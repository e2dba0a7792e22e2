"""An independent check of a converged calibration at ANY size: the ORACLE's rows at x*, the arrow-structured
Gauss-Newton step formed from them on the host (numpy: per-pose 6 x 6 elimination, G x G solve, box bounds respected).

At a least-squares optimum that step vanishes, whatever solver found the point -- so "the HIP solver converges to the same
intrinsics as the reference's ceres::Solve (src/calibration/unified_calibration.cpp:42-53) within 1e-6" is checked at
BASELINE sizes as: the oracle's cost at x* equals the solver's, and the oracle's undamped Gauss-Newton step from x* moves
no parameter by more than 1e-6.  (The distance to the optimum IS that step, to first order: delta = -(J^T J)^-1 J^T r.)
Nothing here touches the product: rows from oracle/vgo.py, algebra from numpy.  Test infrastructure only.

A case is the dict of tests/golden_cases.py (cameras / transforms / datasets, image b of a dataset uses element b of its
sequence transform).
"""
import os

import numpy as np

from tests import golden_cases as G


def full_size_case(name):
    """BASELINE.json's configurations at their full sizes, from the seeded generator (visgeom_amd/synthetic.py)"""
    from visgeom_amd import synthetic as S

    if name == "headline_eucm_10k":   # the metric's own set: seed index 1
        d = S.make_mono("eucm", 10000, 1)
        return {"name": name, "cameras": [("eucm", d["init_intrinsics"])], "transforms": [(False, d["init_poses"])],
                "datasets": [(0, [(0, 0)], d["board"], d["corners"])]}
    if name == "config2_eucm_1k":
        d = S.make_mono("eucm", 1000, 2)
        return {"name": name, "cameras": [("eucm", d["init_intrinsics"])], "transforms": [(False, d["init_poses"])],
                "datasets": [(0, [(0, 0)], d["board"], d["corners"])]}
    if name == "config3_stereo_2k":
        s = S.make_stereo(2000)
        return {"name": name, "cameras": [("eucm", s["init_intrinsics1"]), ("eucm", s["init_intrinsics2"])],
                "transforms": [(True, s["init_xi12"][None, :]), (False, s["init_poses"])],
                "datasets": [(0, [(1, 0)], s["board"], s["corners1"]), (1, [(0, 1), (1, 0)], s["board"], s["corners2"])]}
    if name == "config4_mei_10k":
        d = S.make_mono("mei", 10000, 4)
        return {"name": name, "cameras": [("mei", d["init_intrinsics"])], "transforms": [(False, d["init_poses"])],
                "datasets": [(0, [(0, 0)], d["board"], d["corners"])]}
    if name == "config5_rig_5k":
        r = S.make_rig(5000, sigma=0.1)
        return {"name": name, "cameras": list(zip(r["models"], r["init_intrinsics"])),
                "transforms": [(True, x[None, :]) for x in r["init_xi1k"]] + [(False, r["init_poses"])],
                "datasets": [(0, [(3, 0)], r["board"], r["corners"][0])] +
                            [(k + 1, [(k, 1), (3, 0)], r["board"], r["corners"][k + 1]) for k in range(3)]}
    raise KeyError(name)


def shard_case(c, lo, hi):
    """images [lo, hi) of every dataset and sequence transform (what one rank of a sharded solve holds)"""
    return {"name": "%s[%d:%d]" % (c["name"], lo, hi), "cameras": c["cameras"],
            "transforms": [(g, v if g else np.asarray(v)[lo:hi]) for g, v in c["transforms"]],
            "datasets": [(cam, chain, board, np.asarray(corners)[lo:hi]) for cam, chain, board, corners in c["datasets"]]}


def gauss_newton_step(c, x, threads=None):
    """-> dict(cost, dg [G], gcols [G] parameter index of every global column, dp [P, 6], pose_param [P] first parameter
    of every pose block, grad_g, grad_p).  Undamped: (J^T J) delta = -J^T r, solved through the Schur complement of the
    pose blocks; global parameters sitting on a bound of their camera's box with the step pointing outwards are held.
    The mu = 0, no-loss case of the damped step of tests/oracle_lm.py."""
    from tests import oracle_lm

    if threads is None:
        threads = max(1, min(32, os.cpu_count() or 1))
    sy = oracle_lm.arrow_system(c, x, threads=threads)
    st = oracle_lm.damped_step(sy, 0.0)
    return {"cost": sy["cost"], "dg": st["dg"], "gcols": sy["gcols"], "dp": st["dp"], "pose_param": sy["pose_param"],
            "grad_g": sy["gg"], "grad_p": sy["gp"], "held": st["held"]}


def assert_converged(c, x, final_cost, tol=1e-6, cost_rtol=1e-9, cost_scale=1.0, what=""):
    """the bar of BASELINE.json / VERDICT r2 item 1: oracle cost == solver cost (1e-9), Gauss-Newton step of the oracle
    at x* <= tol on every global parameter (relative to max(|x|, 1)) and on every pose component (absolute)"""
    g = gauss_newton_step(c, x)
    assert abs(cost_scale * g["cost"] - final_cost) <= cost_rtol * final_cost, (what, g["cost"], final_cost)
    xg = np.asarray(x, float)[g["gcols"]]
    step_g = np.max(np.abs(g["dg"]) / np.maximum(np.abs(xg), 1.0)) if g["dg"].size else 0.0
    step_p = float(np.max(np.abs(g["dp"]))) if g["dp"].size else 0.0
    assert step_g <= tol, (what, "global step", step_g)
    assert step_p <= tol, (what, "pose step", step_p)
    return step_g, step_p
