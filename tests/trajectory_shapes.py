"""Inputs of the trajectory shape tests (tests/test_gpu_trajectory_shapes.py, tests/test_trajectory_shapes_cpu.py): the scene of
tests/golden/trajectory_plan.json ("the plan": its camera, image size and quality parameters) at the sizes where the launches of
vg_trajectory.hpp change shape, and the restatement's results on them (tests/trajectory_ref.py, long double and float64), each
computed once per process and left unchanged.  "tilted" is the plan with min_camera_dist 3.5 and the board turned 0.7 about its
y axis, as in tests/test_gpu_trajectory.py: the distance and normal penalties become active.

A  A_STEPS: 8 trajectories, 18 slots, four trajectories of a single slot, two of them adjacent at the front; A-invalid: two
   poses in the middle of trajectory 5 out of view, three valid trajectories behind them.
B  B1_STEPS [256, 2] and B8_STEPS [256] * 8 (2040 slots): the prepass walk at its cap, next to the shortest one.
C  BOARDS: 1024 and 1023 corners, the 2 x 2 minimum, single rows and columns of cells, 65 and 128 corners, on 2 + 3 poses.
D  D_STEPS, T = 3: 130 points; the prepass items 3 k .. 3 k + 2 put points 21 and 42 astride a block of 64.
E  one trajectory of 2 poses in front of a 2 x 2 board at the cap of 65 535 points, cycling over three points.
F  seven starts of the plan's own two trajectories for the lock-step minimisation."""
import copy
import os

import numpy as np

from tests import trajectory_ref as tr

PLAN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trajectory_plan.json")
LD = np.longdouble
EPS = 2. ** -52
WAVE = 64                                      # lanes of a prepass or finish block
TILT, TILTED_MIN_DIST = 0.7, 3.5
SETTINGS = ("plan", "tilted")
TERMS = ("information", "image_limits", "curvature", "distance", "normal")
BASE = [0.2, 0.1, 0.05, 0.15, 0.12]            # trajectory 1 of the plan
COND_MAX = 1e-6 / (64 * EPS)                   # above it the bound 64 eps cond(JtCJ) on cov says nothing

A_STEPS = [2, 2, 3, 2, 9, 2, 2, 4]
A_INVALID_SLOTS = [11, 12]
A_THETA_LAST = 0.6                             # without it the image-limits term of A is 0.39 (plan) and 0 (tilted): not "active"
B1_STEPS = [256, 2]
B1_PARAMS = [0.2, 0.1, 0.05, 0.004, 0.003, -0.1, -0.2, -0.1, 0.1, -0.05]
B8_STEPS = [256] * 8
C_STEPS = [2, 3]
C_PARAMS = [0.2, 0.1, 0.05, 0.15, 0.12, -0.1, -0.2, -0.1, 0.1, -0.09]   # a turn of -0.1 would sit on the curvature threshold: 1e-30, not 0
BOARDS = ((32, 32, 0.02), (31, 33, 0.02), (2, 2, 0.5), (2, 33, 0.02), (33, 2, 0.02), (13, 5, 0.06), (16, 8, 0.05))   # cols, rows, step
D_STEPS = [3, 2, 4]
D_THIRD = [0.0, 0.3, 0.2, 0.12, -0.08]
D_POINTS = 130
D_CHECKED = (0, 21, 42, 63, 64, 65, 129)
D_CHUNK = 21                                   # 21 points x 3 trajectories = 63 items: one block for either kernel
E_STEPS = [2]
E_BOARD = (2, 2, 0.5)
E_POINTS = 65535
E_THREE = [BASE, [-0.1, -0.2, -0.1, 0.1, -0.2], D_THIRD]
F_STARTS = 7
_CACHE = {}


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def plan():
    """dict(cam, w, h, q, steps, start) of the plan file"""
    if "plan" not in _CACHE:
        cam, w, h, q, steps, start = tr.load_plan(PLAN)
        _CACHE["plan"] = dict(cam=cam, w=w, h=h, q=q, steps=steps, start=_f64(start))
    return _CACHE["plan"]


def quality_parameters(setting, board=None):
    """the "quality_parameters" object of a setting, with another board (cols, rows, step) when one is given"""
    assert setting in SETTINGS
    q = copy.deepcopy(plan()["q"])
    if setting == "tilted":
        q["min_camera_dist"] = TILTED_MIN_DIST
        q["xiOrigBoard"] = [float(v) for v in tr.compose(_f64(q["xiOrigBoard"]), _f64([0, 0, 0, 0, TILT, 0]))]
    if board is not None:
        q["board"] = dict(cols=int(board[0]), rows=int(board[1]), step=float(board[2]))
    return q


def quality(setting, steps, board=None, dtype=np.float64):
    p = plan()
    return tr.Quality(p["cam"], p["w"], p["h"], quality_parameters(setting, board), steps, dtype)


def reference(setting, steps, params, board=None):
    """the restatement's evaluate at one point: dict(ld, f64: (cost, terms, invalid), poses: the per-pose detail in float64)"""
    key = ("ref", setting, tuple(steps), board, _f64(params).tobytes())
    if key not in _CACHE:
        ld = quality(setting, steps, board, LD).evaluate(params)
        f64 = quality(setting, steps, board).evaluate(params, detail=True)
        _CACHE[key] = dict(ld=ld, f64=f64[:3], poses=f64[3])
    return _CACHE[key]


def spread(ref):
    """the largest float64 / long-double difference of the cost and the terms of a reference(), over max(1, |ref|); 0 where both
    are the same infinity"""
    worst = 0.
    for a, b in zip([ref["ld"][0]] + list(ref["ld"][1]), [ref["f64"][0]] + list(ref["f64"][1])):
        if np.isinf(float(a)) and float(a) == float(b):
            continue
        worst = max(worst, abs(float(b) - float(a)) / max(1., abs(float(a))))
    return worst


def blocks_of(n):
    return (n + WAVE - 1) // WAVE


def straddlers(n_points, T):
    """the points whose T prepass items lie in two blocks"""
    return [k for k in range(n_points) if (T * k) // WAVE != (T * k + T - 1) // WAVE]


# ---- A -------------------------------------------------------------------------------------------------------------

def a_params(invalid=False):
    rng = np.random.default_rng(1)
    p = np.concatenate([_f64(BASE) * (1 + 0.3 * rng.standard_normal(5)) for _ in A_STEPS])
    p[19] = -0.25                              # the turn of trajectory 4: the curvature penalty
    p[37] = A_THETA_LAST                       # trajectory 8 looks past the board: the image limits in its three poses
    if invalid:
        p[24] = -0.3
    return p


def gradient_reference(setting, steps, params):
    """the restatement's central differences: dict(ld, f64: the gradient, delta)"""
    key = ("grad", setting, tuple(steps), _f64(params).tobytes())
    if key not in _CACHE:
        g, delta = quality(setting, steps, None, LD).gradient(params)
        g64, _ = quality(setting, steps).gradient(params)
        _CACHE[key] = dict(ld=g, f64=g64, delta=delta)
    return _CACHE[key]


# ---- B -------------------------------------------------------------------------------------------------------------

def b8_params():
    return np.concatenate([[0.2 + 0.01 * k, 0.1 - 0.02 * k, 0.05, 0.004 + 0.0002 * k, 0.003 - 0.001 * k] for k in range(8)])


def b1_batch():
    """33 points: B1_PARAMS in the even rows, in the odd rows B1_PARAMS with the second trajectory perturbed"""
    rng = np.random.default_rng(3)
    batch = np.repeat(_f64(B1_PARAMS)[None], 33, axis=0)
    batch[1::2, 5:] += 0.01 * rng.standard_normal((16, 5))
    return batch


# ---- C -------------------------------------------------------------------------------------------------------------

def cell_share(setting, board):
    """(the image-limits term of C on the board, its part from the cell sizes): the whole less what remains at min_cell_size 0"""
    whole = reference(setting, C_STEPS, C_PARAMS, board)["f64"][1][1]
    Q = quality(setting, C_STEPS, board)
    Q.min_cell = np.float64(0.)
    corners = sum(Q.image_limits_cost(pose) for pose in Q.camera_poses(C_PARAMS))
    return float(whole), float(whole - corners)


def cov_reference(board):
    """visual_cov of the board (plan setting) at the three camera poses of C: (poses [3, 6], a list of dict(ld, f64: (cov, JtJ, JtCJ,
    valid), cond))"""
    key = ("cov", board)
    if key not in _CACHE:
        Q, QL = quality("plan", C_STEPS, board), quality("plan", C_STEPS, board, LD)
        poses = Q.camera_poses(C_PARAMS)
        rows = []
        for pose in poses:
            ld, f64 = QL.visual_cov(pose), Q.visual_cov(pose)
            rows.append(dict(ld=ld, f64=f64, cond=float(np.linalg.cond(_f64(ld[2])))))
        _CACHE[key] = (poses, rows)
    return _CACHE[key]


# ---- D -------------------------------------------------------------------------------------------------------------

def d_start():
    return np.concatenate([plan()["start"], D_THIRD])


def d_points():
    return d_start() + 0.01 * np.random.default_rng(7).standard_normal((D_POINTS, 15))


# ---- E -------------------------------------------------------------------------------------------------------------

def e_points():
    return _f64(E_THREE)[np.arange(E_POINTS) % 3]


# ---- F -------------------------------------------------------------------------------------------------------------

def f_starts():
    return plan()["start"] * (1 + 0.15 * np.random.default_rng(11).standard_normal((F_STARTS, 10)))
