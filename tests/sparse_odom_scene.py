"""The scene of the sparse odometry tests: tests/stereo_scene.py's textured planes seen by a 192 x 144 EUCM camera (the camera
and xi_base_cam of tests/photometric_scene.py) from three base poses about 0.15 m apart with a few degrees of yaw, the wheel
odometry's poses (the truth with every increment 5 % off), and a points-only set for the geometric half: 120 correspondences
of the true motion with 0.1 px noise, 25 of them replaced by random wrong pairs and 6 so far away that the regularised branch
of the triangulation is taken, with one fixed sample table [200][2] and one [200][3]."""
import numpy as np

from tests import photometric_ref as pr
from tests import photometric_scene as ps
from tests import sparse_odom_ref as sr
from tests import stereo_scene

W, H = 192, 144
CAM, XI_BASE_CAM = ps.CAM, ps.XI_BASE_CAM
STEPS = [[0.15, 0.01, 0.0, 0.0, 0.0, 0.05], [0.14, -0.02, 0.0, 0.0, 0.0, -0.04]]   # true base increments, [t, rotvec]
ODOM_FACTORS = [1.05, 0.95]
SMALL_FEATURES = 64
SEED = 5
_CACHE = {}


def true_poses():
    poses = [np.zeros(6)]
    for s in STEPS:
        poses.append(pr.compose(poses[-1], s))
    return poses


def odometry_poses():
    poses = [np.zeros(6)]
    for s, f in zip(STEPS, ODOM_FACTORS):
        poses.append(pr.compose(poses[-1], np.asarray(s) * f))
    return poses


def images():
    """u8 [3][H][W]"""
    if "images" not in _CACHE:
        _CACHE["images"] = np.stack([stereo_scene.render(CAM, *ps.camera_pose(xi), W, H) for xi in true_poses()])
    return _CACHE["images"]


def sample_table(points, m, seed=SEED):
    """[200][points] distinct indices below m per row"""
    rng = np.random.default_rng(seed + points)
    return np.stack([rng.choice(m, size=points, replace=False) for _ in range(sr.RANSAC_ITERATIONS)]).astype(np.int32)


def points_set(n=120):
    """dict(x1, x2 [n][3], p2 [n][2], size [n], xi_true, xi_odom, wrong indices, far indices, samples2, samples3): of 120 points
    25 are wrong and 6 far; another n keeps the construction and the shares (the sample tables need n >= 3)"""
    if ("points", n) not in _CACHE:
        rng = np.random.default_rng(SEED)
        xi_true = np.asarray(STEPS[0], float)
        xi_odom = xi_true * ODOM_FACTORS[0]
        xc = sr.camera_motion(np.asarray(XI_BASE_CAM, float), xi_true)
        R, t = pr.rotation_matrix(xc[3:]), xc[:3]
        far = np.arange(n * 100 // 120, n * 106 // 120)
        wrong = np.arange(n * 10 // 120, n * 35 // 120)
        p1 = np.stack([rng.uniform(15, W - 15, n), rng.uniform(15, H - 15, n)], 1)
        d1, _ = pr.reconstruct(CAM, p1[:, 0], p1[:, 1])
        depth = rng.uniform(0.8, 3.0, n)
        depth[far] = 1e4
        X = d1 / np.linalg.norm(d1, axis=1, keepdims=True) * depth[:, None]
        p2, ok = pr.project(CAM, (X - t) @ R)
        assert ok.all()
        noise = rng.normal(0., 0.1, p2.shape)
        noise[far] = 0.   # a far point's parallax is below the noise: kept exact so that its branch is certain
        p2 = p2 + noise
        p2[wrong] = np.stack([rng.uniform(15, W - 15, len(wrong)), rng.uniform(15, H - 15, len(wrong))], 1)
        x2, _ = pr.reconstruct(CAM, p2[:, 0], p2[:, 1])
        _CACHE["points", n] = {"x1": np.ascontiguousarray(d1), "x2": np.ascontiguousarray(x2), "p2": np.ascontiguousarray(p2), "size": np.ones(n),
                               "xi_true": xi_true, "xi_odom": xi_odom, "wrong": wrong, "far": far}
        if n >= 3:
            _CACHE["points", n].update(samples2=sample_table(2, n), samples3=sample_table(3, n))
    return _CACHE["points", n]


def detection(k, max_features):
    """the restatement's (keypoints, number of maxima, descriptors) of image k, cached"""
    key = ("detect", k, max_features)
    if key not in _CACHE:
        kp, n_max = sr.detect(images()[k], max_features)
        _CACHE[key] = (kp, n_max, sr.descriptors(images()[k], kp))
    return _CACHE[key]


def reference_ransac(points=2):
    """the restatement's ransac on the points set, cached and left unchanged"""
    key = ("ransac", points)
    if key not in _CACHE:
        s = points_set()
        _CACHE[key] = sr.ransac(CAM, XI_BASE_CAM, s["x1"], s["x2"], s["p2"], s["size"], s["xi_odom"], s["samples%d" % points], points)
    return _CACHE[key]


def reference_feed():
    """the restatement fed the three frames with the fixed sample table, cached"""
    if "feed" not in _CACHE:
        odo = sr.SparseOdometry(CAM, XI_BASE_CAM)
        states, incr, integ = [], [], []
        for img, xi in zip(images(), odometry_poses()):
            states.append(odo.feed(img, xi, points_set()["samples2"]))
            incr.append(odo.xi_incr.copy())
            integ.append(odo.xi_local.copy())
        _CACHE["feed"] = {"odo": odo, "states": states, "increments": incr, "integrated": integ}
    return _CACHE["feed"]


def pose_error(xi, xi_true):
    d = pr.inverse_compose(xi_true, xi)
    return float(np.linalg.norm(d[:3])), float(np.linalg.norm(d[3:]))


SOLVE_FLOOR = 1e-7


def solve_margin(x1, x2, p2, size, xi_odom, key=None):
    """(xi, margin) of one problem: the restatement's solve and 100 x its own spread -- its result at the default tolerances
    against its result with function and parameter tolerance tightened 100 x and 75 iterations -- with the floor SOLVE_FLOOR"""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    a, _ = sr.solve(CAM, XI_BASE_CAM, x1, x2, p2, size, xi_odom)
    b, _ = sr.solve(CAM, XI_BASE_CAM, x1, x2, p2, size, xi_odom, 75, sr.FTOL / 100, sr.PTOL / 100)
    out = (a, max(SOLVE_FLOOR, 100. * float(np.abs(a - b).max())))
    if key is not None:
        _CACHE[key] = out
    return out


def hypothesis_solves(points):
    """(xi [200][6], margin [200]) of the sample table's problems on the points set"""
    key = ("hyp", points)
    if key not in _CACHE:
        s = points_set()
        rows = [solve_margin(s["x1"][r], s["x2"][r], s["p2"][r], s["size"][r], s["xi_odom"]) for r in s["samples%d" % points]]
        _CACHE[key] = (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]))
    return _CACHE[key]


def short_solves(points, iterations=3):
    """dict(xi [200][6], iterations [200], initial_cost [200]) of the sample table's problems stopped after `iterations`"""
    key = ("short", points, iterations)
    if key not in _CACHE:
        s = points_set()
        rows = [sr.solve(CAM, XI_BASE_CAM, s["x1"][r], s["x2"][r], s["p2"][r], s["size"][r], s["xi_odom"], iterations) for r in s["samples%d" % points]]
        _CACHE[key] = {"xi": np.array([r[0] for r in rows]), "iterations": np.array([r[1]["iterations"] for r in rows]),
                       "initial_cost": np.array([r[1]["initial_cost"] for r in rows])}
    return _CACHE[key]


def clean_block(n=120):
    """indices of the correspondences that were not replaced: 95 of 120"""
    return np.setdiff1d(np.arange(n), points_set(n)["wrong"])
