"""The scene of the photometric tests: tests/stereo_scene.py's textured planes seen by a 256 x 192 EUCM camera, the key
frame's depth map on a scale-2 grid (the true range, with holes and a few far values so that every depth test of the
selection is reached), three target views at known poses, and the poses the tests evaluate at.  256 x 192 with three scales
is the smallest shape at which the 50 / scale margin leaves an interior at every scale (39 x 23 pixels at scale 4).  It is
one size per level: the sizes at which the kernels' launches change shape (more workgroups than scan threads, packs of exactly a
wave or a workgroup, eight levels, points outside the target) live in tests/localization_shapes.py."""
import numpy as np

from tests import photometric_ref as pr
from tests import stereo_scene

W, H, NUM_SCALES = 256, 192, 3
CAM = [0.6, 1.05, 127., 125., 128., 96.]
PRM = {"scale": 2, "u0": 16, "v0": 16, "x_max": (W - 32) // 2 + 1, "y_max": (H - 32) // 2 + 1}
XI_BASE_CAM = [0.05, -0.02, 0.1, 0.01, -0.02, 0.015]
# the base frame of each target in the key frame's base frame, [t, rotvec]
TRUE_POSES = [[0.06, -0.03, 0.04, 0.01, -0.015, 0.02], [-0.05, 0.02, 0.03, -0.012, 0.01, -0.008], [0.02, 0.05, -0.04, 0.006, 0.012, 0.015]]
START_OFFSET = [0.02, -0.012, 0.015, 0.005, -0.006, 0.004]   # 2.8 cm and 0.5 degrees
_CACHE = {}


def camera_pose(xi):
    """(R, t) of the camera of base pose xi in the key frame's camera: xi_base_cam^-1 o xi o xi_base_cam"""
    c = pr.inverse_compose(XI_BASE_CAM, pr.compose(xi, XI_BASE_CAM))
    return pr.rotation_matrix(c[3:]), c[:3]


def scene():
    """dict(base u8 [H][W], targets u8 [3][H][W], depth [y_max][x_max])"""
    if "scene" not in _CACHE:
        base = stereo_scene.render(CAM, np.eye(3), np.zeros(3), W, H)
        targets = np.stack([stereo_scene.render(CAM, *camera_pose(xi), W, H) for xi in TRUE_POSES])
        yy, xx = np.mgrid[0:PRM["y_max"], 0:PRM["x_max"]]
        d = stereo_scene.reconstruct_np(CAM, (xx * PRM["scale"] + PRM["u0"]).astype(float), (yy * PRM["scale"] + PRM["v0"]).astype(float))
        lam = stereo_scene.cast(np.zeros(3), d)
        rng = lam * np.linalg.norm(d, axis=-1)
        depth = np.where(np.isfinite(rng), rng, 0.)
        rnd = np.random.default_rng(11)
        pick = rnd.random(depth.shape)
        depth[pick < 0.03] = 0.                          # OUT_OF_RANGE
        depth[(pick >= 0.03) & (pick < 0.05)] = 60.      # beyond DIST_MAX
        depth[(pick >= 0.05) & (pick < 0.06)] = 0.1      # below MIN_DEPTH: dropped by DepthMap::reconstruct
        _CACHE["scene"] = {"base": base, "targets": targets, "depth": np.ascontiguousarray(depth)}
    return _CACHE["scene"]


def localizer():
    """the reference restatement on the scene, built once and left unchanged"""
    if "loc" not in _CACHE:
        s = scene()
        loc = pr.Localizer(CAM, PRM, XI_BASE_CAM, NUM_SCALES)
        loc.set_base(s["base"], s["depth"])
        loc.set_targets(list(s["targets"]))
        _CACHE["loc"] = loc
    return _CACHE["loc"]


def start_pose(k=0, factor=1.):
    return list(np.asarray(TRUE_POSES[k]) + factor * np.asarray(START_OFFSET))


def eval_poses():
    """(poses [4][6], target index [4]) of the evaluate test: two targets, the truth, the start pose and two more"""
    poses = [TRUE_POSES[0], start_pose(0), start_pose(1, -0.7), list(np.asarray(TRUE_POSES[1]) + [0.01, 0.02, -0.015, -0.004, 0.003, 0.006])]
    return np.array(poses, float), np.array([0, 0, 1, 1], np.int32)


def reference_solve(k=0, factor=1., prior=False):
    """the restatement's computePose from start_pose(k, factor), cached"""
    key = ("solve", k, factor, prior)
    if key not in _CACHE:
        x0 = start_pose(k, factor)
        _CACHE[key] = localizer().compute_pose(x0, k, x0 if prior else None)
    return _CACHE[key]


def pose_error(xi, k=0):
    """(translation error in metres, rotation error in radians) against the truth of target k"""
    d = pr.inverse_compose(TRUE_POSES[k], xi)
    return float(np.linalg.norm(d[:3])), float(np.linalg.norm(d[3:]))
