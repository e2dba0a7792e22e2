"""The scene of the mutual-information tests: tests/photometric_scene.py's key frame, packs and three targets, plus target 0
passed through the grey-level remap of tests/mi_ref.py as target 3 (a second pass with another exposure), the poses the tests
evaluate at, and the restatement's solves, cached per process and left unchanged."""
import numpy as np

from tests import mi_ref as mr
from tests import photometric_ref as pr
from tests import photometric_scene as ps

REMAPPED = 3                      # the target index of the remapped target 0
TIGHT = {"ftol": 1e-9, "gtol": 1e-6}   # the tolerances at which the restatement's solves from three starts end at one point
# a pose far from every truth: 14 % to 18 % of each pack fails projectPoint, none within 1e-4 of its thresholds
FAILING_POSE = list(np.asarray(ps.TRUE_POSES[0]) + [0.3, 0., -0.2, 0., 1.7, 0.])
XI_ODOM = [0.05, 0.01, 0., 0., 0., 0.03]
_CACHE = {}


def target_images():
    """uint8 [4][H][W]: the three plain targets and the remapped target 0"""
    t = ps.scene()["targets"]
    return np.concatenate([t, mr.remap(t[0])[None]])


def localizer():
    """the restatement with the four targets; base and packs are those of photometric_scene.localizer(), which stays as it is"""
    if "loc" not in _CACHE:
        loc0 = ps.localizer()
        loc = pr.Localizer(ps.CAM, ps.PRM, ps.XI_BASE_CAM, ps.NUM_SCALES)
        loc.base, loc.packs = loc0.base, loc0.packs
        loc.targets = list(loc0.targets) + [pr.pyramid(target_images()[REMAPPED], ps.NUM_SCALES, gradients=False)]
        _CACHE["loc"] = loc
    return _CACHE["loc"]


def eval_poses():
    """(poses [5][6], target index [5]): photometric_scene.eval_poses() and the pose at which projections fail"""
    poses, targets = ps.eval_poses()
    return np.concatenate([poses, [FAILING_POSE]]), np.concatenate([targets, [0]]).astype(np.int32)


def reference_evaluate(scale, i):
    """the restatement's evaluate_mi at eval pose i, cached"""
    key = ("eval", scale, i)
    if key not in _CACHE:
        poses, targets = eval_poses()
        _CACHE[key] = mr.evaluate_mi(localizer(), scale, poses[i], int(targets[i]))
    return _CACHE[key]


def reference_solve(target=0, factor=1., tight=True, odom=False):
    """the restatement's compute_pose_mi from start_pose(0, factor) against `target` (0 or REMAPPED), cached"""
    key = ("solve", target, factor, tight, odom)
    if key not in _CACHE:
        kw = TIGHT if tight else {}
        _CACHE[key] = mr.compute_pose_mi(localizer(), ps.start_pose(0, factor), target, XI_ODOM if odom else None, **kw)
    return _CACHE[key]
