"""Inputs of the localization shape tests (tests/test_gpu_localization_shapes.py, tests/test_localization_shapes_cpu.py): the
scene of tests/photometric_scene.py at the sizes where the launches of vg_photometric.hpp and vg_photometric_mi.hpp change
shape, each with the restatement's Localizer on it, built once per process and left unchanged.

A  scaled(w, h): the scene with its camera scaled to the width, two scales, at 256 x 256, 257 x 256 and 416 x 320: 256, 257 and
   520 workgroups of 256 pixels at level 0, so that the scan of the block counts runs with chunks of 1, 2 and 3.
B  exact(m): 256 x 192, one scale, one depth cell per pixel, the depth kept at exactly m pixels whose points all evaluate
   inside the margin at POSE_B: packs of exactly m points.
C  noise(): a 384 x 256 noise image for eight pyramid levels.
D  OUTSIDE_POSES: rotations of 0.6 rad that carry a part of the cloud beyond every side of the target image."""
import numpy as np

from tests import photometric_ref as pr
from tests import photometric_scene as ps
from tests import stereo_scene

LANES = 256                                     # pixels, and points, per workgroup
SHAPES = ((256, 256), (257, 256), (416, 320))   # A: (width, height)
SCALES_A = 2
EXACT_SIZES = (1, 63, 64, 65, 255, 256, 257, 512, 1024)   # B
PRM_B = {"scale": 1, "u0": 0, "v0": 0, "x_max": ps.W, "y_max": ps.H}
POSE_B = ps.start_pose(0)                       # photometric_scene.eval_poses()[0][1]
NOISE_W, NOISE_H, NOISE_SCALES = 384, 256, 8    # C: level 7 is 3 x 2
_TURN = 0.6
OUTSIDE_POSES = np.array([np.asarray(ps.TRUE_POSES[0]) + d for d in ([0, 0, 0, _TURN, 0, 0], [0, 0, 0, -_TURN, 0, 0],
                                                                     [0, 0, 0, 0, _TURN, 0], [0, 0, 0, 0, -_TURN, 0])])
_CACHE = {}


def blocks_of(n):
    return (n + LANES - 1) // LANES


def block_counts(idx, pixels):
    """points of a pack per workgroup of 256 pixels of its level: what the first selection pass hands to the scan"""
    return np.bincount(np.asarray(idx) // LANES, minlength=blocks_of(pixels))


# ---- A -------------------------------------------------------------------------------------------------------------

def camera(w, h):
    f = w / 256.
    return [ps.CAM[0], ps.CAM[1], ps.CAM[2] * f, ps.CAM[3] * f, w / 2., h / 2.]


def grid(w, h):
    return {"scale": 2, "u0": 16, "v0": 16, "x_max": (w - 32) // 2 + 1, "y_max": (h - 32) // 2 + 1}


def scaled(w, h):
    """dict(cam, prm, base u8 [h][w], target u8 [h][w] at TRUE_POSES[0], depth [y_max][x_max] with photometric_scene's holes,
    far and near values, loc: the Localizer with SCALES_A scales)"""
    key = ("scaled", w, h)
    if key not in _CACHE:
        cam, prm = camera(w, h), grid(w, h)
        base = stereo_scene.render(cam, np.eye(3), np.zeros(3), w, h)
        target = stereo_scene.render(cam, *ps.camera_pose(ps.TRUE_POSES[0]), w, h)
        depth = stereo_scene.true_range(cam, prm["u0"], prm["v0"], prm["x_max"], prm["y_max"], prm["scale"])
        pick = np.random.default_rng(11).random(depth.shape)
        depth[pick < 0.03] = 0.                          # OUT_OF_RANGE
        depth[(pick >= 0.03) & (pick < 0.05)] = 60.      # beyond DIST_MAX
        depth[(pick >= 0.05) & (pick < 0.06)] = 0.1      # below MIN_DEPTH
        loc = pr.Localizer(cam, prm, ps.XI_BASE_CAM, SCALES_A)
        loc.set_base(base, depth)
        loc.set_targets([target])
        _CACHE[key] = {"cam": cam, "prm": prm, "base": base, "target": target, "depth": np.ascontiguousarray(depth), "loc": loc}
    return _CACHE[key]


def poses_a():
    """the truth, the start pose, the start offset taken the other way, and the truth turned by -0.4 rad about x.  A pack is in
    raster order, so near the truth its last workgroup of points lies in the bottom margin and adds zeros to every sum; the turn
    lifts those points into the interior, and the last partial sum of the second pass counts."""
    return np.array([ps.TRUE_POSES[0], ps.start_pose(0), ps.start_pose(0, -0.7), np.asarray(ps.TRUE_POSES[0]) + [0, 0, 0, -0.4, 0, 0]], float)


# ---- B -------------------------------------------------------------------------------------------------------------

def full_depth():
    """the true range at every pixel of the 256 x 192 scene"""
    if "full" not in _CACHE:
        _CACHE["full"] = np.ascontiguousarray(stereo_scene.true_range(ps.CAM, 0, 0, ps.W, ps.H, 1))
    return _CACHE["full"]


def _localizer_b(depth):
    s = ps.scene()
    loc = pr.Localizer(ps.CAM, PRM_B, ps.XI_BASE_CAM, 1)
    loc.set_base(s["base"], depth)
    loc.set_targets([s["targets"][0]])
    return loc


def full_localizer():
    if "full_loc" not in _CACHE:
        _CACHE["full_loc"] = _localizer_b(full_depth())
    return _CACHE["full_loc"]


def inside_pixels():
    """the pixels of the full level-0 pack whose points evaluate inside the margin at POSE_B, in pack order"""
    if "inside" not in _CACHE:
        loc = full_localizer()
        state = loc.evaluate(0, POSE_B, 0, want_jac=False)["state"]
        _CACHE["inside"] = loc.packs[0]["idx"][state == 0]
    return _CACHE["inside"]


def exact(m):
    """dict(depth [H][W]: the full depth at a run of m of inside_pixels() from the middle of that list and 0 elsewhere, loc)"""
    key = ("exact", m)
    if key not in _CACHE:
        pix = inside_pixels()
        first = (len(pix) - m) // 2
        depth = np.zeros_like(full_depth())
        keep = pix[first:first + m]
        depth.flat[keep] = full_depth().flat[keep]
        _CACHE[key] = {"depth": depth, "loc": _localizer_b(depth)}
    return _CACHE[key]


# ---- C -------------------------------------------------------------------------------------------------------------

def noise(seed=0):
    return np.random.default_rng(21 + seed).integers(0, 256, (NOISE_H, NOISE_W), dtype=np.uint8)


# ---- D -------------------------------------------------------------------------------------------------------------

def outside_projection(scale, xi):
    """(u, v, ok) of photometric_scene's pack of `scale` under pose xi, in level-0 pixels, by pr.project"""
    loc = ps.localizer()
    xc = pr.compose(xi, loc.xbc)
    X = (loc.packs[scale]["cloud"] - xc[:3]) @ pr.rotation_matrix(-xc[3:]).T
    pt, ok = pr.project(loc.cam, X)
    return pt[:, 0], pt[:, 1], ok
