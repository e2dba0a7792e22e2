"""The key-frame test sequence on tests/stereo_scene.py's planes, ONE camera throughout (the reference's mapping loop warps
within one camera): the key frame is CAM1 at the origin and the further views are CAM1 at the rig's second pose and at the four
poses of tests/motion_scene.py.  The loop of the tests: SGM on the first pair, two motion stereo steps, a key-frame switch at
the fourth view, one more motion stereo step in the new frame, with filterNoise where the reference's mapping loop runs it
(after every SGM or motion stereo update, and on the switch's SGM map)."""
import numpy as np

from tests import depth_ref as dr
from tests import motion_ref as mr
from tests import motion_scene as ms
from tests import stereo_ref as sr
from tests import stereo_scene

CAM = stereo_scene.CAM1
KEY_INDEX = 4   # the view that becomes the key frame
_VIEWS = {}
# warp poses of the depth fusion tests, one per regime: [t, rotvec] of the new frame in the old
WARP_POSES = {
    "sideways": [0.2, 0.004, -0.003, 0.004, -0.006, 0.01],
    "backward": [0.01, -0.02, -0.45, -0.004, 0.006, 0.003],   # the camera retreats: many sources share a target
    "forward": [0.03, 0.02, 0.25, 0.003, -0.004, 0.002],      # the camera advances: the map spreads and leaves holes
}


def rot(xi):
    return np.array(sr.rotation_matrix([float(v) for v in xi[3:]], 1.)).reshape(3, 3)


def view(xi):
    """the u8 image of CAM at pose xi (in the first key frame)"""
    key = tuple(float(v) for v in xi)
    if key not in _VIEWS:
        _VIEWS[key] = stereo_scene.render(CAM, rot(xi), np.array(key[:3]), 125, 93)
    return _VIEWS[key]


def true_range(xi, prm):
    """the true range along CAM's rays at pose xi of every depth pixel of the grid `prm`, 0 where no plane is hit"""
    yy, xx = np.mgrid[0:prm["y_max"], 0:prm["x_max"]]
    d = stereo_scene.reconstruct_np(CAM, (xx * prm["scale"] + prm["u0"]).astype(float), (yy * prm["scale"] + prm["v0"]).astype(float))
    lam = stereo_scene.cast(np.array([float(v) for v in xi[:3]]), d @ rot(xi).T)
    rng = lam * np.linalg.norm(d, axis=-1)
    return np.where(np.isfinite(rng), rng, 0.)


def sequence(rig):
    """(images, poses): the key frame and five views; poses[i] is view i in the first key frame (poses[0] the identity)"""
    poses = [[0.] * 6, list(stereo_scene.RIGS[rig])] + ms.poses(rig)
    return [view(q) for q in poses], poses


def stat(dep, rng):
    """median relative range error, share of the pixels with a depth and a true range, their number"""
    m = (dep > 0) & (rng > 0)
    return float(np.median(np.abs(dep[m] - rng[m]) / rng[m])), float(m.mean()), int(m.sum())


class RefOps:
    """the loop's operations on the restatements; maps are (depth, sigma, cost) numpy triples"""

    def __init__(self, prm):
        self.prm = prm
        self.M = mr.MotionStereo(CAM, CAM, prm)

    def set_base(self, img):
        self.M.set_base(img)

    def sgm(self, img1, img2, xi):
        r = sr.stereo(CAM, CAM, xi, self.prm, img1, img2)
        return r["depth"], r["sigma"], r["cost"]

    def motion(self, xi, img, maps):
        r = self.M.compute(xi, img, maps)
        return r["depth"], r["sigma"], r["cost"]

    def filter_noise(self, maps):
        r = dr.filter_noise(maps[0], maps[1])
        return r["depth"], r["sigma"], maps[2]

    def warp(self, xi, maps):
        r = dr.warp(CAM, self.prm, xi, *maps)
        return r["depth"], r["sigma"], r["cost"]

    def merge(self, maps, maps2):
        r = dr.merge(maps[0], maps[1], maps2[0], maps2[1])
        return r["depth"], r["sigma"], maps[2]


def run_loop(ops, images, poses, pose_in_frame, pose_inverse):
    """the loop on `ops` (RefOps or the GPU's): the maps after every view, [(depth, sigma, cost)] * 5.  The two pose
    functions are the library's (the poses are inputs of the loop, not part of what is compared)."""
    out = []
    ops.set_base(images[0])
    cur = ops.filter_noise(ops.sgm(images[0], images[1], poses[1]))
    out.append(cur)
    for i in (2, 3):
        cur = ops.filter_noise(ops.motion(poses[i], images[i], cur))
        out.append(cur)
    base = poses[KEY_INDEX]   # pushInterFrame
    new = ops.filter_noise(ops.sgm(images[KEY_INDEX], images[0], pose_inverse(base)))
    cur = ops.merge(ops.warp(base, cur), new)
    ops.set_base(images[KEY_INDEX])
    out.append(cur)
    cur = ops.filter_noise(ops.motion(pose_in_frame(base, poses[5]), images[5], cur))
    out.append(cur)
    return out


def synthetic_maps(prm, seed=5):
    """two (depth, sigma, cost) triples on the grid `prm` that reach every branch of merge and filterNoise: the true range
    with noise and holes; and a second map with holes, values below MIN_DEPTH, much nearer and much farther values"""
    rnd = np.random.default_rng(seed)
    rng0 = true_range([0.] * 6, prm)
    shape = rng0.shape
    d1 = rng0 * (1. + 0.01 * rnd.standard_normal(shape))
    d1[rnd.random(shape) < 0.35] = 0.                        # holes: isolated pixels and pixels with one neighbour arise
    d1[rnd.random(shape) < 0.05] *= 1.5                      # outliers the filter clears
    s1 = rnd.uniform(0.01, 0.05, shape)
    c1 = rnd.integers(0, 150, shape).astype(np.float64)
    d2 = rng0 * (1. + 0.01 * rnd.standard_normal(shape))
    pick = rnd.random(shape)
    d2[pick < 0.2] = 0.
    d2[(pick >= 0.2) & (pick < 0.25)] = 0.1                  # below MIN_DEPTH
    d2[(pick >= 0.25) & (pick < 0.35)] *= 0.5                # nearer: replaces
    d2[(pick >= 0.35) & (pick < 0.45)] *= 2.                 # farther: map 1 kept
    s2 = rnd.uniform(0.01, 0.05, shape)
    c2 = rnd.integers(0, 150, shape).astype(np.float64)
    return (d1, s1, c1), (d2, s2, c2)
