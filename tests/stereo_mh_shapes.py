"""Inputs of the multi-hypothesis shape tests (tests/test_gpu_stereo_mh_shapes.py, tests/test_stereo_mh_shapes_cpu.py): hand-made
hypothesis maps at the sizes where the launches of vg_depth_pack_mh and vg_depth_regularize change shape, and the stereo cases
that reach what tests/test_gpu_stereo_mh.py leaves out of vg_stereo_compute_mh.  Everything is built once per process and left
unchanged; nothing here needs a GPU.

A  maps for the pack, on stereo_scene.CAM1 at scale 1: small(P, fill) of 1 ... 513 pixels, blocks(w, h) of 256, 257 and 520
   workgroups with a density that changes from workgroup to workgroup, full(), patterns(), values(), hand_made().
B  maps for regularize: exhaustive(K), every pattern of K planes over {0, 0.1, filled}; regularize_values(); random_map().
C  stereo: the restatement of strip and rig cases at other K and hypo_difference, and the cost-0 rig."""
import math

import numpy as np

from tests import stereo_mh_ref as smh
from tests import stereo_ref as sr
from tests import stereo_scene
from tests import stereo_strip as strip
from tests.test_gpu_stereo import BASE, EPIPOLE_MARGIN

LANES = 256                      # pixels per workgroup of the pack and of regularize
CAM = stereo_scene.CAM1
BELOW = math.nextafter(smh.MIN_DEPTH, 0.)
NAN = float("nan")
SMALL = {1: (1, 1), 63: (63, 1), 64: (64, 1), 65: (65, 1), 255: (255, 1), 256: (256, 1), 257: (257, 1), 259: (7, 37), 513: (27, 19)}
FILLS = ("random", "last", "first")
BLOCK_SHAPES = ((256, 256), (257, 256), (416, 320))   # (width, height): 256, 257 and 520 workgroups, scan runs of 1, 2 and 3
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def blocks_of(n):
    return (n + LANES - 1) // LANES


def grid(w, h, u0=0, v0=0, scale=1):
    return {"scale": scale, "u0": u0, "v0": v0, "x_max": w, "y_max": h, "u_max": max(w, 1), "v_max": max(h, 1)}


def distinct(shape, first=1.):
    """a value per element that no other element has, exact in float64"""
    return first + np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) / 2. ** 22


# ---- the pack's rule, vectorised -------------------------------------------------------------------------------------

def directions(cam, prm):
    """(dir [P][3], seen [P], det [P]): sr.reconstruct(...) normalised, per pixel in raster order, in its order of operations"""
    alpha, beta, fu, fv, cu, cv = cam
    yy, xx = np.mgrid[0:prm["y_max"], 0:prm["x_max"]]
    u = (xx.ravel() * prm["scale"] + prm["u0"]).astype(np.float64)
    v = (yy.ravel() * prm["scale"] + prm["v0"]).astype(np.float64)
    xn = (u - cu) / fu
    yn = (v - cv) / fv
    u2 = xn * xn + yn * yn
    gamma = 1. - alpha
    num = 1. - u2 * alpha * alpha * beta
    det = 1 - (alpha - gamma) * beta * u2
    seen = ~(det < 0)
    z = num / (gamma + alpha * np.sqrt(np.where(seen, det, 0.)))
    nrm = np.sqrt(xn * xn + yn * yn + z * z)
    return np.stack([xn / nrm, yn / nrm, z / nrm], 1), seen, det


def pack_fast(cam, prm, depth, sigma):
    """smh.pack_mh without its pixel loop: pixel-major, planes ascending, one direction per pixel"""
    H = depth.shape[0]
    d, s = depth.reshape(H, -1), sigma.reshape(H, -1)
    P = d.shape[1]
    with np.errstate(invalid="ignore"):
        keep = (d >= smh.MIN_DEPTH) & (d[0] >= smh.MIN_DEPTH)[None]
    pix, hyp = np.nonzero(keep.T)   # row-major over [P][H]: pixels ascending, planes ascending within a pixel
    dirs, seen, _ = directions(cam, prm)
    cloud = np.where(seen[pix, None], dirs[pix] * d[hyp, pix][:, None], 0.)
    assert P == prm["x_max"] * prm["y_max"]
    return pix.astype(np.int32), hyp.astype(np.int32), cloud, s[hyp, pix]


def entries_per_block(idx, P):
    """entries of a pack per workgroup of 256 pixels: what the first pass hands to the scan"""
    return np.bincount(np.asarray(idx) // LANES, minlength=blocks_of(P))


# ---- A: maps for the pack --------------------------------------------------------------------------------------------

def small(P, fill, K=4):
    """(prm, depth [K][h][w], sigma): random from {0, 0.1, 0.25, 1, 3}, or one pixel with all its planes filled"""
    def make():
        w, h = SMALL[P]
        rng = np.random.default_rng(100 + P)
        if fill == "random":
            depth = rng.choice([0., 0.1, 0.25, 1., 3.], size=(K, h, w))
            if P == 1:
                depth[0] = 1.   # the single pixel is a query
        else:
            depth = np.zeros((K, h, w))
            depth.reshape(K, -1)[:, -1 if fill == "last" else 0] = [1.5, 0.25, 2., 3.][:K]
        return grid(w, h), depth, distinct(depth.shape)
    return cached(("small", P, fill, K), make)


def blocks(w, h, K=8):
    """(prm, depth [K][h][w], sigma) over w h / 256 workgroups.  Plane 0 is filled with a probability that is one of 0, 0.03, 0.5,
    1 per workgroup (and 0 on a fifth of the 64-pixel waves of the others); the planes above are filled on half of all pixels,
    whether plane 0 is or not.  u0, v0 put camera 1's principal point at pixel (162.5, 126.5), so that the pixels further than
    about 135 px from it, which the camera refuses, and the others both occur."""
    def make():
        P = w * h
        rng = np.random.default_rng(7 * w + h)
        nb = blocks_of(P)
        density = np.repeat(rng.choice([0., 0.03, 0.5, 1.], size=nb), LANES)[:P]
        wave_off = np.repeat(rng.random(blocks_of(P) * 4) < 0.2, 64)[:P]
        filled = rng.random((K, P)) < 0.5
        filled[0] = (rng.random(P) < density) & ~wave_off
        depth = np.where(filled, rng.uniform(0.25, 6., (K, P)), rng.choice([0., 0.1, BELOW], size=(K, P)))
        return grid(w, h, -100, -80), depth.reshape(K, h, w), distinct((K, h, w))
    return cached(("blocks", w, h, K), make)


def full():
    """257 x 3 with all 8 planes of every pixel filled: 2048 entries in every full workgroup"""
    def make():
        shape = (8, 3, 257)
        return grid(257, 3), distinct(shape, 0.25), distinct(shape, 9.)
    return cached("full", make)


def patterns():
    """40 x 15: pixel p holds the fill pattern (p + 37) % 256, plane h filled where bit h is set -- every pattern of 8 planes,
    more than twice, with other patterns either side of the workgroup boundaries at 256 and 512"""
    def make():
        shape = (8, 15, 40)
        pat = (np.arange(600) + 37) % 256
        filled = (pat[None, :] >> np.arange(8)[:, None]) & 1 == 1
        depth = np.where(filled, distinct((8, 600), 0.5), 0.)
        return grid(40, 15, 30, 20), depth.reshape(shape), distinct(shape, 9.), pat
    return cached("patterns", make)


# per pixel: its three planes, and the planes that give an entry
VALUE_PIXELS = [([0.25, BELOW, 1.], [0, 2]), ([BELOW, 1., 1.], []), ([-1., 2., 2.], []), ([1., -3., 0.25], [0, 2]),
                ([NAN, 1., 1.], []), ([1., NAN, 2.], [0, 2]), ([1., 1., NAN], [0, 1]), ([-0., 1., 1.], []), ([0.25, 0.25, 0.25], [0, 1, 2])]


def values():
    """(prm, depth [3][1][9], sigma, entries [(pixel, plane)]): exactly MIN_DEPTH, the double below it, negative depths, NaN"""
    def make():
        depth = np.array([p for p, _ in VALUE_PIXELS]).T.reshape(3, 1, -1).copy()
        entries = [(i, h) for i, (_, hs) in enumerate(VALUE_PIXELS) for h in hs]
        return grid(len(VALUE_PIXELS), 1, 40, 30), depth, distinct(depth.shape), entries
    return cached("values", make)


HAND_CAM = [0.6, 1., 100., 10., 0., 0.]


def hand_made():
    """the 2 x 2 map of tests/test_stereo_mh_cpu.py test_pack_hand_made_map: scale 30, row 1 is refused by the camera"""
    depth = np.array([[[2., 3.], [0.2, 1.]], [[0.1, 4.], [5., 0.25]]])
    return grid(2, 2, scale=30), depth, np.arange(8.).reshape(2, 2, 2)


def one_entry(w, h, K=8):
    """a map of blocks()'s shape with a single entry, in the middle of it"""
    depth = np.zeros((K, h, w))
    depth[0, h // 2, w // 2] = 2.
    return depth


# ---- B: maps for regularize ------------------------------------------------------------------------------------------

def exhaustive(K):
    """(depth, sigma, cost) [K][1][3^K]: pixel p holds the base-3 digits of p, plane h its digit h: 0 -> 0, 1 -> 0.1, 2 -> a
    depth of its own; sigma and cost differ at every (plane, pixel)"""
    def make():
        P = 3 ** K
        digit = (np.arange(P)[None, :] // 3 ** np.arange(K)[:, None]) % 3
        depth = np.choose(digit, [np.zeros((K, P)), np.full((K, P), 0.1), distinct((K, P), 0.5)])
        return depth.reshape(K, 1, P), distinct((K, 1, P), 100.), np.arange(K * P, dtype=np.float64).reshape(K, 1, P)
    return cached(("exhaustive", K), make)


# per pixel: its three planes before and after (a NaN depth is not below MIN_DEPTH: it counts as filled and stays or moves)
REGULARIZE_PIXELS = [([BELOW, 0.25, 1.], [0.25, 1., 0.]), ([-1., 0., 2.], [2., 0., 0.]), ([NAN, 0., 3.], [NAN, 3., 0.]),
                     ([0., NAN, 3.], [NAN, 3., 0.]), ([0.25, BELOW, -2.], [0.25, BELOW, -2.]), ([-0., -5., 0.25], [0.25, -5., 0.]),
                     ([0.1, BELOW, NAN], [NAN, BELOW, 0.])]


def regularize_values():
    """(depth, sigma, cost) [3][1][7] and the depth planes expected, by hand"""
    def make():
        depth = np.array([p for p, _ in REGULARIZE_PIXELS]).T.reshape(3, 1, -1).copy()
        want = np.array([q for _, q in REGULARIZE_PIXELS]).T.reshape(3, 1, -1).copy()
        return depth, distinct(depth.shape, 100.), distinct(depth.shape, 7.), want
    return cached("regularize_values", make)


def random_map(P, K, n=None):
    """(depth, sigma, cost) [K][h][w], or [n][K][h][w], of one of SMALL's shapes, depths from {0, 0.1, 0.25, 1, 3}"""
    def make():
        w, h = SMALL[P]
        shape = (K, h, w) if n is None else (n, K, h, w)
        depth = np.random.default_rng(1000 * K + P).choice([0., 0.1, 0.25, 1., 3.], size=shape)
        return depth, distinct(shape, 100.), distinct(shape, 7.)
    return cached(("random_map", P, K, n), make)


def bits(a):
    """the array's bit patterns, so that NaN compares like any other value"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- C: stereo -------------------------------------------------------------------------------------------------------

RIG = "sideways"
ZERO_XI = [0.2, 0., 0., 0., 0., 0.]          # the cost-0 rig: camera 1 twice, a pure sideways baseline
STRIP_K = (3, 5, 6, 7)                       # on case j at hypo_difference 200
DISP_MAX_CASES = ((4, 4), (8, 8))            # (disp_max, K) on the rig at hypo_difference 1 000 000
DIFF_CASES = (0, -1, 1000000)                # on case a, K = 3
CHUNK_PRM = dict(strip.BASE, disp_max=256, use_uv_cache=1, v0=4, y_max=40)


def rig_scene():
    return cached("rig_scene", lambda: stereo_scene.make_scene(RIG))


def rig_prm(**kw):
    return dict(BASE, epipole_margin=EPIPOLE_MARGIN[RIG], **kw)


def rig_reference(hyp, diff, **kw):
    """(single-hypothesis restatement, multi-hypothesis restatement) of the sideways rig"""
    key = tuple(sorted(kw.items()))
    img1, img2, _, xi = rig_scene()
    prm = sr.params(**rig_prm(**kw))
    base = cached(("rig_base", key), lambda: sr.stereo(stereo_scene.CAM1, stereo_scene.CAM2, xi, prm, img1, img2))
    return base, cached(("rig_mh", key, hyp, diff),
                        lambda: smh.stereo_mh(stereo_scene.CAM1, stereo_scene.CAM2, xi, prm, img1, img2, hyp, diff, base=base))


def zero_reference(hyp, diff):
    """the same for the cost-0 rig: img1 against itself through two cameras CAM1, so that disparity 0 is the same pixel"""
    img1 = rig_scene()[0]
    prm = sr.params(**rig_prm())
    base = cached("zero_base", lambda: sr.stereo(CAM, CAM, ZERO_XI, prm, img1, img1))
    return base, cached(("zero_mh", hyp, diff), lambda: smh.stereo_mh(CAM, CAM, ZERO_XI, prm, img1, img1, hyp, diff, base=base))


def strip_reference(name, hyp, diff):
    """(img1, img2, single-hypothesis restatement, multi-hypothesis restatement) of a case of tests/stereo_strip.py"""
    img1, img2, base = strip.reference(name)
    xi = strip.images(*strip.CASES[name][:2])[3]
    mh = cached(("strip_mh", name, hyp, diff), lambda: smh.stereo_mh(strip.S["cam1"], strip.S["cam2"], xi, sr.params(**strip.prm_of(name)),
                                                                     img1, img2, hyp, diff, base=base))
    return img1, img2, base, mh


def tie_pixels(base, mh, error_max):
    """pixels where an accepted hypothesis has three or more candidates of its cost"""
    n = 0
    Y, X, _ = base["err"].shape
    for y in range(Y):
        for x in range(X):
            if mh["disparity"][1, y, x] < 0:
                continue
            costs = [c for c, _ in smh.candidates(base["err"][y, x], base["total"][y, x], error_max)]
            taken = mh["final_cost"][:, y, x][mh["disparity"][:, y, x] >= 0]
            n += any(costs.count(int(c)) >= 3 for c in taken)
    return n


def rig_pairs():
    """three pairs of rig images for a batch: the scene's, the same with the rows reversed, and the two images swapped"""
    img1, img2 = rig_scene()[:2]
    return np.stack([img1, img1[::-1], img2]), np.stack([img2, img2[::-1], img1])


def rig_pair_reference(i, hyp, diff):
    """the multi-hypothesis restatement of pair i of rig_pairs()"""
    a, b = rig_pairs()
    xi = rig_scene()[3]
    prm = sr.params(**rig_prm())
    base = cached(("pair_base", i), lambda: sr.stereo(stereo_scene.CAM1, stereo_scene.CAM2, xi, prm, a[i], b[i]))
    return cached(("pair_mh", i, hyp, diff), lambda: smh.stereo_mh(stereo_scene.CAM1, stereo_scene.CAM2, xi, prm, a[i], b[i], hyp, diff, base=base))
