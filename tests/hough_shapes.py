"""Inputs of the line detection shape tests (tests/test_gpu_hough_shapes.py, tests/test_hough_shapes_cpu.py): the smallest
images, cameras and parameters at which the detector's kernels take the paths that the six cases of tests/hough_scene.py leave
out -- accumulators that are not square, cameras that are not isotropic, every parameter at the ends of its range, a loaded
compaction, both line statuses, both reasons for dropping a candidate maximum, and the three threshold comparisons at equality.
Each case names the conditions (NEED) that the restatement (tests/hough_ref.py) must meet for the case to be live: conditions on
the case, not measurements.  Everything is built once per process and left unchanged; nothing here needs a GPU."""
import math

import numpy as np

from tests import hough_ref, hough_scene

LANES = 256   # bins per workgroup of the blur and of the maxima's compaction
MAX_LINES = 512   # above every case's count
NORMALS, STEPS, CAM = hough_scene.NORMALS, hough_scene.STEPS, hough_scene.CAM
ANISO_CAM = (0.57, 1.1, 62., 48., 77.3, 48.6)
WIDE, TALL = (0.5, 1., 34., 22., 70.6, 45.2), (0.5, 1., 22., 34., 45.2, 70.6)
EDGE = ((0.1, 1., 0.5),)   # one hard edge; its normal projects near the middle of the small accumulators
CROSS = ((0.1, 1., 0.05), (1., 0.2, 0.03))   # two hard edges through the image's centre: they reach all four borders
MANY = dict(search_size=1, blur_size=3, blur_sigma=0.6, acc_thresh=0.3, acc_delta_thresh=0., grad_thresh=0.0002)
QUARTERS_SIGMA = math.sqrt(0.5 / math.log(2.))   # the 3-tap Gaussian (1/4, 1/2, 1/4): every blurred value is exact

# name -> (width, height, camera, accumulator camera, normals, steps, softness, parameter overrides)
CASES = {
    # fu != fv in both cameras, u0 != v0, odd accumulator sides, wider than high and higher than wide
    "aniso": (150, 100, ANISO_CAM, WIDE, NORMALS, STEPS, 0.02, {}),
    "aniso_tall": (100, 150, (0.57, 1.1, 48., 62., 48.6, 77.3), TALL, NORMALS, STEPS, 0.02, {}),
    # the circle of the end points has the radii r fu, r fv, the one of distanceCheck sqrt(fu fv) r: lines of both statuses
    "no_end_points": (150, 100, (0.57, 1.6, 70., 40., 77.3, 48.6), WIDE, NORMALS, STEPS, 0.02, {}),
    # a loaded compaction: more than 256 blocks, more than 128 maxima, blocks with 3 and more of them
    "many_maxima": (160, 120, CAM, (0.5, 1., 75., 55., 150., 110.), NORMALS, STEPS, 0.02, MANY),
    "many_maxima_negative_delta": (160, 120, CAM, (0.5, 1., 75., 55., 150., 110.), NORMALS, STEPS, 0.02, dict(MANY, acc_delta_thresh=-0.25)),
    # the widest blur on a side of r + 1 = 8 bins; the widest search on a side of 2 s + 3 = 19 bins
    "blur15_min_side": (96, 64, (0.57, 1.1, 40., 40., 48., 32.), (0.5, 1., 2., 10., 4.2, 20.), EDGE, (200.,), 0.005,
                        dict(blur_size=15, blur_sigma=6., acc_thresh=1., acc_delta_thresh=0.)),
    "blur3_search8": (96, 64, (0.57, 1.1, 40., 40., 48., 32.), (0.5, 1., 5., 12., 9.6, 25.), EDGE, (200.,), 0.005,
                      dict(blur_size=3, blur_sigma=0.8, search_size=8, acc_thresh=1., acc_delta_thresh=0.)),
    # margin 1: one tile exactly, one pixel over a tile in both directions, the smallest image; a margin above a tile's height
    "margin1_one_tile": (64, 16, (0.57, 1.1, 30., 30., 31.5, 7.5), (0.5, 1., 8., 8., 20., 20.), CROSS, (100., 100.), 0.005,
                         dict(margin=1, acc_thresh=2.)),
    "margin1_ragged": (65, 17, (0.57, 1.1, 30., 30., 32., 8.), (0.5, 1., 8., 8., 20., 20.), CROSS, (100., 100.), 0.005,
                       dict(margin=1, acc_thresh=2.)),
    "min_image": (5, 5, (0.57, 1.1, 4., 4., 2., 2.), (0.5, 1., 3., 3., 8., 8.), ((0.3, 1., 0.1),), (200.,), 0.005,
                  dict(margin=1, acc_thresh=0.3, acc_delta_thresh=0.)),
    "margin_over_tile": (70, 60, (0.57, 1.1, 30., 30., 35., 30.), (0.5, 1., 8., 8., 20., 20.), NORMALS, STEPS, 0.02,
                         dict(margin=20, acc_thresh=2.)),
    # every voting pixel casts its antipode (some fail beyond the horizon of an accumulator camera with alpha > 0.5); none does
    "horizon_all": (160, 120, CAM, (0.62, 1., 30., 30., 64., 64.), NORMALS, STEPS, 0.02, dict(horizon_ratio=1e30)),
    "horizon_none": (160, 120, CAM, hough_scene.ACC, NORMALS, STEPS, 0.02, dict(horizon_ratio=0.)),
    "horizon_negative": (160, 120, CAM, hough_scene.ACC, NORMALS, STEPS, 0.02, dict(horizon_ratio=-1.)),
    # a candidate maximum among the antipode votes beyond the accumulator camera's horizon: its reconstruction has n[2] < 0
    # (alpha 0.62), or fails because the centroid lies past the circle det = 0 on which the projection ends (alpha 0.7)
    "behind": (96, 64, (0.57, 1.1, 30., 30., 48., 32.), (0.62, 1., 12., 12., 32., 32.), ((0.1, 1., 0.4),), (200.,), 0.005,
               dict(horizon_ratio=1e30, acc_thresh=2.)),
    "behind_not_reconstructed": (96, 64, (0.57, 1.1, 30., 30., 48., 32.), (0.7, 1., 12., 12., 32., 32.), ((0.1, 1., 0.4),), (200.,), 0.005,
                                 dict(horizon_ratio=1e30, acc_thresh=2.)),
}
# An image that is its own mirror image in u (u0 = (width - 1) / 2, one edge with A = 0) votes mirror images about the accumulator's
# u0 = 24.5, between bins 24 and 25; with the blur (1/4, 1/2, 1/4) every sum is exact, so the two bins of the peak are equal.
TIE = (96, 64, (0.57, 1.1, 40., 40., 47.5, 32.), (0.5, 1., 8., 8., 24.5, 24.), ((0., 1., 0.3),), (200.,), 0.005,
       dict(blur_size=3, blur_sigma=QUARTERS_SIGMA, acc_thresh=2., acc_delta_thresh=0.))

# What the restatement must show for a case to be live (tests/test_hough_shapes_cpu.py asserts every entry):
#   acc (acc_w, acc_h); blocks_over / lines_over n: more than n; blocks_with_3 n: at least n blocks of 256 bins hold 3 maxima or more;
#   statuses: the set of line statuses; positive: counters above 0; lines / inside: at least one line / one vote in the accumulator;
#   antipode all / none; window_dropped: (behind, not_reconstructed) are exactly these; empty_tiles: tiles of 64 x 16 without a
#   visited pixel
NEED = {
    "aniso": dict(acc=(141, 90), positive=("antipode_votes", "outside"), lines=True),
    "aniso_tall": dict(acc=(90, 141), positive=("antipode_votes", "outside"), lines=True),
    "no_end_points": dict(acc=(141, 90), statuses={0, 1}),
    "many_maxima": dict(acc=(300, 220), blocks_over=256, lines_over=128, blocks_with_3=5),
    "many_maxima_negative_delta": dict(acc=(300, 220), blocks_over=256, lines_over=128, blocks_with_3=5),
    "blur15_min_side": dict(acc=(8, 40), inside=True, lines=True),
    "blur3_search8": dict(acc=(19, 50), inside=True, lines=True),
    "margin1_one_tile": dict(inside=True, lines=True, border_selected=True),
    "margin1_ragged": dict(inside=True, lines=True, border_selected=True),
    "min_image": dict(inside=True, lines=True, border_selected=True),
    "margin_over_tile": dict(inside=True, lines=True, empty_tiles=6),
    "horizon_all": dict(antipode="all", positive=("failed_projections",), lines=True),
    "horizon_none": dict(antipode="none", lines=True),
    "horizon_negative": dict(antipode="none", lines=True),
    "behind": dict(window_dropped=(1, 0), lines=True),
    "behind_not_reconstructed": dict(window_dropped=(0, 1), lines=True),
    "equal_grad": dict(lines=True),
    "equal_acc": dict(lines=True),
    "tie": dict(acc=(49, 48), inside=True),
    "tie_broken": dict(acc=(49, 48), lines=True),
}

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _frozen(a):
    a.setflags(write=False)
    return a


def _table(spec):
    w, h, cam, acc, normals, steps, softness, over = spec
    return _frozen(hough_scene.image(w, h, cam, normals, steps, softness)), np.array(cam), np.array(acc), hough_ref.params(**over)


def grad_at_equality():
    """(grad_thresh, pixels at equality): the value k / 2^22, exact in double, of the integer k = kx^2 + ky^2 that the most visited
    pixels of "aniso" have among the 20 smallest values at or above the default threshold (the smallest such k on a draw)"""
    img, _, _, prm = case("aniso")
    kx, ky = hough_ref.sobel(img)
    m = prm["margin"]
    k = (kx * kx + ky * ky)[m:img.shape[0] - m, m:img.shape[1] - m].ravel()
    values, n = np.unique(k[k / 4194304. >= prm["grad_thresh"]], return_counts=True)
    values, n = values[:20], n[:20]
    best = int(np.argmax(n))   # the first of equal counts: the smallest k
    return int(values[best]) / 4194304., int(n[best])


def acc_at_equality():
    """(acc_thresh, bin): the float value, as a double, of the lowest maximum of "aniso" and its raster position"""
    st = stats("aniso")
    ref = reference("aniso")
    j = int(np.argmin(ref["lines"][:, 2]))
    return float(ref["lines"][j, 2]), st["bins"][j]


def tie_delta():
    """the acc_delta_thresh one double below zero at the tied peak's value: peak + delta is the double below the peak"""
    peak = float(reference("tie")["blur"].max())
    return -(math.nextafter(peak, math.inf) - peak)


DERIVED = {
    "equal_grad": lambda: case("aniso")[:3] + (dict(case("aniso")[3], grad_thresh=grad_at_equality()[0]),),
    "equal_acc": lambda: case("aniso")[:3] + (dict(case("aniso")[3], acc_thresh=acc_at_equality()[0]),),
    "tie": lambda: _table(TIE),
    "tie_broken": lambda: case("tie")[:3] + (dict(case("tie")[3], acc_delta_thresh=tie_delta()),),
}
NAMES = sorted(list(CASES) + list(DERIVED))
assert set(NAMES) == set(NEED)


def case(name):
    """(image u8 [height, width], camera, accumulator camera, parameters) of a case; built once"""
    return cached(("case", name), lambda: _table(CASES[name]) if name in CASES else DERIVED[name]())


def with_params(name, **over):
    """the case with some parameters replaced (for the boundary proofs): not cached"""
    img, cam, acc, prm = case(name)
    return img, cam, acc, dict(prm, **over)


def _detect(name):
    st = {}
    return hough_ref.detect(*case(name), st), st


def reference(name):
    """the restatement's result for a case (hough_ref.detect), computed once and shared: do not modify"""
    return cached(("ref", name), lambda: _detect(name))[0]


def stats(name):
    """what hough_ref.vote and hough_ref.maxima report about the case: see there"""
    return cached(("ref", name), lambda: _detect(name))[1]


def blocks_of(n):
    return (n + LANES - 1) // LANES


def maxima_per_block(name):
    """the number of maxima in every block of 256 bins of the case's accumulator"""
    aw, ah = hough_ref.acc_size(case(name)[2])
    return np.bincount(np.array(stats(name)["bins"], dtype=np.int64) // LANES, minlength=blocks_of(aw * ah))


def cut_inside_a_block(name):
    """a max_lines that cuts between two maxima of one block: one more than the lines up to the first maximum of the fullest block"""
    bins = np.array(stats(name)["bins"], dtype=np.int64)
    block = int(np.argmax(maxima_per_block(name)))
    first = int(np.searchsorted(bins // LANES, block))
    assert bins[first] // LANES == bins[first + 1] // LANES == block
    return first + 1


# ---- the mixed batch: items of very different counts on one handle (size, cameras and parameters of "many_maxima")
BATCH = ("many_maxima", "blank", "flipped", "many_maxima")


def batch_image(item):
    img = case("many_maxima")[0]
    if item == "blank":
        return cached(("img", item), lambda: _frozen(np.full_like(img, 30)))
    if item == "flipped":
        return cached(("img", item), lambda: _frozen(np.ascontiguousarray(img[::-1, ::-1])))
    return img


def batch_reference(item):
    """the restatement on one item of the batch, computed once"""
    if item == "many_maxima":
        return reference(item)
    return cached(("batch", item), lambda: hough_ref.detect(batch_image(item), *case("many_maxima")[1:]))
