"""Images with known lines for the line detection tests: every great circle n . X = 0 of the viewing sphere is a soft step edge
in an EUCM image, img = 30 + sum_i step_i clip(d_i / softness + 0.5, 0, 1) with d_i = n_i . X / |X| the sine of the ray's angle
to plane i, rounded half to even; a pixel that does not reconstruct is 0.  The cases are the smallest shapes at which each
branch of the vote is live; the counts in the comments are those of tests/hough_ref.py."""
import math

import numpy as np

from tests import hough_ref

NORMALS = ((0.9, 0.1, 0.3), (-0.2, 1., 0.15), (0.5, -0.6, 0.7), (0.02, 0.03, 1.), (1., 0.4, 0.01))
STEPS = (40., 45., 50., 35., 40.)

CAM = (0.57, 1.1, 60., 60., 80., 60.)
ACC = (0.5, 1., 30., 30., 64., 64.)

# name -> (width, height, camera, accumulator camera, normals, steps, softness, parameter overrides)
CASES = {
    # 1142 selected, 221 antipode votes, 194 bins hit, 4 lines: normals 0, 1, 2 and 4 (0.07 - 1.15 degrees off); line 3's great circle
    # is outside the image
    "five_lines": (160, 120, CAM, ACC, NORMALS, STEPS, 0.02, {}),
    # sides no multiple of the wave or tile size, odd accumulator 81 x 81: 865 selected, 162 antipode votes, 4 lines
    "odd": (157, 83, (0.57, 1.1, 50., 50., 78.3, 41.7), (0.5, 1., 19., 19., 40.5, 40.5), NORMALS, STEPS, 0.02, {}),
    # 772 votes outside the accumulator (590 + 1 cast), 2 lines
    "small_acc": (160, 120, CAM, (0.5, 1., 30., 30., 50., 50.), NORMALS, STEPS, 0.02, {}),
    # 45 of 829 selected pixels with det < 0, 3 lines
    "no_reconstruct": (96, 64, (0.75, 1.2, 36., 36., 48., 32.), (0.5, 1., 22., 22., 48., 48.), NORMALS, STEPS, 0.02, {}),
    # grad_thresh 0: 2052 selected, the zero normals of 1611 flat pixels fail the projection, 40 votes outside, 1 line
    "flat": (64, 48, (0.57, 1.1, 30., 30., 32., 24.), (0.6, 1., 20., 20., 32., 32.), NORMALS, STEPS, 0.02, {"grad_thresh": 0.}),
    # one hard edge through the centre: 450 + 450 votes into 14 bins (150 in the fullest), the worst contention; 2 lines
    "one_line": (160, 120, CAM, ACC, ((0., 1., 0.),), (200.,), 0.005, {}),
}
TRUTH = {"five_lines": (0, 1, 2, 4)}   # the normals whose great circle crosses the image


def image(width, height, cam, normals, steps, softness):
    v, u = np.mgrid[0:height, 0:width].astype(np.float64)
    with np.errstate(all="ignore"):
        ok, x, y, z = hough_ref.reconstruct_v(cam, u, v)
        nrm = np.sqrt(x * x + y * y + z * z)
        img = np.full((height, width), 30.)
        for n, step in zip(normals, steps):
            n = np.asarray(n, dtype=np.float64)
            n = n / np.sqrt(n @ n)
            d = (n[0] * x + n[1] * y + n[2] * z) / nrm
            img = img + step * np.clip(d / softness + 0.5, 0., 1.)
    img = np.where(ok, img, 0.)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


_cache = {}


def case(name):
    """(image u8 [height, width], camera, accumulator camera, parameters) of a case; built once"""
    if name not in _cache:
        w, h, cam, acc, normals, steps, softness, over = CASES[name]
        img = image(w, h, cam, normals, steps, softness)
        img.setflags(write=False)
        _cache[name] = (img, np.array(cam), np.array(acc), hough_ref.params(**over))
    return _cache[name]


_ref = {}


def reference(name):
    """the restatement's result for a case (hough_ref.detect), computed once and shared: do not modify"""
    if name not in _ref:
        img, cam, acc, prm = case(name)
        _ref[name] = hough_ref.detect(img, cam, acc, prm)
    return _ref[name]


def angle_to_truth(normal, which):
    """the smallest angle (rad) between the line through `normal` and those through NORMALS[k], k in which"""
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.sqrt(n @ n)
    best = np.inf
    for k in which:
        t = np.asarray(NORMALS[k], dtype=np.float64)
        t = t / np.sqrt(t @ t)
        best = min(best, float(np.arccos(min(1., abs(float(n @ t))))))
    return best


def check_truth(name, lines):
    """every drawn line that crosses the image is found within one accumulator pixel at the accumulator's centre, 1 / f_acc rad
    (the accumulator's resolution, not a margin on a measurement), and nothing else is found"""
    _, _, acc_cam, _ = case(name)
    bar = 1. / acc_cam[2]
    for k in TRUTH[name]:
        errs = [angle_to_truth(L[3:6], (k,)) for L in lines]
        print("line %d: nearest detection %.3f deg (bar %.3f)" % (k, math.degrees(min(errs)), math.degrees(bar)))
        assert min(errs) <= bar, (k, errs)
    for L in lines:
        assert angle_to_truth(L[3:6], range(len(NORMALS))) <= bar, L
