"""The stereo cases on the strip scene (tests/stereo_scene.py STRIP): long disparity ranges, where the aggregation kernels'
lanes hold more than one disparity each (d = lane + 64 q, q < 4).  Each case names its world, its parameters and the
conditions its restatement output has to meet, so that no case can go vacuous: tests/test_stereo_cpu.py checks the conditions
without a GPU, tests/test_gpu_stereo.py compares the kernels with the same restatement outputs.  Images and restatement
results are computed once per process.

What the restatement gives (share of skipped pixels; winners per quarter of [0, 256); pixels with descriptor step 1 / 2 / >= 3):
    a     0.000   70 / 495 / 586 / 384    1532 /   4 /  0
    b     0.000  258 / 385 / 720 / 173    1277 / 243 / 16
    c     0.000  209 / 1237 / 0 / 0       1532 /   4 /  0
    d66   0.000  914 / 338 / 0 / 0        1532 /   4 /  0
    d130  0.000  185 / 1233 / 75 / 0      1532 /   4 /  0
    e     0.000  258 / 385 / 720 / 173    1277 / 243 / 16
    f     0.000  172 / 317 / 446 / 73      788 / 188 / 32
    g     0.037  481 / 833 / 0 / 0        1004 / 475 /  0    (winners on 0.855 of all pixels, 0.888 of those not skipped)
    h     0.000  352 / 954 / 109 / 0      1277 / 243 / 16
    i0    0.000  182 / 1236 / 75 / 0      1532 /   4 /  0
    i1    0.000  151 / 530 / 14 / 0       1532 /   4 /  0    (841 pixels not skipped and without a winner)
    j     0.000  335 / 881 / 106 / 0      1192 / 218 / 15
    k_row 0.000   31 / 22 / 40 / 3          83 /  13 /  0
    k_col 0.000    0 / 0 / 8 / 8            16 /   0 /  0
    k_one 0.000    winner 191                1 /   0 /  0"""
import numpy as np

from tests import stereo_ref as sr
from tests import stereo_scene

S = stereo_scene.STRIP
BASE = dict(u_max=S["u_max"], v_max=S["v_max"], equal_margins=0, epipole_margin=2500, salient_points_only=0, disp_max=256,
            error_max=150, flaw_cost=25, desc_length=5, scales=[1, 2, 3, 5], desc_resp_thresh=2, use_uv_cache=0, **S["grid"])

# name -> (wall, texture, parameter overrides, conditions beyond the common ones)
#   steps:     at least 100 pixels with descriptor step 2 and 10 with step >= 3 (fillGaps and the step-dependent jump cost run)
#   winners:   winners on at least this share of all pixels
#   no_winner: disparity -1 occurs on pixels that are not skipped
#   line:      a one-line grid, too few pixels for the per-quarter counts: nothing skipped, and winners in these ranges
CASES = {
    "a": ("steep", "fine", dict(use_uv_cache=1), {}),
    "b": ("steep", "coarse", dict(), dict(steps=True)),
    "c": ("steep", "fine", dict(disp_max=120, use_uv_cache=1), {}),
    "d66": ("steep", "fine", dict(disp_max=66), {}),
    "d130": ("steep", "fine", dict(disp_max=130, use_uv_cache=1), {}),
    "e": ("steep", "coarse", dict(disp_max=254, use_uv_cache=1), {}),
    # scale 2 from (292, 4): 48 x 21 depth pixels over rows 4 ... 44
    "f": ("steep", "coarse", dict(disp_max=200, scale=2, u0=292, v0=4, x_max=48, y_max=21), dict(steps=True)),
    # 31 rows do not match across the steep wall's foreshortening (errors saturate at 255 on 98 % of the volume), so the longest
    # descriptor looks at the flat wall at 0.7 m: disparities 56 ... 67, across 63|64, at the file's error_max of 150
    "g": ("flat", "broad", dict(disp_max=128, desc_length=31, scales=[1, 2], use_uv_cache=1), dict(winners=0.3)),
    "h": ("steep", "coarse", dict(disp_max=130, jump_cost=50, image_based_cost=1), dict(steps=True)),
    "i0": ("steep", "fine", dict(disp_max=130, step_cost=0, use_uv_cache=1), {}),
    "i1": ("steep", "fine", dict(disp_max=130, error_max=20, use_uv_cache=1), dict(no_winner=True)),
    "j": ("steep", "coarse", dict(disp_max=130, x_max=95, y_max=15, use_uv_cache=1), {}),
    "k_row": ("steep", "coarse", dict(x_max=96, y_max=1, v0=24, use_uv_cache=1), dict(line=[(0, 64), (64, 128), (128, 192), (192, 256)])),
    "k_col": ("steep", "coarse", dict(x_max=1, y_max=16, u0=360), dict(line=[(128, 192), (192, 256)])),
    "k_one": ("steep", "coarse", dict(x_max=1, y_max=1, u0=360, v0=24, use_uv_cache=1), dict(line=[(128, 256)])),
}
# the other two pairs of case j's batch: the same cameras and grid, other walls and textures
J_BATCH = [("steep", "coarse"), ("steep", "fine"), ("flat", "broad")]

_IMAGES, _REFS = {}, {}


def images(wall, tex):
    if (wall, tex) not in _IMAGES:
        _IMAGES[wall, tex] = stereo_scene.make_strip(tex, wall)
    return _IMAGES[wall, tex]


def prm_of(name):
    return dict(BASE, **CASES[name][2])


def reference(name, world=None):
    """(img1, img2, restatement output) of a case, on its own world or on `world` = (wall, texture); the output is shared:
    do not change it"""
    world = world or CASES[name][:2]
    if (name, world) not in _REFS:
        img1, img2, _, xi = images(*world)
        _REFS[name, world] = sr.stereo(S["cam1"], S["cam2"], xi, sr.params(**prm_of(name)), img1, img2)
    return images(*world)[:2] + (_REFS[name, world],)


def slots(D):
    """the ranges of d one aggregation slot q holds, [64 q, min(64 q + 64, D))"""
    return [(lo, min(lo + 64, D)) for lo in range(0, D, 64)]


def check_conditions(name, ref):
    """the conditions on a case's restatement output under which comparing a kernel with it says something"""
    cond = CASES[name][3]
    D = prm_of(name)["disp_max"]
    skip, step, disp = ref["skip"], ref["step"], ref["disparity"]
    live = skip == 0
    w = disp[disp >= 0]

    def count(lo, hi):
        return int(((w >= lo) & (w < hi)).sum())

    assert skip.mean() <= 0.05, (name, skip.mean())
    if "line" in cond:
        assert live.all(), name
        for lo, hi in cond["line"]:
            assert count(lo, hi) >= 1, (name, lo, hi)
        return
    if D == 256:
        for lo, hi in slots(D):
            assert count(lo, hi) >= 30, (name, lo, hi, count(lo, hi))
        for lo in (63, 127, 191):
            assert count(lo, lo + 2) >= 1, (name, lo)
    else:   # winners in every slot, the partial one above the last 64 boundary too
        for lo, hi in slots(D):
            assert count(lo, hi) >= 1, (name, lo, hi)
    if cond.get("steps"):
        assert (step[live] == 2).sum() >= 100 and (step[live] >= 3).sum() >= 10, (name, np.bincount(step[live]))
    if "winners" in cond:
        assert (disp >= 0).mean() >= cond["winners"], (name, (disp >= 0).mean())
    if cond.get("no_winner"):
        assert (disp[live] == -1).any(), name
