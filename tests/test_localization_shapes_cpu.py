"""The conditions the inputs of tests/localization_shapes.py have to meet for tests/test_gpu_localization_shapes.py to test
what it says, asserted on the restatement alone (tests/photometric_ref.py, tests/mi_ref.py).  No GPU."""
import numpy as np
import pytest

from tests import localization_shapes as ls
from tests import mi_ref as mr
from tests import photometric_ref as pr
from tests import photometric_scene as ps
from tests.test_photometric_cpu import near_boundary


def no_point_left_out(loc, scale, xi, target=0):
    """neither comparison of the GPU tests would leave a point out: none within 1e-9 px of a pixel boundary or a margin edge,
    none within 1e-9 of a threshold of the projection"""
    e = loc.evaluate(scale, xi, target, want_jac=False)
    slack = mr.evaluate_mi(loc, scale, xi, target, want_grad=False)["slack"]
    return not near_boundary(loc, scale, e).any() and not (slack < 1e-9).any()


@pytest.mark.parametrize("w,h", ls.SHAPES)
def test_scaled_scenes(w, h):
    """A: the workgroups of level 0 are 256, 257 and 520, so the scan's chunks are 1, 2 and 3, and with a chunk above 1 the
    last thread in use holds a single block; every pack is larger than one workgroup and ends in a partly filled one, every
    rejection of the selection is reached, a pose leaves points inside and in the margin, and no point is left out"""
    loc = ls.scaled(w, h)["loc"]
    nb = ls.blocks_of(w * h)
    chunk = (nb + ls.LANES - 1) // ls.LANES
    assert (nb, chunk) == {(256, 256): (256, 1), (257, 256): (257, 2), (416, 320): (520, 3)}[(w, h)]
    assert [lv[0].shape for lv in loc.base] == [(h, w), (h // 2, w // 2)]
    for scale in range(ls.SCALES_A):
        pack = loc.packs[scale]
        assert len(pack["idx"]) > ls.LANES and pack["dropped_depth"] >= 1
        assert len(pack["idx"]) % ls.LANES != 0   # a partly filled last workgroup of points
        for xi in ls.poses_a():
            state = loc.evaluate(scale, xi, 0, want_jac=False)["state"]
            assert (state == 0).sum() >= 1000 and (state == 2).sum() >= 1000
            assert no_point_left_out(loc, scale, xi)
        # at the turned pose the last workgroup of points carries a visible part of the cost
        e = loc.evaluate(scale, ls.poses_a()[-1], 0, want_jac=False)
        last = (len(e["res"]) - 1) // ls.LANES * ls.LANES
        assert (e["state"][last:] == 0).sum() >= 10 and e["res"][last:] @ e["res"][last:] >= 1e-4 * (e["res"] @ e["res"])
    if (w, h) == (416, 320):
        counts = ls.block_counts(loc.packs[0]["idx"], w * h)
        print("416 x 320: empty workgroups", (counts == 0).sum(), "of", len(counts), "largest", counts.max(), "pack", counts.sum())
        assert len(counts) == 520 and (counts == 0).sum() >= 20 and counts.max() > 128
    if chunk > 1:
        assert nb % chunk == 1   # thread nb / chunk holds one block of its chunk, the threads behind it none


def test_exact_sizes():
    """B: exactly m points, each of them a residual (state 0) at POSE_B, none left out; at the truth as well"""
    assert len(ls.full_localizer().packs[0]["idx"]) > len(ls.inside_pixels()) >= 2 * max(ls.EXACT_SIZES)
    print("full pack", len(ls.full_localizer().packs[0]["idx"]), "inside the margin at POSE_B", len(ls.inside_pixels()))
    for m in ls.EXACT_SIZES:
        loc = ls.exact(m)["loc"]
        assert len(loc.packs[0]["idx"]) == m
        assert (loc.evaluate(0, ls.POSE_B, 0, want_jac=False)["state"] == 0).all()
        for xi in (ls.POSE_B, ps.TRUE_POSES[0]):
            assert no_point_left_out(loc, 0, xi)


def test_one_point_has_no_mutual_information():
    """B, m = 1: the joint histogram of one point is the product of its marginals, cost and gradient are exactly 0; the GPU test
    takes its absolute bars from log(8) and from the gradient at m = 64"""
    e = mr.evaluate_mi(ls.exact(1)["loc"], 0, ls.POSE_B, 0)
    assert e["cost"] == 0. and (e["gradient"] == 0.).all()
    assert abs(e["hist"].sum() - 1.) <= 1e-15
    assert np.abs(mr.evaluate_mi(ls.exact(64)["loc"], 0, ls.POSE_B, 0)["gradient"]).max() > 1.


def test_noise_pyramid_has_eight_levels():
    """C: 384 x 256 halves seven times to 3 x 2; the values stay integers / 4^level below 2^24, exact in float32"""
    lv = pr.pyramid(ls.noise(), ls.NOISE_SCALES, gradients=False)
    assert [x[0].shape for x in lv] == [(ls.NOISE_H >> i, ls.NOISE_W >> i) for i in range(8)] and lv[7][0].shape == (2, 3)
    for i, (img, _, _) in enumerate(lv):
        q = img.astype(np.float64) * 4. ** i
        assert (q == np.round(q)).all() and q.max() < 2. ** 24
    # by hand: row 0 of every level takes source row 0 alone, so level 7's is the image's row 0 summed over 128 columns / 4^7
    top = ls.noise()[0].astype(np.int64).reshape(3, 128).sum(1) / 4. ** 7
    assert lv[7][0][0].tolist() == top.tolist()


def test_outside_poses():
    """D: every pose projects at least 99 % of the points; over the four poses each side of the target image has at least 1000
    points of scale 0 beyond it; every pose has at least 10 points of scale 0 in (-1, 0) on some axis, where floor and a cast
    differ (and at least one at scale 2); no point is left out"""
    W, H = ps.W, ps.H
    beyond = np.zeros(4, int)
    for xi in ls.OUTSIDE_POSES:
        for scale in (0, 2):
            u, v, ok = ls.outside_projection(scale, xi)
            assert ok.mean() >= 0.99
            sc = float(1 << scale)
            between = ok & (((u / sc > -1.) & (u / sc < 0.)) | ((v / sc > -1.) & (v / sc < 0.)))
            assert between.sum() >= (10 if scale == 0 else 1)
            if scale == 0:
                beyond += [(ok & (u < 0.)).sum(), (ok & (u > W - 1.)).sum(), (ok & (v < 0.)).sum(), (ok & (v > H - 1.)).sum()]
            assert no_point_left_out(ps.localizer(), scale, xi)
            state = ps.localizer().evaluate(scale, xi, 0, want_jac=False)["state"]
            assert (state == 0).sum() >= 100 and (state == 2).sum() >= 100
    print("beyond left, right, top, bottom:", beyond.tolist())
    assert (beyond >= 1000).all()
