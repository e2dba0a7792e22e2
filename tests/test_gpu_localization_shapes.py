"""Photometric and mutual-information localization on the GPU (vg_photometric.hpp, vg_photometric_mi.hpp) across their launch
boundaries, on the inputs of tests/localization_shapes.py against the restatement (tests/photometric_ref.py, tests/mi_ref.py)
at the bars of tests/test_gpu_photometric.py and tests/test_gpu_mi.py:
A  the packs and both costs where the scan of the block counts runs with chunks of 1, 2 and 3 (256, 257 and 520 workgroups),
   at poses near the truth and at one turned so far that the last workgroup of points leaves the margin and counts in the sums;
B  packs of exactly 1, 63, 64, 65, 255, 256, 257, 512 and 1024 points: a wave, a workgroup, and one point either side;
C  a pyramid of eight levels down to 3 x 2, and the refusal of a ninth;
D  poses that carry points beyond every side of the target image, and into (-1, 0) where floor and a cast differ;
E  a handle whose packs shrink, whose target count changes and whose pose batch grows has the bits of a fresh one.
tests/test_localization_shapes_cpu.py asserts on the restatement alone that the inputs are what these tests need: in
particular that no point lies within 1e-9 of a decision, so every comparison below is over all points."""
import math

import numpy as np
import pytest

from tests import localization_shapes as ls
from tests import mi_ref as mr
from tests import photometric_ref as pr
from tests import photometric_scene as ps
from tests.test_photometric_cpu import near_boundary

pytestmark = pytest.mark.gpu
PARITY = 1e-10   # the project's parity bar, relative to max |.| per array


@pytest.fixture(scope="module")
def torch():
    import torch

    from visgeom_amd import _build

    _build.build()
    return torch


def params(prm):
    from visgeom_amd import stereo

    return stereo.make_params(equal_margins=0, **prm)


def make_handle(torch, cam, prm, w, h, scales, base=None, depth=None, targets=None):
    from visgeom_amd import photometric

    hd = photometric.Photometric(cam, params(prm), ps.XI_BASE_CAM, w, h, scales)
    if base is not None:
        hd.set_base(torch.from_numpy(base).cuda(), torch.from_numpy(depth).cuda())
    if targets is not None:
        hd.set_targets(torch.from_numpy(targets).cuda())
    return hd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def host(t):
    return t.cpu().numpy()


# ---- the comparisons -----------------------------------------------------------------------------------------------

def compare_pack(hd, scale, want):
    idx, val, cloud = [host(t) for t in hd.pack(scale)]
    assert idx.shape == want["idx"].shape, (scale, idx.shape, want["idx"].shape)
    assert (idx == want["idx"]).all()
    assert (val.view(np.uint64) == want["val"].view(np.uint64)).all()
    assert np.abs(cloud - want["cloud"]).max() <= PARITY * np.abs(want["cloud"]).max()


def compare_evaluate(hd, loc, scale, poses, targets):
    """the bars of test_gpu_photometric.test_evaluate with no point left out, and the sums without the rows to the bit"""
    out = hd.evaluate(scale, poses, targets)
    lean = hd.evaluate(scale, poses, targets, rows=False)
    assert lean["residuals"] is None and lean["jacobians"] is None
    for k in ("cost", "jtj", "jtr"):
        assert (bits(out[k]) == bits(lean[k])).all(), k
    res, jac = host(out["residuals"]), host(out["jacobians"])
    for i, (xi, k) in enumerate(zip(poses, targets)):
        e = loc.evaluate(scale, xi, int(k))
        assert not near_boundary(loc, scale, e).any()   # so rows and sums are over the same points
        zero = e["state"] != 0
        assert (res[i][zero] == 0.).all() and (jac[i][zero] == 0.).all()   # zero rows exactly where the restatement has them
        assert ((e["res"] != 0.) == (res[i] != 0.)).all()
        cost, jtj, jtr = pr.sums(e["res"], e["jac"])
        print("scale", scale, "pose", i, "points", len(e["res"]), "in the margin", int(zero.sum()), "cost", cost, out["cost"][i])
        assert np.abs(res[i] - e["res"]).max() <= PARITY * np.abs(e["res"]).max()
        assert np.abs(jac[i] - e["jac"]).max() <= PARITY * np.abs(e["jac"]).max()
        assert abs(out["cost"][i] - cost) <= PARITY * cost
        assert np.abs(out["jtj"][i] - jtj).max() <= PARITY * np.abs(jtj).max()
        assert np.abs(out["jtr"][i] - jtr).max() <= PARITY * np.abs(jtr).max()


def compare_mi(hd, loc, scale, poses, targets, cost_bar=None, gradient_bar=None):
    """the bars of test_gpu_mi.test_evaluate_mi with no point left out.  cost_bar, gradient_bar: absolute bars in place of the
    relative ones, for the pack of one point whose cost and gradient are 0"""
    out = hd.evaluate_mi(scale, poses, targets)
    lean = hd.evaluate_mi(scale, poses, targets, values=False, gradient=False)
    assert (bits(out["cost"]) == bits(lean["cost"])).all() and (bits(out["hist"]) == bits(lean["hist"])).all()
    val = host(out["values"])
    for i, (xi, k) in enumerate(zip(poses, targets)):
        e = mr.evaluate_mi(loc, scale, xi, int(k))
        assert not (e["slack"] < 1e-9).any()   # so histogram, cost and gradient are over the same decisions
        print("scale", scale, "pose", i, "points", len(e["values"]), "failed", int((~e["ok"]).sum()), "cost", e["cost"], out["cost"][i],
              "gradient", np.abs(e["gradient"]).max(), np.abs(out["gradient"][i] - e["gradient"]).max())
        assert (val[i][~e["ok"]] == 0.).all()
        assert np.abs(val[i] - e["values"]).max() <= PARITY * mr.VAL_MAX
        h, hr = out["hist"][i].ravel(), e["hist"]
        assert ((h == 0.) == (hr == 0.)).all()   # exactly zero bins are zero in both
        assert np.abs(h - hr).max() <= PARITY * hr.max()
        assert abs(out["cost"][i] - e["cost"]) <= (PARITY * abs(e["cost"]) if cost_bar is None else cost_bar)
        assert np.abs(out["gradient"][i] - e["gradient"]).max() <= (PARITY * np.abs(e["gradient"]).max() if gradient_bar is None else gradient_bar)


def same_bits(a, b, keys, tensors):
    for k in keys:
        assert (bits(a[k]) == bits(b[k])).all(), k
    for k in tensors:
        assert (bits(host(a[k])) == bits(host(b[k]))).all(), k


PHOTO = (("cost", "jtj", "jtr"), ("residuals", "jacobians"))
MI = (("cost", "hist", "gradient"), ("values",))


# ---- A: the scan with chunks ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scaled_handle(torch):
    made = {}

    def get(w, h):
        if (w, h) not in made:
            s = ls.scaled(w, h)
            made[(w, h)] = make_handle(torch, s["cam"], s["prm"], w, h, ls.SCALES_A, s["base"], s["depth"], s["target"])
        return made[(w, h)]

    yield get
    for hd in made.values():
        hd.close()


@pytest.mark.parametrize("w,h", ls.SHAPES)
def test_scaled_packs(torch, scaled_handle, w, h):
    loc = ls.scaled(w, h)["loc"]
    hd = scaled_handle(w, h)
    for scale in range(ls.SCALES_A):
        compare_pack(hd, scale, loc.packs[scale])
        for g, want in zip([host(t) for t in hd.level(scale)], loc.base[scale]):   # the odd width halves as the restatement's
            assert g.shape == want.shape and (g.view(np.uint32) == want.view(np.uint32)).all(), scale


@pytest.mark.parametrize("w,h", ls.SHAPES)
def test_scaled_evaluate(torch, scaled_handle, w, h):
    loc = ls.scaled(w, h)["loc"]
    poses = ls.poses_a()
    for scale in range(ls.SCALES_A):
        compare_evaluate(scaled_handle(w, h), loc, scale, poses, np.zeros(len(poses), np.int32))


@pytest.mark.parametrize("w,h", ls.SHAPES)
def test_scaled_evaluate_mi(torch, scaled_handle, w, h):
    loc = ls.scaled(w, h)["loc"]
    poses = ls.poses_a()
    for scale in range(ls.SCALES_A):
        compare_mi(scaled_handle(w, h), loc, scale, poses, np.zeros(len(poses), np.int32))


# ---- B: exact pack sizes -------------------------------------------------------------------------------------------

def exact_handle(torch, depth):
    s = ps.scene()
    return make_handle(torch, ps.CAM, ls.PRM_B, ps.W, ps.H, 1, s["base"], depth, s["targets"][0])


@pytest.mark.parametrize("m", ls.EXACT_SIZES)
def test_exact_pack_size(torch, m):
    """a pack of exactly m points, every one a residual at POSE_B; the truth as a second pose.  With one point the mutual
    information is 0 (the joint histogram is the product of its marginals) and the GPU may return a rounding residue: the cost
    is held absolutely to 1e-10 log(8), the bound of the cost with 8 bins, and the gradient to 1e-10 of the restatement's
    max |gradient| at m = 64 for the same pose"""
    x = ls.exact(m)
    loc = x["loc"]
    hd = exact_handle(torch, x["depth"])
    try:
        assert int(hd.pack(0)[0].numel()) == m
        compare_pack(hd, 0, loc.packs[0])
        poses, targets = np.array([ls.POSE_B, ps.TRUE_POSES[0]], float), np.zeros(2, np.int32)
        compare_evaluate(hd, loc, 0, poses, targets)
        if m == 1:
            ref64 = ls.exact(64)["loc"]
            for xi in poses:
                compare_mi(hd, loc, 0, xi[None], targets[:1], cost_bar=PARITY * math.log(mr.NUM_BINS),
                           gradient_bar=PARITY * np.abs(mr.evaluate_mi(ref64, 0, xi, 0)["gradient"]).max())
        else:
            compare_mi(hd, loc, 0, poses, targets)
    finally:
        hd.close()


# ---- C: eight levels -----------------------------------------------------------------------------------------------

NOISE_CAM = ls.camera(ls.NOISE_W, ls.NOISE_H)
NOISE_PRM = ls.grid(ls.NOISE_W, ls.NOISE_H)


def test_eight_levels_bit_equal(torch):
    """384 x 256 down to 3 x 2: every level of the image and both gradients, for the key frame and for a target"""
    base, target = ls.noise(0), ls.noise(1)
    depth = np.full((NOISE_PRM["y_max"], NOISE_PRM["x_max"]), 2.)
    hd = make_handle(torch, NOISE_CAM, NOISE_PRM, ls.NOISE_W, ls.NOISE_H, ls.NOISE_SCALES, base, depth, target)
    try:
        assert hd.sizes[7] == (3, 2)
        for which, img in ((None, base), (0, target)):
            want = pr.pyramid(img, ls.NOISE_SCALES)
            for scale in range(ls.NOISE_SCALES):
                got = [host(t) for t in hd.level(scale, which)]
                for g, w in zip(got, want[scale]):
                    assert g.dtype == np.float32 and g.shape == w.shape == (ls.NOISE_H >> scale, ls.NOISE_W >> scale)
                    assert (g.view(np.uint32) == w.view(np.uint32)).all(), (which, scale)
    finally:
        hd.close()


def test_level_count_refusals(torch):
    """vg_photometric_create's two rules: num_scales in [1, 8] (so nine levels are refused at 384 x 256, although 384 >> 8 and
    256 >> 8 are both 1), and a coarsest level of at least 1 x 1: eight levels need 128 rows"""
    from visgeom_amd import capi, photometric

    def refused(w, h, n):
        with pytest.raises(capi.VisgeomError) as e:
            photometric.Photometric(NOISE_CAM, params(NOISE_PRM), ps.XI_BASE_CAM, w, h, n)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT

    refused(ls.NOISE_W, ls.NOISE_H, 9)
    refused(ls.NOISE_W, ls.NOISE_H, 0)
    refused(ls.NOISE_W, 127, 8)   # 127 >> 7 == 0
    refused(127, ls.NOISE_H, 8)
    hd = photometric.Photometric(NOISE_CAM, params(NOISE_PRM), ps.XI_BASE_CAM, ls.NOISE_W, 128, 8)
    assert hd.sizes[7] == (3, 1)
    hd.close()


# ---- D: samples outside the target ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene_handle(torch):
    s = ps.scene()
    hd = make_handle(torch, ps.CAM, ps.PRM, ps.W, ps.H, ps.NUM_SCALES, s["base"], s["depth"], s["targets"])
    yield hd
    hd.close()


def outside_preconditions():
    beyond = np.zeros(4, int)
    for xi in ls.OUTSIDE_POSES:
        u, v, ok = ls.outside_projection(0, xi)
        assert ok.mean() >= 0.99
        assert (ok & (((u > -1.) & (u < 0.)) | ((v > -1.) & (v < 0.)))).sum() >= 10
        beyond += [(ok & (u < 0.)).sum(), (ok & (u > ps.W - 1.)).sum(), (ok & (v < 0.)).sum(), (ok & (v > ps.H - 1.)).sum()]
    assert (beyond >= 1000).all(), beyond


def test_outside_mi(torch, scene_handle):
    """mutual information samples through the clamping grid wherever a point lands"""
    outside_preconditions()
    for scale in (0, 2):
        compare_mi(scene_handle, ps.localizer(), scale, ls.OUTSIDE_POSES, np.zeros(4, np.int32))


def test_outside_photometric(torch, scene_handle):
    """the photometric cost at the same poses: zero residual and row at exactly the points the restatement puts in the margin"""
    outside_preconditions()
    for scale in (0, 2):
        compare_evaluate(scene_handle, ps.localizer(), scale, ls.OUTSIDE_POSES, np.zeros(4, np.int32))


# ---- E: a reused handle --------------------------------------------------------------------------------------------

def test_set_base_after_a_shrink(torch):
    """set_base with the full depth (35 489 points, 139 workgroups, every scratch buffer grown by both costs), then with the
    depth of 65 points: the pack, evaluate and evaluate_mi have the bits of a fresh handle given only the second call"""
    small = ls.exact(65)["depth"]
    poses, targets = np.array([ls.POSE_B, ps.TRUE_POSES[0]], float), np.zeros(2, np.int32)
    used, fresh = exact_handle(torch, ls.full_depth()), exact_handle(torch, small)
    try:
        assert int(used.pack(0)[0].numel()) == len(ls.full_localizer().packs[0]["idx"])
        used.evaluate(0, poses, targets)
        used.evaluate_mi(0, poses, targets)
        used.set_base(torch.from_numpy(ps.scene()["base"]).cuda(), torch.from_numpy(small).cuda())
        for a, b in zip(used.pack(0), fresh.pack(0)):
            assert a.shape == b.shape and a.shape[0] == 65 and torch.equal(a, b)
        same_bits(used.evaluate(0, poses, targets), fresh.evaluate(0, poses, targets), *PHOTO)
        same_bits(used.evaluate_mi(0, poses, targets), fresh.evaluate_mi(0, poses, targets), *MI)
    finally:
        used.close()
        fresh.close()


def test_set_targets_after_a_change_of_count(torch):
    """three targets, then one: the pyramid and both costs have the bits of a fresh handle, and the old indices are refused"""
    from visgeom_amd import capi

    s = ps.scene()
    poses, targets = np.array([ps.TRUE_POSES[1], ps.start_pose(1)], float), np.zeros(2, np.int32)
    used = make_handle(torch, ps.CAM, ps.PRM, ps.W, ps.H, ps.NUM_SCALES, s["base"], s["depth"], s["targets"])
    fresh = make_handle(torch, ps.CAM, ps.PRM, ps.W, ps.H, ps.NUM_SCALES, s["base"], s["depth"], s["targets"][1])
    try:
        used.evaluate(0, poses, np.array([2, 1], np.int32))
        used.evaluate_mi(0, poses, np.array([2, 1], np.int32))
        used.set_targets(torch.from_numpy(s["targets"][1]).cuda())
        with pytest.raises(capi.VisgeomError) as e:
            used.evaluate(0, poses, np.array([0, 1], np.int32), rows=False)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT
        for scale in range(ps.NUM_SCALES):
            for a, b in zip(used.level(scale, 0), fresh.level(scale, 0)):
                assert torch.equal(a, b)
            same_bits(used.evaluate(scale, poses, targets), fresh.evaluate(scale, poses, targets), *PHOTO)
            same_bits(used.evaluate_mi(scale, poses, targets), fresh.evaluate_mi(scale, poses, targets), *MI)
    finally:
        used.close()
        fresh.close()


def test_a_growing_pose_batch(torch):
    """1 pose, then 7, then 2 on a fresh handle, at scale 1 and then at scale 0 (27 and then 97 workgroups per pose, so the
    [n][blocks] scratch grows twice more): every pose of a batch has the bits of its single call"""
    s = ps.scene()
    p4, t4 = ps.eval_poses()
    poses = np.concatenate([p4, [ps.start_pose(2), ps.TRUE_POSES[2], ps.start_pose(0, -0.7)]])
    targets = np.concatenate([t4, [2, 2, 0]]).astype(np.int32)
    hd = make_handle(torch, ps.CAM, ps.PRM, ps.W, ps.H, ps.NUM_SCALES, s["base"], s["depth"], s["targets"])
    try:
        for scale in (1, 0):
            first = (hd.evaluate(scale, poses[:1], targets[:1]), hd.evaluate_mi(scale, poses[:1], targets[:1]))
            seven = (hd.evaluate(scale, poses, targets), hd.evaluate_mi(scale, poses, targets))
            two = (hd.evaluate(scale, poses[5:], targets[5:]), hd.evaluate_mi(scale, poses[5:], targets[5:]))
            for i in range(7):
                single = first if i == 0 else (hd.evaluate(scale, poses[i:i + 1], targets[i:i + 1]), hd.evaluate_mi(scale, poses[i:i + 1], targets[i:i + 1]))
                for got, one, (keys, tensors) in zip(seven, single, (PHOTO, MI)):
                    same_bits({k: got[k][i] for k in keys + tensors}, {k: one[k][0] for k in keys + tensors}, keys, tensors)
                if i >= 5:
                    for got, one, (keys, tensors) in zip(two, single, (PHOTO, MI)):
                        same_bits({k: got[k][i - 5] for k in keys + tensors}, {k: one[k][0] for k in keys + tensors}, keys, tensors)
    finally:
        hd.close()
