"""Photometric localization on the GPU (vg_photometric_*, visgeom_amd.photometric) against the restatement
(tests/photometric_ref.py) on the scene of tests/photometric_scene.py: 256 x 192, depth map scale 2, three pyramid scales,
three targets.  Pyramids and gradients bit for bit, the data packs in order, the cost with its rows and sums to 1e-10, its
determinism, computePose against the restatement's own solve, batching, the motion prior, and the refusals."""
import numpy as np
import pytest

from tests import photometric_ref as pr
from tests import photometric_scene as ps
from tests.test_photometric_cpu import near_boundary

pytestmark = pytest.mark.gpu
PARITY = 1e-10   # the project's parity bar, relative to max |.| per array
# computePose is not compared iterate by iterate: the cost is not smooth (points switch in and out of the margin and across the
# loss cut), so two correct solvers may walk differently.  The restatement alone, from the start pose and from 0.9 x and
# 1.1 x its offset, ends at the finest scale with costs 29.362439904, 29.362439903, 29.362440220 (spread 1.1e-8 relative) and
# pose errors against the truth of 0.3253146 mm / 0.2417370 mrad (spread 8.5e-9 m / 4.4e-9 rad).  Margins chosen from that: the
# cost within 1e-5 (ten function tolerances, a thousand spreads), the pose error within 1e-3 relative plus a floor of 1e-6 m
# and 1e-6 rad (a hundred spreads, 0.3 % of the error itself).
COST_MARGIN, POSE_MARGIN, POSE_FLOOR = 1e-5, 1e-3, 1e-6


@pytest.fixture(scope="module")
def torch():
    import torch

    from visgeom_amd import _build

    _build.build()
    return torch


def params():
    from visgeom_amd import stereo

    return stereo.make_params(equal_margins=0, **ps.PRM)


@pytest.fixture(scope="module")
def handle(torch):
    from visgeom_amd import photometric

    s = ps.scene()
    h = photometric.Photometric(ps.CAM, params(), ps.XI_BASE_CAM, ps.W, ps.H, ps.NUM_SCALES)
    h.set_base(torch.from_numpy(s["base"]).cuda(), torch.from_numpy(s["depth"]).cuda())
    h.set_targets(torch.from_numpy(s["targets"]).cuda())
    yield h
    h.close()


def test_pyramids_and_gradients_bit_equal(torch, handle):
    loc = ps.localizer()
    s = ps.scene()
    for scale in range(ps.NUM_SCALES):
        for which in (None, 0, 1, 2):
            want = loc.base[scale] if which is None else (loc.targets[which][scale][0],) + pr.sobel(loc.targets[which][scale][0])
            got = [t.cpu().numpy() for t in handle.level(scale, which)]
            for g, w in zip(got, want):
                assert g.dtype == np.float32 and g.shape == w.shape == (ps.H >> scale, ps.W >> scale)
                assert (g.view(np.uint32) == w.view(np.uint32)).all(), (scale, which)
    assert s["base"].shape == (ps.H, ps.W)


def test_pyramid_odd_sizes_bit_equal(torch):
    """37 x 29 -> 18 x 14 -> 9 x 7 -> 4 x 3: odd at every level, levels smaller than a wave"""
    from visgeom_amd import photometric

    rnd = np.random.default_rng(5)
    img = rnd.integers(0, 256, (29, 37), dtype=np.uint8)
    h = photometric.Photometric(ps.CAM, params(), ps.XI_BASE_CAM, 37, 29, 4)
    h.set_targets(torch.from_numpy(img).cuda())
    want = pr.pyramid(img, 4)
    for scale in range(4):
        got = [t.cpu().numpy() for t in h.level(scale, 0)]
        for g, w in zip(got, want[scale]):
            assert g.shape == w.shape and (g.view(np.uint32) == w.view(np.uint32)).all(), scale
    h.close()


def test_data_packs(torch, handle):
    loc = ps.localizer()
    for scale in range(ps.NUM_SCALES):
        idx, val, cloud = [t.cpu().numpy() for t in handle.pack(scale)]
        want = loc.packs[scale]
        assert idx.tolist() == want["idx"].tolist()
        assert (val.view(np.uint64) == want["val"].view(np.uint64)).all()
        assert np.abs(cloud - want["cloud"]).max() <= PARITY * np.abs(want["cloud"]).max()


def test_evaluate(torch, handle):
    loc = ps.localizer()
    poses, targets = ps.eval_poses()
    for scale in range(ps.NUM_SCALES):
        out = handle.evaluate(scale, poses, targets)
        res, jac = out["residuals"].cpu().numpy(), out["jacobians"].cpu().numpy()
        again = handle.evaluate(scale, poses, targets)
        for k in ("cost", "jtj", "jtr"):
            assert (out[k].view(np.uint64) == again[k].view(np.uint64)).all(), k
        assert (again["residuals"].cpu().numpy().view(np.uint64) == res.view(np.uint64)).all()
        assert (again["jacobians"].cpu().numpy().view(np.uint64) == jac.view(np.uint64)).all()
        for i, (xi, k) in enumerate(zip(poses, targets)):
            e = loc.evaluate(scale, xi, int(k))
            skip = near_boundary(loc, scale, e)
            assert skip.mean() <= 0.005
            keep = ~skip
            zero = e["state"] != 0
            assert (res[i][keep & zero] == 0.).all() and (jac[i][keep & zero] == 0.).all()   # zero rows exactly where the restatement has them
            assert ((e["res"] != 0.) == (res[i] != 0.))[keep].all()
            assert np.abs(res[i] - e["res"])[keep].max() <= PARITY * np.abs(e["res"]).max()
            assert np.abs(jac[i] - e["jac"])[keep].max() <= PARITY * np.abs(e["jac"]).max()
            assert not skip.any()   # so the sums below are over the same points
            cost, jtj, jtr = pr.sums(e["res"], e["jac"])
            assert abs(out["cost"][i] - cost) <= PARITY * cost
            assert np.abs(out["jtj"][i] - jtj).max() <= PARITY * np.abs(jtj).max()
            assert np.abs(out["jtr"][i] - jtr).max() <= PARITY * np.abs(jtr).max()


def test_evaluate_sums_only_and_one_pose(torch, handle):
    """the sums without the rows, and a batch of one, give the bits of the batch of four"""
    poses, targets = ps.eval_poses()
    full = handle.evaluate(1, poses, targets)
    lean = handle.evaluate(1, poses, targets, rows=False)
    one = handle.evaluate(1, poses[2], targets[2:3], rows=False)
    for k in ("cost", "jtj", "jtr"):
        assert (full[k].view(np.uint64) == lean[k].view(np.uint64)).all()
        assert (full[k][2].view(np.uint64) == one[k][0].view(np.uint64)).all()
    assert lean["residuals"] is None


def test_compute_pose_against_the_restatement(torch, handle):
    """see the comment at COST_MARGIN: the restatement's cost at the GPU's pose within 1e-5 of the restatement's own final cost
    (finest scale), the GPU's pose error within 1e-3 + 1e-6 of the restatement's"""
    loc = ps.localizer()
    ref_x, ref_rep = ps.reference_solve(0)
    x, rep = handle.compute_pose(ps.start_pose(0), [0])
    print("GPU pose", x.tolist(), "report", rep.tolist(), "reference", ref_x.tolist(), [r["final_cost"] for r in ref_rep])
    cost_at_gpu = loc.cost(0, x, 0)
    print("reference cost at the GPU pose", cost_at_gpu, "reference final", ref_rep[0]["final_cost"])
    assert cost_at_gpu <= ref_rep[0]["final_cost"] * (1. + COST_MARGIN)
    (et, er), (rt, rr) = ps.pose_error(x), ps.pose_error(ref_x)
    print("pose error", et, er, "reference", rt, rr)
    assert et <= rt * (1. + POSE_MARGIN) + POSE_FLOOR and er <= rr * (1. + POSE_MARGIN) + POSE_FLOOR
    assert rep.shape == (ps.NUM_SCALES, 4)
    for s in range(ps.NUM_SCALES):
        assert 1 <= rep[s, 0] <= pr.MAX_ITERATIONS and rep[s, 2] <= rep[s, 1] and rep[s, 3] in (0, 1, 2, 3, 4)
    assert abs(rep[ps.NUM_SCALES - 1, 1] - ref_rep[ps.NUM_SCALES - 1]["initial_cost"]) <= PARITY * rep[ps.NUM_SCALES - 1, 1]


def test_compute_pose_batch_equals_single_calls(torch, handle):
    starts = np.array([ps.start_pose(k) for k in range(3)])
    xb, rb = handle.compute_pose(starts, [0, 1, 2])
    for k in range(3):
        x1, r1 = handle.compute_pose(starts[k], [k])
        assert (x1.view(np.uint64) == xb[k].view(np.uint64)).all() and (r1.view(np.uint64) == rb[k].view(np.uint64)).all()
        (et, er), (rt, rr) = ps.pose_error(xb[k], k), ps.pose_error(ps.reference_solve(k)[0], k)   # every target is found
        assert et <= rt * (1. + POSE_MARGIN) + POSE_FLOOR and er <= rr * (1. + POSE_MARGIN) + POSE_FLOOR, (k, et, er, rt, rr)


def test_motion_prior_pulls_towards_the_prior(torch, handle):
    x0 = np.array(ps.start_pose(0))
    free, _ = handle.compute_pose(x0, [0])
    held, _ = handle.compute_pose(x0, [0], xi_prior=x0)
    assert np.linalg.norm(held - x0) < np.linalg.norm(free - x0)


def test_refusals(torch, handle):
    from visgeom_amd import capi, photometric

    poses, targets = ps.eval_poses()

    def refused(fn):
        with pytest.raises(capi.VisgeomError) as e:
            fn()
        assert e.value.code == capi.ERR_INVALID_ARGUMENT

    fresh = photometric.Photometric(ps.CAM, params(), ps.XI_BASE_CAM, ps.W, ps.H, ps.NUM_SCALES)
    refused(lambda: fresh.evaluate(0, poses, targets, rows=False))      # before set_base
    s = ps.scene()
    fresh.set_base(torch.from_numpy(s["base"]).cuda(), torch.from_numpy(s["depth"]).cuda())
    refused(lambda: fresh.evaluate(0, poses, targets, rows=False))      # before set_targets
    refused(lambda: fresh.compute_pose(poses[0], [0]))
    fresh.close()
    refused(lambda: handle.evaluate(ps.NUM_SCALES, poses, targets, rows=False))
    refused(lambda: handle.evaluate(-1, poses, targets, rows=False))
    refused(lambda: handle.evaluate(0, poses, [0, 0, 1, 3], rows=False))   # three targets: index 3 is out of range
    refused(lambda: handle.compute_pose(poses[0], [-1]))
    refused(lambda: photometric.Photometric(ps.CAM, params(), ps.XI_BASE_CAM, ps.W, ps.H, 9))   # 192 >> 8 == 0
    refused(lambda: photometric.Photometric(ps.CAM, params(), ps.XI_BASE_CAM, 16, 12, 5))       # 12 >> 4 == 0
    # the grid the wrappers compute for their shape checks is the library's (vg_depth_fusion_size), in both margin modes
    from visgeom_amd import _handle, depth_fusion, stereo

    for kw in (dict(equal_margins=0, **ps.PRM), dict(equal_margins=1, scale=3, u0=10, v0=7, u_max=ps.W, v_max=ps.H)):
        p = stereo.make_params(**kw)
        f = depth_fusion.DepthFusion(ps.CAM, p)
        assert _handle._grid_size(p) == (f.x_max, f.y_max)
        f.close()
