"""Mutual-information localization on the GPU (vg_mi_evaluate / _compute_pose_mi, visgeom_amd.photometric) against
the restatement (tests/mi_ref.py) on the scene of tests/mi_scene.py: 256 x 192, three scales, the three plain targets and
target 0 with its grey levels remapped.  The cost with values, histogram and gradient to 1e-10, its determinism, computePoseMI
against the restatement's own solve, the remapped target against the photometric cost, batching, the odometry term, refusals."""
import numpy as np
import pytest

from tests import mi_ref as mr
from tests import mi_scene as ms
from tests import photometric_scene as ps

pytestmark = pytest.mark.gpu
PARITY = 1e-10   # the project's parity bar
# The restatement's gradient summed in reversed point order differs from the forward sum by at most 1.2e-14 of max|g| over the
# fifteen (scale, pose) cases of test_evaluate_mi (asserted there below 1e-12): summation order is worth 1e-4 of the bar.
#
# compute_pose_mi is not compared iterate by iterate.  At the tolerances ms.TIGHT (function 1e-9, gradient 1e-6) the restatement
# from the start pose and from 0.9 x and 1.1 x its offset ends, on the plain target, at the finest-scale cost
# -0.92725980685596 (spread 2.4e-16 relative) and pose errors 0.21846656 mm / 0.20519729 mrad (spread 8.5e-17 m / 6.9e-18 rad);
# on the remapped target at -0.38176987592409 (2.9e-16) and 0.62029045 mm / 0.37687127 mrad (4.9e-17 m / 5.1e-17 rad): the
# three runs end at one point to rounding.  Two correct solvers need not: both stop once max|g| <= 1e-6, which with the cost's
# curvature (the gradient changes by about 20 over the start offset of 0.03: about 1e3) leaves 1e-9 in the pose and 1e-15 in
# the cost.  Margins: the cost within 1e-8 |cost| and the pose error within 1e-3 relative plus 1e-6 m / 1e-6 rad -- each more
# than a million spreads, and a thousand times what the stopping rule leaves.
COST_MARGIN, POSE_MARGIN, POSE_FLOOR = 1e-8, 1e-3, 1e-6
# The reason for the feature, on the restatement at ms.TIGHT: mutual information finds the remapped target to 0.620 mm /
# 0.377 mrad against 0.218 mm / 0.205 mrad on the plain one (2.84 x and 1.84 x), the photometric cost to 34.3 mm / 9.19 mrad
# against 0.325 mm / 0.242 mrad.  The factor allowed below is 4: the larger ratio with a margin of 1.4.
REMAP_FACTOR = 4.


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
    h.set_targets(torch.from_numpy(ms.target_images()).cuda())
    yield h
    h.close()


@pytest.fixture(scope="module")
def handle1(torch):
    """one scale, the plain target 0: the finest scale on its own"""
    from visgeom_amd import photometric

    s = ps.scene()
    h = photometric.Photometric(ps.CAM, params(), ps.XI_BASE_CAM, ps.W, ps.H, 1)
    h.set_base(torch.from_numpy(s["base"]).cuda(), torch.from_numpy(s["depth"]).cuda())
    h.set_targets(torch.from_numpy(s["targets"][0]).cuda())
    yield h
    h.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_evaluate_mi(torch, handle):
    loc = ms.localizer()
    poses, targets = ms.eval_poses()
    for scale in range(ps.NUM_SCALES):
        out = handle.evaluate_mi(scale, poses, targets)
        val = out["values"].cpu().numpy()
        for i in range(len(poses)):
            e = ms.reference_evaluate(scale, i)
            rev = mr.evaluate_mi(loc, scale, poses[i], int(targets[i]), reverse=True)["gradient"]
            order = np.abs(rev - e["gradient"]).max() / np.abs(e["gradient"]).max()
            failed = (~e["ok"]).mean()
            print("scale", scale, "pose", i, "failed", failed, "order sensitivity", order, "cost", e["cost"], out["cost"][i])
            assert order <= 1e-12
            if i == 4:
                assert 0.01 <= failed <= 0.5   # the rule "counted in bin 0 of the second axis" is exercised
            skip = e["slack"] < 1e-9
            assert not skip.any()   # so histogram, cost and gradient are over the same decisions (the cap would be 0.5 %)
            assert (val[i][~e["ok"]] == 0.).all()
            assert np.abs(val[i] - e["values"]).max() <= PARITY * mr.VAL_MAX
            h, hr = out["hist"][i].ravel(), e["hist"]
            assert ((h == 0.) == (hr == 0.)).all()   # exactly zero bins are zero in both
            assert np.abs(h - hr).max() <= PARITY * hr.max()
            assert abs(out["cost"][i] - e["cost"]) <= PARITY * abs(e["cost"])
            assert np.abs(out["gradient"][i] - e["gradient"]).max() <= PARITY * np.abs(e["gradient"]).max()


def test_evaluate_mi_is_deterministic_and_batch_independent(torch, handle):
    poses, targets = ms.eval_poses()
    for scale in range(ps.NUM_SCALES):
        a, b = handle.evaluate_mi(scale, poses, targets), handle.evaluate_mi(scale, poses, targets)
        lean = handle.evaluate_mi(scale, poses, targets, values=False, gradient=False)
        one = handle.evaluate_mi(scale, poses[3], targets[3:4])
        for k in ("cost", "hist", "gradient"):
            assert (bits(a[k]) == bits(b[k])).all(), k
            assert (bits(a[k][3]) == bits(one[k][0])).all(), k
        assert (bits(a["values"].cpu().numpy()) == bits(b["values"].cpu().numpy())).all()
        assert (bits(a["values"][3].cpu().numpy()) == bits(one["values"][0].cpu().numpy())).all()
        assert (bits(a["cost"]) == bits(lean["cost"])).all() and (bits(a["hist"]) == bits(lean["hist"])).all()
        assert lean["gradient"] is None and lean["values"] is None


def test_compute_pose_mi_against_the_restatement(torch, handle):
    """see the comment at COST_MARGIN"""
    loc = ms.localizer()
    ref_x, ref_rep = ms.reference_solve(0)
    x, rep = handle.compute_pose_mi(ps.start_pose(0), [0], function_tolerance=ms.TIGHT["ftol"], gradient_tolerance=ms.TIGHT["gtol"])
    print("GPU pose", x.tolist(), "report", rep.tolist(), "reference", ref_x.tolist(), [r["final_cost"] for r in ref_rep])
    cost_at_gpu = mr.evaluate_mi(loc, 0, x, 0, want_grad=False)["cost"]
    print("reference cost at the GPU pose", cost_at_gpu, "reference final", ref_rep[0]["final_cost"])
    assert cost_at_gpu <= ref_rep[0]["final_cost"] + COST_MARGIN * abs(ref_rep[0]["final_cost"])
    (et, er), (rt, rr) = ps.pose_error(x), ps.pose_error(ref_x)
    print("pose error", et, er, "reference", rt, rr)
    assert et <= rt * (1. + POSE_MARGIN) + POSE_FLOOR and er <= rr * (1. + POSE_MARGIN) + POSE_FLOOR


def test_compute_pose_mi_at_the_reference_tolerances(torch, handle, handle1):
    """two correct solvers may stop apart at a function tolerance of 1 %: only the report's shape, bounds and codes, final <=
    initial, and the initial cost where both start from the same pose: the coarsest scale of the three-scale handle, and the
    finest scale through a one-scale handle"""
    loc = ms.localizer()
    x, rep = handle.compute_pose_mi(ps.start_pose(0), [0])
    x1, rep1 = handle1.compute_pose_mi(ps.start_pose(0), [0])
    print("report", rep.tolist(), "one scale", rep1.tolist())
    assert rep.shape == (ps.NUM_SCALES, 4) and rep1.shape == (1, 4)
    for r in list(rep) + list(rep1):
        assert 0 <= r[0] <= mr.MAX_ITERATIONS and r[0] == int(r[0]) and r[2] <= r[1]
        assert r[3] in (mr.TERM_FUNCTION, mr.TERM_GRADIENT, mr.TERM_NO_CONVERGENCE, mr.TERM_FAILURE)
    _, ref_rep = ms.reference_solve(0, tight=False)
    top = ps.NUM_SCALES - 1
    assert abs(rep[top, 1] - ref_rep[top]["initial_cost"]) <= PARITY * abs(ref_rep[top]["initial_cost"])
    want = mr.evaluate_mi(loc, 0, ps.start_pose(0), 0, want_grad=False)["cost"]
    assert abs(rep1[0, 1] - want) <= PARITY * abs(want)


def test_remapped_target(torch, handle):
    """see the comment at REMAP_FACTOR: where the grey levels are remapped the photometric cost loses the pose and mutual
    information keeps it"""
    kw = {"function_tolerance": ms.TIGHT["ftol"], "gradient_tolerance": ms.TIGHT["gtol"]}
    x_plain, _ = handle.compute_pose_mi(ps.start_pose(0), [0], **kw)
    x_remap, rep = handle.compute_pose_mi(ps.start_pose(0), [ms.REMAPPED], **kw)
    x_photo, _ = handle.compute_pose(ps.start_pose(0), [ms.REMAPPED])
    (pt, pr_), (rt, rr), (ft, fr) = ps.pose_error(x_plain), ps.pose_error(x_remap), ps.pose_error(x_photo)
    print("MI plain", pt, pr_, "MI remapped", rt, rr, "photometric remapped", ft, fr, "report", rep.tolist())
    assert rt <= REMAP_FACTOR * pt and rr <= REMAP_FACTOR * pr_
    assert rt < ft and rr < fr
    (qt, qr) = ps.pose_error(ms.reference_solve(ms.REMAPPED)[0])
    assert rt <= qt * (1. + POSE_MARGIN) + POSE_FLOOR and rr <= qr * (1. + POSE_MARGIN) + POSE_FLOOR


def test_compute_pose_mi_batch_equals_single_calls(torch, handle):
    tg = [0, 1, 2, ms.REMAPPED]
    starts = np.array([ps.start_pose(k) for k in (0, 1, 2, 0)])
    xb, rb = handle.compute_pose_mi(starts, tg)
    for k in range(4):
        x1, r1 = handle.compute_pose_mi(starts[k], [tg[k]])
        assert (bits(x1) == bits(xb[k])).all() and (bits(r1) == bits(rb[k])).all()
        e0, e1 = ps.pose_error(starts[k], tg[k] % 3), ps.pose_error(xb[k], tg[k] % 3)   # every target is approached
        assert e1[0] < 0.5 * e0[0] and e1[1] < 0.5 * e0[1], (k, e0, e1)


def test_odometry_term(torch, handle, handle1):
    """the added cost and gradient are host arithmetic (held to the restatement in tests/test_mi_cpu.py); here through the
    solve: after one iteration the reported cost is the restatement's cost plus its odometry term at the reported pose, and
    the solved pose lies closer to the start pose than without the term"""
    from visgeom_amd import photometric

    loc = ms.localizer()
    x0 = np.array(ps.start_pose(0))
    x1, rep = handle1.compute_pose_mi(x0, [0], xi_odom=ms.XI_ODOM, max_iterations=1)
    assert rep[0, 0] == 1 and np.abs(x1 - x0).max() > 1e-4
    odom = mr.MiOdometry(ms.XI_ODOM, x0)
    want = mr.evaluate_mi(loc, 0, x1, 0, want_grad=False)["cost"] + odom.evaluate(x1)[0]
    c, g = photometric.mi_odometry(ms.XI_ODOM, x0, x1)
    print("odometry term", c, odom.evaluate(x1)[0], "cost", rep[0, 2], want)
    assert abs(c - odom.evaluate(x1)[0]) <= PARITY * c and np.abs(g - odom.evaluate(x1)[1]).max() <= PARITY * np.abs(g).max()
    assert c > 1e-6 * abs(want)   # the term is visible in the sum
    assert abs(rep[0, 2] - want) <= PARITY * abs(want)
    kw = {"function_tolerance": ms.TIGHT["ftol"], "gradient_tolerance": ms.TIGHT["gtol"]}
    free, _ = handle.compute_pose_mi(x0, [0], **kw)
    held, _ = handle.compute_pose_mi(x0, [0], xi_odom=ms.XI_ODOM, **kw)
    print("free", np.linalg.norm(free - x0), "held", np.linalg.norm(held - x0))
    assert np.linalg.norm(held - x0) < np.linalg.norm(free - x0)


def test_refusals(torch, handle):
    from visgeom_amd import capi, photometric

    poses, targets = ms.eval_poses()

    def refused(fn):
        with pytest.raises(capi.VisgeomError) as e:
            fn()
        assert e.value.code == capi.ERR_INVALID_ARGUMENT

    s = ps.scene()
    fresh = photometric.Photometric(ps.CAM, params(), ps.XI_BASE_CAM, ps.W, ps.H, ps.NUM_SCALES)
    refused(lambda: fresh.evaluate_mi(0, poses, targets, values=False))      # before set_base
    refused(lambda: fresh.compute_pose_mi(poses[0], [0]))
    fresh.set_base(torch.from_numpy(s["base"]).cuda(), torch.from_numpy(s["depth"]).cuda())
    refused(lambda: fresh.evaluate_mi(0, poses, targets, values=False))      # before set_targets
    refused(lambda: fresh.compute_pose_mi(poses[0], [0]))
    fresh.set_base(torch.from_numpy(s["base"]).cuda(), torch.zeros_like(torch.from_numpy(s["depth"])).cuda())   # no depth: empty packs
    fresh.set_targets(torch.from_numpy(s["targets"]).cuda())
    assert [int(fresh.pack(i)[0].numel()) for i in range(ps.NUM_SCALES)] == [0, 0, 0]
    refused(lambda: fresh.evaluate_mi(1, poses, targets, values=False))
    refused(lambda: fresh.compute_pose_mi(poses[0], [0]))
    fresh.close()
    L = capi.load()
    import ctypes
    dp, i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    cost = np.zeros(5)
    for scale in (ps.NUM_SCALES, -1):   # the wrapper checks the scale itself: the library's own check
        assert L.vg_mi_evaluate(handle._h, scale, 5, poses.ctypes.data_as(dp), targets.ctypes.data_as(i32p), None, None,
                                            cost.ctypes.data_as(dp), None) == capi.ERR_INVALID_ARGUMENT
    refused(lambda: handle.evaluate_mi(0, poses, [0, 0, 1, 4, 0], values=False))   # four targets: index 4 is out of range
    refused(lambda: handle.compute_pose_mi(poses[0], [-1]))
    bad = poses.copy()
    bad[2, 4] = np.nan
    refused(lambda: handle.evaluate_mi(0, bad, targets, values=False))
    refused(lambda: handle.compute_pose_mi(bad[2], [0]))
    bad[2, 4] = np.inf
    refused(lambda: handle.evaluate_mi(0, bad, targets, values=False))
    with pytest.raises(ValueError):
        handle.evaluate_mi(ps.NUM_SCALES, poses, targets)
