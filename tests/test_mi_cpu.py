"""The mutual-information restatement (tests/mi_ref.py) against itself -- histogram sums, its gradient against central
differences, the cost falling towards the true pose with and without a grey-level remap -- and the new entries of the C ABI:
declared, exported, bound, their host-side refusals and the host-only odometry term.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mi_ref as mr
from tests import mi_scene as ms
from tests import photometric_scene as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vg_mi_evaluate", "vg_mi_compute_pose", "vg_mi_odometry")


def test_shares_by_hand():
    """histStep = 255 / 7: 0 and 255 sit on the outer bins without a neighbour, half a step above bin 3 shares 1/2 with bin 4
    (round half away from zero makes bin 4 the first), values beyond the range are clamped with share 0"""
    step = 255. / 7
    i1, i2, s = mr.shares(np.array([0., 255., 3.5 * step, 3.25 * step, 2.75 * step, -30., 300., 0.25 * step]))
    assert i1.tolist() == [0, 7, 4, 3, 3, 0, 7, 0] and i2.tolist() == [-1, -1, 3, 4, 2, -1, -1, 1]
    assert np.allclose(s, [1., 1., 0.5, 0.875, 0.875, 0., 0., 0.875], atol=1e-15)
    _, j2, der = mr.share_derivative(np.array([3.25 * step, 2.75 * step, 0., 300.]))
    assert j2.tolist() == [4, 2, -1, -1] and np.allclose(der, [-1. / step, 1. / step, 0., 0.], atol=1e-15)
    # a clamped value still counts: the whole increment goes to the outer bin
    assert mr.hist(np.array([-30., 300., 0.]))[[0, 7]].tolist() == [2. / 3, 1. / 3]


def test_histograms_sum_to_one():
    for scale in range(ps.NUM_SCALES):
        for i in range(5):
            e = ms.reference_evaluate(scale, i)
            h = e["hist"].reshape(mr.NUM_BINS, mr.NUM_BINS)
            assert abs(h.sum() - 1.) <= 1e-13 and abs(e["hist1"].sum() - 1.) <= 1e-13
            assert np.abs(h.sum(0) - e["hist1"]).max() <= 1e-13    # the first axis is the key frame
            assert np.abs(h.sum(1) - e["hist2"]).max() <= 1e-13


def test_failing_pose_is_counted_in_bin_zero():
    for scale in range(ps.NUM_SCALES):
        e = ms.reference_evaluate(scale, 4)
        frac = (~e["ok"]).mean()
        assert 0.01 <= frac <= 0.5, frac
        assert (e["values"][~e["ok"]] == 0.).all() and (e["terms"][~e["ok"]] == 0.).all()
        assert e["hist2"][0] >= frac - 1e-13   # every failed point puts its whole increment into row 0
        assert e["slack"].min() > 1e-9


def test_gradient_matches_central_differences():
    """The cost is C1 with a piecewise continuous second derivative (the neighbour bin of a share changes at a bin centre, the
    bicubic's second derivative jumps at pixel borders), so a central difference is first order in h, not round-off small.
    Measured over the twelve (scale, pose) cases below, relative to max|g|: h = 1e-5: at most 1.0e-4; h = 1e-6: at most 2.1e-6.
    The bars are ten times that."""
    loc = ms.localizer()
    poses, targets = ps.eval_poses()
    for scale in range(ps.NUM_SCALES):
        for i, (xi, k) in enumerate(zip(poses, targets)):
            g = ms.reference_evaluate(scale, i)["gradient"]
            for h, bar in ((1e-5, 1e-3), (1e-6, 2e-5)):
                num = np.zeros(6)
                for j in range(6):
                    d = np.zeros(6)
                    d[j] = h
                    num[j] = (mr.evaluate_mi(loc, scale, xi + d, int(k), want_grad=False)["cost"] -
                              mr.evaluate_mi(loc, scale, xi - d, int(k), want_grad=False)["cost"]) / (2 * h)
                err = np.abs(num - g).max() / np.abs(g).max()
                print("scale", scale, "pose", i, "h", h, "error", err)
                assert err <= bar, (scale, i, h, err)


def test_cost_falls_towards_the_truth():
    """cost at the truth < at half the start offset < at the start pose, at every scale, plain and remapped.  The values, plain:
    -0.927 / -0.446 / -0.142, -0.816 / -0.499 / -0.206, -0.574 / -0.435 / -0.219; remapped: -0.382 / -0.242 / -0.092,
    -0.334 / -0.244 / -0.120, -0.229 / -0.190 / -0.110 (scales 0, 1, 2)."""
    loc = ms.localizer()
    want = {0: [(-0.927, -0.446, -0.142), (-0.816, -0.499, -0.206), (-0.574, -0.435, -0.219)],
            ms.REMAPPED: [(-0.382, -0.242, -0.092), (-0.334, -0.244, -0.120), (-0.229, -0.190, -0.110)]}
    assert [len(p["val"]) for p in loc.packs] == [24606, 6806, 1366]
    for target in (0, ms.REMAPPED):
        for scale in range(ps.NUM_SCALES):
            es = [mr.evaluate_mi(loc, scale, ps.start_pose(0, f), target, want_grad=False) for f in (0., 0.5, 1.)]
            c = [e["cost"] for e in es]
            assert all(e["ok"].all() for e in es)   # every point projects at these poses
            assert c[0] < c[1] < c[2] < 0., (target, scale, c)
            assert np.abs(np.array(c) - want[target][scale]).max() < 5e-4, (target, scale, c)


def test_odometry_term():
    x0 = np.array(ps.start_pose(0))
    o = mr.MiOdometry(ms.XI_ODOM, x0)
    c, g = o.evaluate(x0)
    assert c < 1e-30 and np.abs(g).max() < 1e-12   # err = prior^-1 o prior is zero up to the quaternion product's rounding
    x = x0 + [0.01, -0.02, 0.005, 0.003, -0.002, 0.004]
    c, g = o.evaluate(x)
    num = np.zeros(6)
    for j in range(6):
        d = np.zeros(6)
        d[j] = 1e-6
        num[j] = (o.evaluate(x + d)[0] - o.evaluate(x - d)[0]) / 2e-6
    # the reference's J is the Jacobian of err C err^T / 2 only to first order in err (it is built at the prior): 10 %
    assert c > 0. and np.abs(num - g).max() <= 0.1 * np.abs(g).max()


@pytest.fixture(scope="module")
def lib():
    from visgeom_amd import _build, capi

    _build.build()
    return capi.load()


def test_symbols_declared_exported_bound(lib):
    from visgeom_amd import _build, capi

    with open(os.path.join(ROOT, "include", "visgeom_amd.h")) as fh:
        header = fh.read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in capi.SIGNATURES and hasattr(lib, name)
    for const in ("VG_MI_NUM_BINS 8", "VG_MI_VALUE_MAX 255.0", "VG_MI_FUNCTION_TOLERANCE 1e-2", "VG_MI_GRADIENT_TOLERANCE 1e-3",
                  "VG_MI_MAX_ITERATIONS 50", "VG_MI_ODOMETRY_DAMPING 0.0002"):
        assert "#define " + const in header
    out = subprocess.check_output(["nm", "-D", "--defined-only", _build.LIB], text=True)
    for name in SYMBOLS:
        assert " T %s\n" % name in out
    with open(os.path.join(ROOT, "visgeom_amd", "csrc", "vg_photometric_tu.hip")) as fh:
        tu = fh.read()
    assert '#include "vg_photometric_mi.hpp"' in tu
    assert [f[0] for f in capi.MiOptions._fields_] == ["function_tolerance", "gradient_tolerance", "max_iterations"]
    assert capi.MI_DEFAULTS == {"function_tolerance": mr.FTOL, "gradient_tolerance": mr.GTOL, "max_iterations": mr.MAX_ITERATIONS}


def test_refusals_without_a_gpu(lib):
    """a NULL handle and NULL arguments are refused before HIP is touched"""
    from visgeom_amd import capi

    dp, i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    xi, tg, out = np.zeros(6), np.zeros(1, np.int32), np.zeros(6)
    P = lambda a: a.ctypes.data_as(dp)
    assert lib.vg_mi_evaluate(None, 0, 1, P(xi), tg.ctypes.data_as(i32p), None, None, P(out), None) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_mi_compute_pose(None, 1, P(xi), tg.ctypes.data_as(i32p), None, None, P(out), None) == capi.ERR_INVALID_ARGUMENT
    c = ctypes.c_double()
    assert lib.vg_mi_odometry(None, P(xi), P(xi), ctypes.byref(c), None) == capi.ERR_INVALID_ARGUMENT
    bad = np.array([0., 0., np.nan, 0., 0., 0.])
    assert lib.vg_mi_odometry(P(xi), P(xi), P(bad), ctypes.byref(c), None) == capi.ERR_INVALID_ARGUMENT


def test_library_odometry_term_matches_the_restatement(lib):
    """host arithmetic: the library's MutualInformationOdom term against the restatement's at 1e-12 of the largest entry"""
    from visgeom_amd import photometric

    rnd = np.random.default_rng(7)
    for odom in (ms.XI_ODOM, [0.2, -0.1, 0.05, 0.01, 0.02, -0.4], [0., 0., 0., 0., 0., 0.]):
        prior = np.array(ps.start_pose(0)) + rnd.normal(size=6) * 0.1
        x = prior + rnd.normal(size=6) * 0.02
        c, g = photometric.mi_odometry(odom, prior, x)
        cr, gr = mr.MiOdometry(odom, prior).evaluate(x)
        assert abs(c - cr) <= 1e-12 * cr and np.abs(g - gr).max() <= 1e-12 * np.abs(gr).max()
        c1, _ = photometric.mi_odometry(odom, prior, prior)
        assert c1 < 1e-30
