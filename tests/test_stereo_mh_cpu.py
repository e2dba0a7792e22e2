"""Multi-hypothesis stereo without a GPU: the restatement (tests/stereo_mh_ref.py) against hand-derived cost rows and small
hand-made maps, and the three new entries declared in the header, exported from both libraries and bound."""
import os
import re
import subprocess

import numpy as np

from tests import stereo_mh_ref as smh

ENTRIES = ("vg_stereo_compute_mh", "vg_depth_regularize", "vg_depth_pack_mh")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = smh.NO_COST
BAD = 99   # a matching error above EMAX
EMAX = 10


def rows(c, err=None):
    """(err, total) of one pixel from the costs c = total - 2 err wanted at every disparity"""
    err = np.array(err if err is not None else [0] * len(c), np.uint8)
    return err, np.array(c, np.int64) + 2 * err.astype(np.int64)


def pick(c, hyp, diff, err=None):
    return smh.select_row(*rows(c, err), EMAX, hyp, diff)


def test_skipped_disparity_between_a_minimum_and_its_successor():
    # V = 0 1 3 4 with c = 9 3 7 8: the minimum at d = 1 is seen when d = 3 arrives and reports 3 - 1 = 2, the skipped one
    err = [0, 0, BAD, 0, 0]
    assert smh.candidates(*rows([9, 3, 0, 7, 8], err), EMAX) == [(3, 2)]
    assert pick([9, 3, 0, 7, 8], 2, 10, err) == ([2, -1], [3, NONE])
    # two skipped ones: the report is the last of them
    assert smh.candidates(*rows([9, 3, 0, 0, 7], [0, 0, BAD, BAD, 0]), EMAX) == [(3, 3)]


def test_first_valid_disparity_as_a_minimum():
    assert smh.candidates(*rows([0, 2, 5, 6], [BAD, 0, 0, 0]), EMAX) == [(2, 1)]   # V starts at 1: no predecessor to compare with
    # d = 0 is valid here, unlike in the single-hypothesis winner; the plateau 4 4 gives its second element (<= before, < after)
    assert smh.candidates(*rows([1, 4, 4, 5]), EMAX) == [(1, 0), (4, 2)]
    assert pick([1, 4, 4, 5], 3, 10) == ([0, 2, -1], [1, 4, NONE])
    # a cost of 0 equals the initial m = 0 and passes because its disparity is not the initial -1
    assert pick([0, 3], 2, 10) == ([0, -1], [0, NONE])


def test_last_valid_disparity_is_never_a_minimum():
    assert smh.candidates(*rows([5, 4, 3, 2]), EMAX) == []
    assert pick([5, 4, 3, 2], 2, 10) == ([-1, -1], [NONE, NONE])
    assert pick([5, 3, 4, 1], 2, 10) == ([1, -1], [3, NONE])
    assert smh.candidates(*rows([5, 3, 4, 1, 0], [0, 0, 0, 0, BAD]), EMAX) == [(3, 1)]   # the last VALID one: d = 3


def test_two_way_tie_alternates():
    assert smh.candidates(*rows([7, 5, 9, 5, 8]), EMAX) == [(5, 1), (5, 3)]
    assert pick([7, 5, 9, 5, 8], 4, 10) == ([1, 3, 1, 3], [5, 5, 5, 5])
    assert pick([7, 5, 9, 5, 8], 4, 0) == ([1, 3, 1, 3], [5, 5, 5, 5])   # a gap of 0 is within any hypo_difference >= 0


def test_gate_is_measured_from_the_previous_hypothesis():
    c = [20, 10, 30, 18, 40, 26, 50]
    assert smh.candidates(*rows(c), EMAX) == [(10, 1), (18, 3), (26, 5)]
    assert pick(c, 4, 8) == ([1, 3, 5, -1], [10, 18, 26, NONE])   # 26 > 10 + 8, but 26 <= 18 + 8
    assert pick(c, 4, 7) == ([1, -1, -1, -1], [10, NONE, NONE, NONE])
    assert pick([2000, 1000, 3000], 2, 5) == ([1, -1], [1000, NONE])   # hypothesis 0 has no gate


def test_no_candidate_at_all():
    assert pick([1, 2, 3], 3, 10, [BAD, BAD, BAD]) == ([-1] * 3, [NONE] * 3)
    assert pick([1, 2, 3], 3, 10, [BAD, 0, BAD]) == ([-1] * 3, [NONE] * 3)   # one valid disparity has no successor
    assert pick([4, 4, 4], 3, 10) == ([-1] * 3, [NONE] * 3)                  # a plateau never falls below its successor
    assert smh.select([], 2, 10) == ([-1, -1], [NONE, NONE])


def test_winner_switches_off_non_salient_pixels_only():
    err, tot = rows([7, 5, 9, 5, 8])
    err, tot = np.stack([err, err])[None], np.stack([tot, tot])[None]   # [1][2][5]
    sal = np.array([[1, 0]], np.uint8)
    d, c = smh.winner_mh(dict(salient_points_only=1, error_max=EMAX), err, tot, sal, 2, 10)
    assert d[:, 0, 0].tolist() == [1, 3] and d[:, 0, 1].tolist() == [-1, -1] and c[:, 0, 1].tolist() == [NONE, NONE]
    d, _ = smh.winner_mh(dict(salient_points_only=0, error_max=EMAX), err, tot, sal, 2, 10)
    assert d[:, 0, 1].tolist() == [1, 3]


def test_regularize_hand_made_map():
    # four pixels, three planes; sigma and cost are 10 h + pixel and 100 + the same
    depth = np.array([[0., 2., 3.], [0.1, 0., 5.], [1., 0.2, 0.25], [0., 0.1, 0.2]]).T.reshape(3, 1, 4).copy()
    sigma = (10. * np.arange(3)[:, None, None] + np.arange(4)[None, None, :]) * np.ones((3, 1, 4))
    cost = sigma + 100.
    d, s, c = smh.regularize(depth, sigma, cost)
    assert d[:, 0, 0].tolist() == [2., 3., 0.] and s[:, 0, 0].tolist() == [10., 20., 20.]     # both filled planes move down
    assert d[:, 0, 1].tolist() == [5., 0., 0.] and s[:, 0, 1].tolist() == [21., 11., 21.]     # 0.1 counts as empty and is overwritten
    assert d[:, 0, 2].tolist() == [1., 0.25, 0.] and s[:, 0, 2].tolist() == [2., 22., 22.]    # 0.25 is filled, 0.2 is not
    assert d[:, 0, 3].tolist() == [0., 0.1, 0.2] and s[:, 0, 3].tolist() == [3., 13., 23.]    # nothing to move: nothing cleared
    np.testing.assert_array_equal(c, s + 100.)
    assert depth[0, 0, 0] == 0. and smh.holes(depth) == 4 and smh.holes(d) == 0


def test_pack_hand_made_map():
    cam = [0.6, 1., 100., 10., 0., 0.]
    prm = dict(scale=30, u0=0, v0=0)   # row 1 is at v = 30, yn = 3: 1 - (2 alpha - 1) beta 9 < 0, the camera refuses it
    depth = np.array([[[2., 3.], [0.2, 1.]], [[0.1, 4.], [5., 0.25]]])     # [2][2][2]
    sigma = np.arange(8.).reshape(2, 2, 2)
    idx, hyp, cloud, sig = smh.pack_mh(cam, prm, depth, sigma)
    # pixel 0: plane 0 only (0.1 is below MIN_DEPTH); pixel 1: both planes; pixel 2: plane 0 is empty, so its plane 1 is never
    # asked; pixel 3: both planes, 0.25 included, not reconstructed
    assert idx.tolist() == [0, 1, 1, 3, 3] and hyp.tolist() == [0, 0, 1, 0, 1] and sig.tolist() == [0., 1., 5., 3., 7.]
    assert cloud[0].tolist() == [0., 0., 2.] and cloud[3].tolist() == [0., 0., 0.] and cloud[4].tolist() == [0., 0., 0.]
    np.testing.assert_allclose(np.linalg.norm(cloud[1:3], axis=1), [3., 4.], rtol=1e-15)
    assert cloud[1, 0] > 0. and cloud[1, 1] == 0. and np.allclose(cloud[2], cloud[1] * 4. / 3., rtol=1e-15)
    assert [len(a) for a in smh.pack_mh(cam, prm, np.zeros((2, 2, 2)), sigma)] == [0, 0, 0, 0]


def test_entries_declared_exported_and_bound():
    from visgeom_amd import _build, capi

    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "visgeom_amd.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.SIGNATURES, name
        assert getattr(lib, name).argtypes is not None
    for path in (_build.LIB, _build.build_production()):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in ENTRIES:
            assert re.search(r" T %s$" % name, out, re.M), (path, name)
    assert lib.vg_abi_version() == 1
    # the arguments are checked before HIP is touched: no handle, no device needed
    assert lib.vg_stereo_compute_mh(None, 1, None, None, 4, None, None, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_depth_regularize(None, 1, 4, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_depth_pack_mh(None, 4, None, None, None, None, None, None, None) == capi.ERR_INVALID_ARGUMENT


def test_hypotheses_in_the_parameters_stay_refused():
    """the hypothesis count is an argument of vg_stereo_compute_mh; the struct field and the JSON key must still be 1"""
    import ctypes

    from tests import stereo_scene
    from visgeom_amd import capi, stereo

    lib = capi.load()
    p = stereo.make_params(u_max=125, v_max=93, u0=15, v0=15, equal_margins=1, disp_max=32, hypotheses=4)
    h = ctypes.c_void_p()
    dp = ctypes.POINTER(ctypes.c_double)
    arr = [np.ascontiguousarray(a, dtype=np.float64) for a in (stereo_scene.CAM1, stereo_scene.CAM2, stereo_scene.RIGS["sideways"])]
    assert lib.vg_stereo_create(ctypes.byref(h), 0, None, *[a.ctypes.data_as(dp) for a in arr], ctypes.byref(p)) == capi.ERR_INVALID_ARGUMENT
    assert b"hypotheses must be 1" in lib.vg_last_error()
