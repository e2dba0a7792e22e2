"""Point clouds, the plane prior and the accuracy score without a GPU: the restatement (tests/cloud_ref.py) on hand-made maps, one
pixel per branch; the restatement against stereo_mh_ref.pack_mh; the argument checks of the three entries, which need neither a
handle nor a device; the refusals of the stereo_accuracy program, which reads and checks everything before the GPU is touched;
and the new symbols declared, exported from both libraries and bound."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cloud_ref as cr
from tests import stereo_mh_ref as smh
from tests import stereo_mh_shapes as ms
from tests import stereo_ref as sr

ENTRIES = ("vg_depth_reconstruct", "vg_depth_generate_plane", "vg_depth_compare")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
CAM = [0.6, 1., 100., 10., 0., 0.]
PRM = dict(scale=30, u0=0, v0=0, x_max=2, y_max=2)   # row 1 is at v = 30, yn = 3: 1 - (2 alpha - 1) beta 9 < 0, the camera refuses it


def hand_map():
    """[1][3][2][2]: pixel 0 has an empty plane 0 under a filled one, pixel 1 a hole between two filled planes, pixel 2 (refused by
    the camera) two planes, pixel 3 (refused) NaN in plane 0; sigma = 10 h + pixel + 1"""
    per_pixel = [[0., 2., 0.], [1., 0., 3.], [2., 0.5, 0.], [NAN, 0., 0.]]
    depth = np.array(per_pixel).T.reshape(1, 3, 2, 2).copy()
    sigma = (10. * np.arange(3)[:, None] + np.arange(4)[None, :] + 1.).reshape(1, 3, 2, 2)
    return depth, sigma


def ray(u, v, d=1.):
    X = sr.reconstruct(CAM, float(u), float(v))
    n = math.sqrt(sr.dot3(X, X))
    return [c / n * d for c in X]


def test_no_query_takes_the_pixels_with_a_depth_in_plane_0():
    depth, sigma = hand_map()
    r = cr.reconstruct(CAM, PRM, depth, sigma)
    assert r["indices"].tolist() == [1, 2] and r["hyp"].tolist() == [0, 0] and r["counts"].tolist() == [2]
    assert r["points"].tolist() == [[30., 0.], [0., 30.]] and r["valid"].tolist() == [1, 0] and r["item"].tolist() == [0, 0]
    assert r["cloud"][0].tolist() == ray(30, 0) and r["cloud"][1].tolist() == [0., 0., 0.]
    assert r["sigma"] is None and r["index_map"] is None
    # an empty plane 0 closes the pixel even when a plane above holds a depth, with or without DEFAULT_VALUES: getIdxVec decides
    r = cr.reconstruct(CAM, PRM, depth, sigma, cr.ALL_HYPOTHESES | cr.DEFAULT_VALUES | cr.SIGMA_VALUE)
    assert r["indices"].tolist() == [1, 1, 2, 2] and r["hyp"].tolist() == [0, 2, 0, 1]   # the hole at (1, 1) is skipped
    assert r["sigma"].tolist() == [2., 22., 3., 13.]
    assert [len(a) for a in (cr.reconstruct(CAM, PRM, np.zeros((1, 3, 2, 2)))[k] for k in ("indices", "cloud"))] == [0, 0]


def test_query_indices_outside_duplicated_and_empty():
    depth, sigma = hand_map()
    q = [0, -1, 4, 1, 1, 3]   # 4 = x_max y_max: the reference's "> hStep" lets it through, the contract does not
    r = cr.reconstruct(CAM, PRM, depth, sigma, cr.QUERY_INDICES | cr.ALL_HYPOTHESES | cr.INDEX_MAPPING, query_indices=q)
    assert r["indices"].tolist() == [0, 1, 1, 1, 1] and r["hyp"].tolist() == [1, 0, 2, 0, 2]   # pixel 0: plane 1 although plane 0 is empty
    assert r["index_map"].tolist() == [0, 3, 3, 4, 4]
    # QUERY_INDICES is stronger than QUERY_POINTS: the points are not looked at
    r2 = cr.reconstruct(CAM, PRM, depth, sigma, cr.QUERY_INDICES | cr.QUERY_POINTS | cr.ALL_HYPOTHESES | cr.INDEX_MAPPING,
                        query_points=[[1e9, 1e9]] * 6, query_indices=q)
    assert all(np.array_equal(r[k], r2[k]) for k in ("indices", "hyp", "index_map", "cloud", "points"))


def test_default_values_fill_plane_0_only():
    depth, sigma = hand_map()
    r = cr.reconstruct(CAM, PRM, depth, sigma, cr.QUERY_INDICES | cr.DEFAULT_VALUES | cr.SIGMA_VALUE, query_indices=[0, 3, 1])
    assert r["indices"].tolist() == [0, 3, 1] and r["hyp"].tolist() == [0, 0, 0]
    assert r["sigma"].tolist() == [30., 30., 2.]                      # NaN counts as below MIN_DEPTH
    assert r["cloud"][0].tolist() == [0., 0., 5.] and r["cloud"][1].tolist() == [0., 0., 0.] and r["valid"].tolist() == [1, 0, 1]
    r = cr.reconstruct(CAM, PRM, depth, sigma, cr.QUERY_INDICES | cr.DEFAULT_VALUES | cr.ALL_HYPOTHESES, query_indices=[0, 3])
    assert r["indices"].tolist() == [0, 0, 3] and r["hyp"].tolist() == [0, 1, 0]   # the default at h = 0, no default above
    r = cr.reconstruct(CAM, PRM, depth, sigma, cr.QUERY_INDICES, query_indices=[0, 3])
    assert r["counts"].tolist() == [0]


def test_minmax_is_clamped_at_min_depth():
    depth, sigma = hand_map()
    r = cr.reconstruct(CAM, PRM, depth, sigma, cr.MINMAX | cr.SIGMA_VALUE | cr.QUERY_INDICES, query_indices=[1])
    assert r["cloud"].shape == (1, 2, 3)
    assert r["cloud"][0, 0].tolist() == ray(30, 0, 0.25) and r["cloud"][0, 1].tolist() == ray(30, 0, 7.)   # 1 -+ 3 * 2
    sigma[0, 0, 0, 1] = 0.125
    r = cr.reconstruct(CAM, PRM, depth, sigma, cr.MINMAX, query_indices=None)
    assert r["cloud"][0, 0].tolist() == ray(30, 0, 0.625) and r["cloud"][0, 1].tolist() == ray(30, 0, 1.375)
    assert r["cloud"][1].tolist() == [[0.] * 3] * 2   # the refused pixel: both ends (0, 0, 0)
    # the default entry: max(5 - 90, MIN_DEPTH) and 95
    r = cr.reconstruct(CAM, PRM, depth, sigma, cr.MINMAX | cr.DEFAULT_VALUES | cr.QUERY_INDICES, query_indices=[0])
    assert r["cloud"][0].tolist() == [[0., 0., 0.25], [0., 0., 95.]]


def test_query_points_round_half_away_from_zero_and_keep_their_ray():
    depth, sigma = hand_map()
    pts = [[15., 0.], [-15., 0.], [-14.9, 0.], [44.9, 0.], [45., 0.], [NAN, 0.], [0., math.inf], [30., -14.9]]
    r = cr.reconstruct(CAM, PRM, depth, sigma, cr.QUERY_POINTS | cr.INDEX_MAPPING | cr.DEFAULT_VALUES, query_points=pts)
    # x + 0.5 goes up to pixel 1; -0.5 goes to -1, outside; -0.4967 to pixel 0 (empty: the default); 1.4967 to 1; 1.5 to 2, outside
    assert r["index_map"].tolist() == [0, 2, 3, 7] and r["indices"].tolist() == [1, 0, 1, 1]
    assert r["points"].tolist() == [pts[0], pts[2], pts[3], pts[7]]                  # the query point, not the pixel's
    assert r["cloud"][0].tolist() == ray(15, 0) and r["cloud"][0].tolist() != ray(30, 0)
    assert r["cloud"][1].tolist() == ray(-14.9, 0, 5.)
    np.testing.assert_allclose(np.linalg.norm(r["cloud"], axis=1), [1., 5., 1., 1.], rtol=1e-15)
    assert cr.cround_f(0.49999999999999994) == 0. and cr.cround_f(-2.5) == -3. and cr.cround_f(2.5) == 3.


def test_poses_move_valid_points_only_and_items_keep_their_order():
    depth, sigma = hand_map()
    two = np.concatenate([depth, depth[:, :, ::-1].copy()])   # item 1: the rows swapped, so its pixels 0 and 1 hold (2, 0.5, 0) and NaN
    poses = [[1., 2., 3., 0., 0., 0.], [0., 0., 0., 0., 0., math.pi / 2]]
    r = cr.reconstruct(CAM, PRM, two, None, 0, poses=poses)
    assert r["counts"].tolist() == [2, 2] and r["item"].tolist() == [0, 0, 1, 1] and r["indices"].tolist() == [1, 2, 0, 3]
    assert r["cloud"][0].tolist() == [a + b for a, b in zip(ray(30, 0), (1., 2., 3.))]
    assert r["cloud"][1].tolist() == [0., 0., 0.]             # a failed entry stays at the origin under a pose
    np.testing.assert_allclose(r["cloud"][2], [0., 0., 2.], atol=1e-15)
    plain = cr.reconstruct(CAM, PRM, two, None, 0)
    np.testing.assert_allclose(np.linalg.norm(r["cloud"][2:], axis=1), np.linalg.norm(plain["cloud"][2:], axis=1), rtol=1e-15)


@pytest.mark.parametrize("P", (63, 259))
def test_all_hypotheses_with_sigma_is_the_pack(P):
    prm, depth, sigma = ms.small(P, "random")
    r = cr.reconstruct(ms.CAM, prm, depth[None], sigma[None], cr.ALL_HYPOTHESES | cr.SIGMA_VALUE)
    want = smh.pack_mh(ms.CAM, prm, depth, sigma)
    for got, w in zip((r["indices"], r["hyp"], r["cloud"], r["sigma"]), want):
        np.testing.assert_array_equal(ms.bits(got) if got.dtype == np.float64 else got, ms.bits(w) if w.dtype == np.float64 else w)
    assert r["counts"].tolist() == [len(want[0])] and r["valid"].all()


def test_compare_every_branch():
    prm = dict(scale=1, u0=0, v0=0, x_max=8, y_max=1)
    truth = np.array([[0., 2., NAN, 2., 2., 2., 2., 2.]], np.float32)
    depth = np.array([[1., 0., 1., NAN, 1.5, 1.5 + 1e-9, 1.5, 2.25]])
    sigma = np.array([[1., 1., 1., 1., 11., 0.5, 0.25, NAN]])
    r = cr.compare(prm, depth, sigma, truth)
    # truth 0; depth 0; NaN truth (it counts as ground truth: NaN != 0); NaN depth; sigma > 10; |diff| == sigma after the rounding to
    # float (an inlier: the test is >); |diff| > sigma; NaN sigma (an inlier: both comparisons are false)
    assert r["counts"] == (7, 4, 2) and r["inliers"].tolist() == [[0, 0, 0, 0, 0, 255, 0, 255]]
    assert r["terms"] == dict(err=[0.5, -0.25], err2=[0.25, 0.0625], dist=[2., 2., 2., 2.])
    assert [tuple(float(v) for v in h[:2]) for h in r["hist"]] == [(0.5, 2.), (0.5, 2.), (0.5, 2.), (-0.25, 2.)]
    fig = cr.figures(r["counts"], [math.fsum(r["terms"][k]) for k in ("err", "err2", "dist")])
    assert fig == (125., math.sqrt(0.3125 / 2) * 1000, 50., 2., 2 / 7)
    assert cr.compare(prm, depth, sigma, truth, sigma_max=12.)["counts"] == (7, 4, 3)
    none = cr.compare(prm, np.zeros((1, 8)), sigma, truth)
    fig = cr.figures(none["counts"], [0., 0., 0.])
    assert none["counts"] == (7, 0, 0) and all(math.isnan(v) for v in fig[:4]) and fig[4] == 0.   # N / Ngt has its denominator
    # the truth is read at (vConv(y), uConv(x)), the pixels in the reference's column-major order
    prm2 = dict(scale=2, u0=1, v0=0, x_max=2, y_max=2)
    t2 = np.zeros((3, 4), np.float32)
    t2[0, 1], t2[0, 3], t2[2, 1], t2[2, 3] = 1., 2., 3., 4.
    r = cr.compare(prm2, np.full((2, 2), 1.), np.full((2, 2), 5.), t2)
    assert r["terms"]["dist"] == [1., 3., 2., 4.] and r["counts"] == (4, 4, 4)


PLANE_CAM = [0.6, 1.05, 127., 125., 128., 96.]
PLANE_PRM = dict(scale=32, u0=0, v0=0, x_max=9, y_max=7)   # pixel (4, 3) is the principal point: its ray is the z axis
SQUARE = [[-1., -1., 0.], [1., -1., 0.], [1., 1., 0.], [-1., 1., 0.]]


def test_generate_plane_in_front_behind_and_edge_on():
    d, s, c, _, _ = cr.generate_plane(PLANE_CAM, PLANE_PRM, [0., 0., 2., 0., 0., 0.], SQUARE)
    assert d[3, 4] == 2. and s[3, 4] == 1. and (c == 5.).all() and ((d > 0) == (s == 1.)).all()
    inside = d > 0
    assert 0 < inside.sum() < d.size and not inside[0, 0]       # the far corners look past the square
    for y, x in zip(*np.nonzero(inside)):                        # |ray| (t . z) / (z . ray): the point lies on the plane z = 2
        X = sr.reconstruct(PLANE_CAM, x * 32., y * 32.)
        assert abs(d[y, x] * X[2] / math.sqrt(sr.dot3(X, X)) - 2.) < 1e-14
    # behind the camera t . z is negative and the reference's norm() still gives a positive depth: the plane's mirror image
    db, _, _, _, _ = cr.generate_plane(PLANE_CAM, PLANE_PRM, [0., 0., -2., 0., 0., 0.], SQUARE)
    assert db[3, 4] == 2.
    # edge on: the plane's z axis is the camera's x axis, z . ray < 1e-3 on the axis and to its left
    de, se, _, _, zdot = cr.generate_plane(PLANE_CAM, PLANE_PRM, [0., 0., 2., 0., math.pi / 2, 0.], SQUARE)
    assert (zdot[:, :5] < 1e-3).all() and (de[:, :5] == 0.).all() and (se[:, :5] == 0.).all()
    # the other winding: every ray is outside
    assert (cr.generate_plane(PLANE_CAM, PLANE_PRM, [0., 0., 2., 0., 0., 0.], SQUARE[::-1])[0] == 0.).all()


def test_generate_plane_triangle_and_16_gon():
    xi = [0., 0., 2., 0., 0., 0.]
    prm = dict(scale=8, u0=0, v0=0, x_max=33, y_max=25)   # pixel (16, 12) is the principal point
    square = cr.generate_plane(PLANE_CAM, prm, xi, SQUARE)[0] > 0
    tri = cr.generate_plane(PLANE_CAM, prm, xi, SQUARE[:3])[0] > 0
    gon = [[math.cos(2 * math.pi * k / 16), math.sin(2 * math.pi * k / 16), 0.] for k in range(16)]
    disc = cr.generate_plane(PLANE_CAM, prm, xi, gon)[0] > 0
    assert tri[12, 16] and disc[12, 16] and 0 < tri.sum() < disc.sum() < square.sum()   # areas 2, 3.06 and 4
    assert (square | ~tri).all() and (square | ~disc).all()


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
    for name, value in (("QUERY_POINTS", 1), ("IMAGE_VALUES", 2), ("MINMAX", 4), ("ALL_HYPOTHESES", 8), ("DEFAULT_VALUES", 16),
                        ("SIGMA_VALUE", 32), ("QUERY_INDICES", 64), ("INDEX_MAPPING", 128)):
        assert getattr(capi, "RECON_" + name) == value == getattr(cr, name)
        assert re.search(r"#define VG_RECON_%s %du\b" % (name, value), header)
    assert os.path.exists(_build.STEREO_ACCURACY_CLI) and "stereo_accuracy" in _build.CLI_SOURCES


def test_arguments_are_checked_without_a_handle_or_a_device():
    from visgeom_amd import capi

    lib = capi.load()
    dp = ctypes.POINTER(ctypes.c_double)
    counts = (ctypes.c_int64 * 2)()
    fake = ctypes.c_void_p(4096)   # a DEVICE pointer is never read on the host
    xi = np.zeros((2, 6))

    def recon(h=None, n=1, hyp=1, flags=0, depth=fake, sigma=fake, poses=None):
        rc = lib.vg_depth_reconstruct(h, n, hyp, flags, depth, sigma, 0, None, None, poses.ctypes.data_as(dp) if poses is not None else None,
                                      counts, None)
        return rc, lib.vg_last_error().decode()

    for kw, text in ((dict(), "handle is NULL"), (dict(flags=capi.RECON_IMAGE_VALUES), "IMAGE_VALUES"), (dict(flags=256), "unknown"),
                     (dict(flags=1 << 31), "unknown"), (dict(hyp=0), "hyp_max"), (dict(hyp=9), "hyp_max"), (dict(n=-1), "item count"),
                     (dict(n=65536), "item count"), (dict(depth=None), "NULL"), (dict(flags=capi.RECON_SIGMA_VALUE, sigma=None), "sigma"),
                     (dict(flags=capi.RECON_MINMAX, sigma=None), "sigma")):
        rc, msg = recon(**kw)
        assert rc == capi.ERR_INVALID_ARGUMENT and text in msg, (kw, msg)
    for bad in (NAN, math.inf):
        xi[1, 4] = bad
        rc, msg = recon(n=2, poses=xi)
        assert rc == capi.ERR_INVALID_ARGUMENT and "finite" in msg
    out = capi.ReconOutputs(sigma_out=4096)
    assert lib.vg_depth_reconstruct(None, 1, 1, 0, fake, fake, 0, None, None, None, counts, ctypes.byref(out)) == capi.ERR_INVALID_ARGUMENT
    assert b"SIGMA_VALUE" in lib.vg_last_error()
    out = capi.ReconOutputs(index_map=4096)
    assert lib.vg_depth_reconstruct(None, 1, 1, capi.RECON_INDEX_MAPPING, fake, fake, 0, None, None, None, counts,
                                    ctypes.byref(out)) == capi.ERR_INVALID_ARGUMENT
    assert b"INDEX_MAPPING" in lib.vg_last_error()

    pose = np.array([0., 0., 2., 0., 0., 0.])
    for k, text in ((2, "3 to 16"), (17, "3 to 16"), (4, "handle is NULL")):
        poly = np.zeros((max(k, 3), 3))
        rc = lib.vg_depth_generate_plane(None, pose.ctypes.data_as(dp), k, poly.ctypes.data_as(dp), fake, fake, None)
        assert rc == capi.ERR_INVALID_ARGUMENT and text in lib.vg_last_error().decode()
    poly = np.array(SQUARE)
    poly[2, 1] = NAN
    assert lib.vg_depth_generate_plane(None, pose.ctypes.data_as(dp), 4, poly.ctypes.data_as(dp), fake, fake, None) == capi.ERR_INVALID_ARGUMENT
    assert b"finite" in lib.vg_last_error()
    assert lib.vg_depth_compare(None, 1, fake, fake, fake, 10., None, None, None) == capi.ERR_INVALID_ARGUMENT


def run_program(path):
    from visgeom_amd import _build

    return subprocess.run([_build.STEREO_ACCURACY_CLI, str(path)], capture_output=True, text=True, timeout=60)


def test_program_refuses_before_the_gpu_is_touched(tmp_path):
    from tests import stereo_accuracy_scene as sc

    def refused(text, **kw):
        with open(tmp_path / "sequence.json", "w") as f:
            json.dump(sc.sequence(**kw), f)
        res = run_program(tmp_path / "sequence.json")
        assert res.returncode == 1 and res.stderr.startswith("stereo_accuracy: ") and text in res.stderr, (kw, res.stderr)

    for key in ("trajectory", "camera_params", "stereo_parameters", "render", "noise", "sgm", "filter_noise"):
        refused("No such node (%s)" % key, **{key: None})
    for key in ("initial", "increment", "step_count"):
        tr = dict(sc.sequence()["trajectory"])
        tr.pop(key)
        refused("No such node (%s)" % key, trajectory=tr)
    refused("sgm: true or false expected", sgm=1)
    refused("filter_noise: true or false expected", filter_noise="yes")
    refused("noise must be in [0, 256]", noise=-1)
    refused("noise: an integer expected", noise=0.5)
    refused("cloud_step must be >= 0", cloud_step=-1)
    for count in (0, -3):
        refused("step_count must be in [1, 65535]", trajectory=dict(sc.sequence()["trajectory"], step_count=count))
    refused("cannot open", render="nowhere.json")
    sc.write(tmp_path)
    sp = dict(sc.sequence()["stereo_parameters"], uMax=sc.W - 2)
    refused("the world's image size differs from uMax x vMax", stereo_parameters=sp)
    assert run_program(tmp_path / "missing.json").returncode == 1
    assert subprocess.run([os.path.join(ROOT, "visgeom_amd", "bin", "stereo_accuracy")], capture_output=True, text=True).returncode == 2
