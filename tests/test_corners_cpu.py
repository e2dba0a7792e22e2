"""Corner detection without a GPU: the section 8 entries are declared, exported from both libraries and bound; they check
their arguments before touching HIP and refuse to compute on the host; the numpy restatement (tests/corners_ref.py) agrees
with hand-computed values; SubpixelCorner's gradient agrees with finite differences of its cost; the front end keeps its
error for an "images" entry with neither image files nor corners."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import corners_ref

ENTRIES = ("vg_corner_detector_create", "vg_corner_detector_destroy", "vg_corner_detect", "vg_corner_response",
           "vg_corner_candidates", "vg_corner_circle", "vg_corner_detector_stats", "vg_corner_detector_chunk")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from visgeom_amd import capi

    return capi.load()


def test_entries_declared_exported_and_bound(lib):
    from visgeom_amd import _build, capi

    header = open(os.path.join(ROOT, "include", "visgeom_amd.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.SIGNATURES, name
        assert getattr(lib, name).argtypes is not None or capi.SIGNATURES[name][1] == []
    prod = _build.PRODUCTION_LIB
    if not os.path.exists(prod):
        _build.build_production()
    out = subprocess.run(["nm", "-D", "--defined-only", prod], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, out, re.M), name


def test_create_checks_arguments_before_hip(lib):
    from visgeom_amd import capi

    h = ctypes.c_void_p()
    assert lib.vg_corner_detector_create(None, 0, None, 9, 7, 0) == capi.ERR_INVALID_ARGUMENT
    for cols, rows, improve in ((1, 7, 0), (9, 1, 0), (21, 20, 0), (9, 7, 2), (9, 7, -1)):
        assert lib.vg_corner_detector_create(ctypes.byref(h), 0, None, cols, rows, improve) == capi.ERR_INVALID_ARGUMENT
        assert not h.value
    # valid arguments: without a device the entry refuses (there is no host detector), with one it succeeds
    rc = lib.vg_corner_detector_create(ctypes.byref(h), 0, None, 9, 7, 0)
    if lib.vg_device_count() == 0:
        assert rc == capi.ERR_NO_DEVICE and not h.value
        assert b"no CPU fallback" in lib.vg_last_error()
    else:
        assert rc == capi.OK
        lib.vg_corner_detector_destroy(h)


def test_calls_check_arguments_before_hip(lib):
    from visgeom_amd import capi

    E = capi.ERR_INVALID_ARGUMENT
    buf = (ctypes.c_uint8 * 16)()
    d = np.zeros(16)
    dp = d.ctypes.data_as(capi._dp)
    assert lib.vg_corner_detect(None, 1, 64, 48, buf, dp, buf, None) == E
    i32 = np.zeros(4, np.int32)
    i64 = np.zeros(4, np.int64)
    assert lib.vg_corner_candidates(None, 1, 64, 48, buf, 1.4, 1, i32.ctypes.data_as(capi._i32p),
                                    i32.ctypes.data_as(capi._i32p), dp, i64.ctypes.data_as(capi._i64p)) == E
    assert lib.vg_corner_response(None, 1, 64, 48, buf, 1.4, buf, buf, buf, buf, buf, buf, dp) == E
    assert lib.vg_corner_detector_stats(None, dp) == E
    n = ctypes.c_int()
    assert lib.vg_corner_detector_chunk(None, 64, 48, ctypes.byref(n)) == E
    assert lib.vg_corner_circle(0, 8, i32.ctypes.data_as(capi._i32p), i32.ctypes.data_as(capi._i32p), ctypes.byref(n)) == E
    assert lib.vg_corner_circle(3, 8, None, None, ctypes.byref(n)) == E


def test_wrapper_refuses_host_tensors():
    import torch

    from visgeom_amd import corners

    with pytest.raises(ValueError, match="CUDA"):
        corners.detect_pattern(torch.zeros((48, 64), dtype=torch.uint8), 9, 7)
    with pytest.raises(ValueError, match="CUDA"):
        corners.detect_pattern(np.zeros((48, 64), np.uint8), 9, 7)


def test_gaussian_weights_by_hand():
    # getGaussianKernel(3, 0.7): exp(-1 / 0.98) at +-1, normalised
    e = math.exp(-0.5 / 0.49)
    assert np.array_equal(corners_ref.gaussian(3, 0.7), np.float32([e / (1 + 2 * e), 1 / (1 + 2 * e), e / (1 + 2 * e)]))
    w = corners_ref.gaussian(5, 2.0)
    a, b = math.exp(-1 / 8), math.exp(-4 / 8)
    s = 1 + 2 * a + 2 * b
    assert np.allclose(w, [b / s, a / s, 1 / s, a / s, b / s], rtol=0, atol=1e-7)
    assert w.dtype == np.float32 and abs(float(w.astype(np.float64).sum()) - 1) < 1e-6


def test_reflect101_border_by_hand():
    assert list(corners_ref.reflect101(np.arange(-3, 8), 5)) == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    # a single bright pixel in the corner: the 3-tap blur sees it twice through the reflected border at (0, 1) / (1, 0)
    img = np.zeros((6, 6), np.uint8)
    img[0, 0] = 200
    w = corners_ref.gaussian(3, 0.7).astype(np.float64)
    out = corners_ref.blur(img, 3, 0.7)
    assert out[0, 0] == round(200 * w[1] * w[1])
    assert out[0, 1] == round(200 * w[1] * w[2])
    assert out[1, 1] == round(200 * w[0] * w[0])


def test_response_by_hand():
    # a 2 x 2 checker: the strongest saddle response of the sigma_2 image lies next to its centre
    img = np.full((32, 32), 150, np.uint8)
    img[:16, :16] = 110
    img[16:, 16:] = 110
    m = corners_ref.response(img, 2.0)
    assert m["gradx"][0].sum() == 0 and m["grady"][:, -1].sum() == 0     # zero on the one-pixel border
    r = m["resp"]
    v, u = (int(x) for x in np.unravel_index(np.argmax(r), r.shape))
    assert r[v, u] > 0.01 and abs(v - 15.5) < 3 and abs(u - 15.5) < 3
    # one response by hand from the sigma_2 image
    s2 = m["src2"].astype(np.int64)
    iuu = s2[v, u - 1] + s2[v, u + 1] - 2 * s2[v, u]
    ivv = s2[v - 1, u] + s2[v + 1, u] - 2 * s2[v, u]
    iuv = (s2[v - 1, u - 1] + s2[v + 1, u + 1] - s2[v + 1, u - 1] - s2[v - 1, u + 1]) / 4
    gx, gy = int((s2[v, u + 1] - s2[v, u - 1]) / 2), int((s2[v + 1, u] - s2[v - 1, u]) / 2)
    assert r[v, u] == np.float32(-iuu * ivv + iuv * iuv - 0.001 * (gx * gx + gy * gy) ** 2)


# the reference's CurveRasterizer steps over one pixel twice on the radius-4 circle (a point of the loop, then its next point
# two rows away); restated as it is
GAPS = {4: [((-3, 3), (-4, 1)), ((3, -3), (4, -1))]}


@pytest.mark.parametrize("r", range(1, 9))
def test_circle_tables(r):
    c = corners_ref.circle(r)
    assert c[0] == (r, 0) and len(set(c)) == len(c)
    gaps = []
    for k in range(len(c)):   # a closed loop: the last point is next to the first
        (u0, v0), (u1, v1) = c[k], c[(k + 1) % len(c)]
        if max(abs(u1 - u0), abs(v1 - v0)) != 1:
            gaps.append((c[k], c[(k + 1) % len(c)]))
        assert abs(math.hypot(u0, v0) - r) <= 1.0, (r, c[k])
    assert gaps == GAPS.get(r, [])
    if r not in GAPS:   # 8-connected and symmetric under quarter turns
        s = set(c)
        assert all((-v, u) in s for u, v in c)


def test_circle_tables_match_the_library(lib):
    from visgeom_amd import corners

    for r in range(1, 9):
        assert [tuple(p) for p in corners.circle(r)] == corners_ref.circle(r)
    assert [len(corners_ref.circle(r)) for r in range(1, 6)] == [8, 12, 16, 22, 28]


def test_subpixel_gradient_matches_finite_differences():
    rng = np.random.default_rng(3)
    H, W = 40, 48
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    gu = (np.sin(xx / 5.) * np.cos(yy / 7.) + 0.05 * rng.standard_normal((H, W))).astype(np.float32)
    gv = (np.cos(xx / 6.) * np.sin(yy / 4.) + 0.05 * rng.standard_normal((H, W))).astype(np.float32)
    for x in ([20.3, 18.7, 0.4, 1.9, 0.3], [24.9, 21.2, -0.7, 0.8, -0.6], [10.1, 30.6, 2.5, -1.3, 0.0]):
        x = np.array(x)
        c0, g = corners_ref.subpixel_cost(gu, gv, (20., 19.), 5.6, x)
        for k in range(5):
            e = np.zeros(5)
            e[k] = 1e-6
            fd = (corners_ref.subpixel_cost(gu, gv, (20., 19.), 5.6, x + e)[0] -
                  corners_ref.subpixel_cost(gu, gv, (20., 19.), 5.6, x - e)[0]) / 2e-6
            assert abs(fd - g[k]) <= 1e-5 * max(1., abs(g[k])), (k, fd, g[k])


def test_bicubic_interpolates_and_clamps():
    g = np.arange(30, dtype=np.float32).reshape(5, 6)   # f = 6 r + c: linear, reproduced exactly inside
    f, dr, dc = corners_ref.bicubic(g, 2.25, 3.5)
    assert abs(f - (6 * 2.25 + 3.5)) < 1e-12 and abs(dr - 6) < 1e-12 and abs(dc - 1) < 1e-12
    f, dr, dc = corners_ref.bicubic(g, -3.0, 2.0)           # clamped rows: constant in r
    assert f == 2.0 and dr == 0.0


def test_frontend_still_refuses_images_without_files_or_corners(tmp_path):
    from visgeom_amd import synthetic as S
    from visgeom_amd.calibration import GenericCameraCalibration

    d = S.make_mono("eucm", 4, 0, sigma=0.0)
    path = S.write_calibration_json(str(tmp_path), d, "eucm", prior=False, init=True, as_images=True)
    root = json.load(open(path))
    del root["data"][0]["corners_file"]
    json.dump(root, open(path, "w"))
    c = GenericCameraCalibration()
    with pytest.raises(Exception, match="corner detector is out of scope"):
        c.addResiduals(path)
    c.close()
