"""Dense stereo without a GPU: the section 9 entries are declared, exported from both libraries and bound; vg_stereo_create
checks its arguments before touching HIP; the host curve walk equals the restatement (tests/stereo_ref.py) step for step;
hand values of compareDescriptor, fillGaps and regDiv; the curve table; the restatement recovers the range of a synthetic
sideways scene; the three rigs' images are what they were before the scene's world became arguments; every case on the strip
scene meets the conditions under which the GPU tests' comparison with it says something."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import stereo_ref as sr
from tests import stereo_scene
from tests import stereo_strip

ENTRIES = ("vg_stereo_params_default", "vg_stereo_create", "vg_stereo_destroy", "vg_stereo_size", "vg_stereo_chunk",
           "vg_stereo_compute", "vg_stereo_geometry", "vg_stereo_curve_cost", "vg_stereo_aggregate", "vg_stereo_curve_walk")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_PARAMS = dict(u_max=125, v_max=93, u0=15, v0=15, equal_margins=1, disp_max=32, error_max=150, flaw_cost=25, desc_length=5,
                    scales=[1, 2, 3, 5], desc_resp_thresh=2, use_uv_cache=0)
# what the restatement reaches on the sideways scene (96 x 64 depth pixels, disp_max 32): median relative range error 0.041,
# valid fraction 0.81
SIDEWAYS_MEDIAN_REL, SIDEWAYS_VALID = 0.06, 0.7


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
        assert getattr(lib, name).argtypes is not None
    prod = _build.PRODUCTION_LIB
    if not os.path.exists(prod):
        _build.build_production()
    out = subprocess.run(["nm", "-D", "--defined-only", prod], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, out, re.M), name


def test_params_default_is_the_reference(lib):
    from visgeom_amd import stereo

    p = stereo.default_params()
    assert (p.disp_max, p.error_max, p.epipole_margin, p.hypotheses, p.flaw_cost, p.desc_length, p.desc_resp_thresh) == \
        (48, 25, 2500, 1, 7, 5, 5)
    assert list(p.scales)[:p.n_scales] == [1, 2, 3, 5] and p.num_epipolar_planes == 2000
    assert (p.step_cost, p.jump_cost, p.image_based_cost, p.salient_points_only, p.use_uv_cache) == (5, 32, 1, 1, 1)


def _create(lib, p, c1=None, c2=None, xi=None):
    h = ctypes.c_void_p()
    arr = [np.ascontiguousarray(a, dtype=np.float64) for a in (c1 or stereo_scene.CAM1, c2 or stereo_scene.CAM2,
                                                               xi or stereo_scene.RIGS["sideways"])]
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.vg_stereo_create(ctypes.byref(h), 0, None, *[a.ctypes.data_as(dp) for a in arr], ctypes.byref(p))
    return rc, h


BAD = [dict(disp_max=3), dict(disp_max=258), dict(disp_max=2), dict(disp_max=33), dict(desc_length=4), dict(desc_length=33),
       dict(desc_length=1), dict(n_scales=0), dict(n_scales=9), dict(scales=[1, 17]), dict(scales=[0]), dict(hypotheses=2),
       dict(u_max=0), dict(v_max=20000), dict(u0=70, equal_margins=1), dict(x_max=0, equal_margins=0), dict(num_epipolar_planes=3),
       dict(num_epipolar_planes=0), dict(scale=0), dict(flaw_cost=-1), dict(jump_cost=20000), dict(epipole_margin=-1)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join("%s=%s" % kv for kv in b.items()) for b in BAD])
def test_create_rejects_bad_parameters_before_hip(lib, bad):
    from visgeom_amd import capi, stereo

    kw = dict(u_max=125, v_max=93, u0=15, v0=15, equal_margins=1, disp_max=32)
    kw.update(bad)
    p = stereo.make_params(**kw)
    rc, h = _create(lib, p)
    assert rc == capi.ERR_INVALID_ARGUMENT and not h.value, lib.vg_last_error()


def test_create_rejects_bad_cameras_before_hip(lib):
    from visgeom_amd import capi, stereo

    p = stereo.make_params(u_max=125, v_max=93, u0=15, v0=15, equal_margins=1, disp_max=32)
    assert _create(lib, p, xi=[0., 0., 0., 0.1, 0., 0.])[0] == capi.ERR_INVALID_ARGUMENT   # no baseline
    assert _create(lib, p, c1=[0.6, 1., 0., 60., 62., 46.])[0] == capi.ERR_INVALID_ARGUMENT   # fu = 0
    assert _create(lib, p, c2=[0.6, 1., math.nan, 60., 62., 46.])[0] == capi.ERR_INVALID_ARGUMENT
    h = ctypes.c_void_p()
    assert lib.vg_stereo_create(ctypes.byref(h), 0, None, None, None, None, ctypes.byref(p)) == capi.ERR_INVALID_ARGUMENT
    # valid arguments: without a device the entry refuses (there is no host stereo), with one it succeeds
    rc, h = _create(lib, p)
    if lib.vg_device_count() == 0:
        assert rc == capi.ERR_NO_DEVICE and not h.value
        assert b"no CPU fallback" in lib.vg_last_error()
    else:
        assert rc == capi.OK
        lib.vg_stereo_destroy(h)


def test_host_curve_walk_equals_restatement():
    from visgeom_amd import stereo

    prm = sr.params(**SCENE_PARAMS)
    G = sr.Geometry(stereo_scene.CAM1, stereo_scene.CAM2, stereo_scene.RIGS["forward"], prm)
    cases = [(sr.Poly2.circle(40, 30, 25), 65, 30, 0, 0, 1, 200), (sr.Poly2.circle(40, 30, 25), 65, 30, 0, 0, -3, -60),
             (sr.Poly2(0.001, 0.0002, -0.0005, 0.3, -0.2, 1.), 10, 12, 100, 80, 2, 150)]
    for cam in range(2):
        for idx in (0, 1, 500, 999, 1000, 1500, 2000):
            cases.append((G.table[cam][idx], 60, 45, G.ep_px[cam, 0][0], G.ep_px[cam, 0][1], 1, 120))
            cases.append((G.table[cam][idx], 60, 45, G.ep_px[cam, 1][0], G.ep_px[cam, 1][1], -2, -80))
    for poly, u, v, eu, ev, m, n in cases:
        host = stereo.curve_walk(poly.k, u, v, eu, ev, m, n)
        np.testing.assert_array_equal(host, sr.walk(poly, u, v, eu, ev, m, n))


def test_curve_walk_rejects_bad_arguments(lib):
    from visgeom_amd import capi

    dp = ctypes.POINTER(ctypes.c_double)
    p = np.zeros(6)
    out = np.zeros(4000, np.int32)
    ip = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.vg_stereo_curve_walk(p.ctypes.data_as(dp), 0, 0, 1, 1, 1, 1001, ip) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_stereo_curve_walk(p.ctypes.data_as(dp), 0, 0, 1, 1, 0, 10, ip) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_stereo_curve_walk(None, 0, 0, 1, 1, 1, 10, ip) == capi.ERR_INVALID_ARGUMENT


def test_circle_walk_is_8_connected_and_on_the_circle():
    c = sr.Poly2.circle(50, 40, 30)
    pts = sr.walk(c, 80, 40, 0, 0, 1, 300)
    d = np.abs(np.diff(pts, axis=0))
    assert d.max() <= 1 and (d.sum(axis=1) > 0).all()
    r = np.hypot(pts[:, 0] - 50, pts[:, 1] - 40)
    assert np.abs(r - 30).max() <= 1.


def test_compare_descriptor_hand_values():
    # a perfect match costs 0 at its own position; a flat descriptor against a step costs the step outside the band
    desc = [10, 50, 90, 50, 10]
    samples = [0, 0] + desc + [0, 0]
    c = sr.compare_descriptor(desc, samples, 7)
    assert c[4] == 0 and c.argmin() == 4
    c = sr.compare_descriptor([100, 100, 100], [100, 100, 100, 120, 120], 5)
    # thresholds all [100, 100]: rowC[j] = min path over 3 rows
    assert list(c) == [5, 0, 5, 40, 50]


def test_fill_gaps_hand_values():
    for step in range(1, 6):
        D = 12
        row = np.zeros(D, np.uint8)
        vals = [0, 60, 30, 90, 120, 200, 10, 250, 40, 70, 80, 90]
        n = (D + step - 1) // step
        for d in range(n):
            row[d * step] = vals[d]
        if step > 1:
            sr.fill_gaps(row, step, D)
        for d in range(1, n):
            a, b = vals[d - 1], vals[d]
            for i in range(1, step):
                assert row[d * step - i] == (a * i + b * (step - i)) // step
        assert (row[(n - 1) * step:] == vals[n - 1]).all()
    row = np.array([30, 0, 0, 90, 0, 0], np.uint8)   # step 3: (2 a + b) / 3, (a + 2 b) / 3
    sr.fill_gaps(row, 3, 6)
    assert list(row) == [30, 50, 70, 90, 90, 90]


def test_reg_div_branches():
    assert sr.reg_div(2., 4.) == 0.5
    assert sr.reg_div(0., -1.) == 2. / 1e-3
    assert sr.reg_div(1., 1e-4) == 2. / 1e-3 - 1e-4 / (1. * 1e-3 * 1e-3)


def test_curve_table_passes_through_epipoles_and_index_is_its_own_plane():
    prm = sr.params(**SCENE_PARAMS)
    for rig in stereo_scene.RIGS:
        G = sr.Geometry(stereo_scene.CAM1, stereo_scene.CAM2, stereo_scene.RIGS[rig], prm)
        for cam in range(2):
            e = G.ep[cam, 0 if G.ep_ok[cam, 0] else 1]
            for poly in G.table[cam][::50]:
                kuu, kuv, kvv, ku, kv, k1 = poly.k
                if kuu == kuv == kvv == 0:
                    continue   # a plane through the projection centre: a line, fixed by the centre instead
                val = (kuu * e[0] + kuv * e[1] + ku) * e[0] + (kvv * e[1] + kv) * e[1] + k1
                grad = math.hypot(2 * kuu * e[0] + kuv * e[1] + ku, kuv * e[0] + 2 * kvv * e[1] + kv)
                assert abs(val) <= 1e-6 * grad * max(1., math.hypot(*e)), (rig, cam, val, grad)
        n = G.n
        for idx in list(range(0, n, 97)) + [n // 2 - 1, n // 2 + 1, n - 1]:
            if idx < n // 2:
                d = [G.xb[i] + (G.pstep * idx - 1) * G.yb[i] for i in range(3)]
            else:
                d = [(G.pstep * (-idx + n // 2) + 1) * G.xb[i] + G.yb[i] for i in range(3)]
            assert G.index(d) % n == idx, (rig, idx)   # plane 0 is also entry n (the table repeats it)


def test_restatement_recovers_sideways_range():
    img1, img2, rng, xi = stereo_scene.make_scene("sideways")
    prm = sr.params(**SCENE_PARAMS)
    out = sr.stereo(stereo_scene.CAM1, stereo_scene.CAM2, xi, prm, img1, img2)
    d = out["depth"]
    m = (d > 0) & (rng > 0)
    assert m.mean() >= SIDEWAYS_VALID
    assert np.median(np.abs(d[m] - rng[m]) / rng[m]) <= SIDEWAYS_MEDIAN_REL



# SHA-256 of (img1, img2, true range) of make_scene(rig), recorded before planes, patch, texture band and cameras became
# arguments of cast, texture, render and make_scene
RIG_IMAGES = {
    "sideways": ("ec5cb2e603ec43f05e9861988f954178a4448037a96b28011852f22ac3983354",
                 "18b5e33ef53602f4a5cd08d990fe2355a07c492a0c82e503da20f8527d82d95f",
                 "d01efb4002978e5b0901898ad5e3237efe1470b4dd67c1cbb14066b7f16bebed"),
    "vertical": ("ec5cb2e603ec43f05e9861988f954178a4448037a96b28011852f22ac3983354",
                 "04db59b12361dfaafa938b5f92bff70d2e4240688ae03eaa12b1b515485f8901",
                 "d01efb4002978e5b0901898ad5e3237efe1470b4dd67c1cbb14066b7f16bebed"),
    "forward": ("ec5cb2e603ec43f05e9861988f954178a4448037a96b28011852f22ac3983354",
                "f38746258ee58cd899b6898c7d6a20d915015ef4839b496a6e735f7cd8482cdd",
                "d01efb4002978e5b0901898ad5e3237efe1470b4dd67c1cbb14066b7f16bebed"),
}


@pytest.mark.parametrize("rig", sorted(RIG_IMAGES))
def test_rig_images_are_unchanged(rig):
    import hashlib

    img1, img2, rng, xi = stereo_scene.make_scene(rig)
    assert img1.dtype == np.uint8 and img1.shape == (93, 125) and rng.dtype == np.float64 and rng.shape == (64, 96)
    assert (int(img1.sum()), int(img2.sum())) == {"sideways": (1491971, 1489317), "vertical": (1491971, 1489889),
                                                  "forward": (1491971, 1494707)}[rig]
    got = tuple(hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in (img1, img2, rng))
    assert got == RIG_IMAGES[rig]
    assert xi == stereo_scene.RIGS[rig]


@pytest.mark.parametrize("name", list(stereo_strip.CASES))
def test_strip_case_meets_its_conditions(name):
    """a scene change that empties a quarter of the disparity range, or a descriptor step, fails here before it reaches a GPU"""
    stereo_strip.check_conditions(name, stereo_strip.reference(name)[2])


def test_strip_batch_pairs_are_distinct_and_not_skipped():
    g = stereo_strip.S["grid"]
    win = (slice(g["v0"], g["v0"] + g["y_max"]), slice(g["u0"], g["u0"] + g["x_max"]))   # the depth grid in image 1
    pairs = [stereo_strip.images(*w)[:2] for w in stereo_strip.J_BATCH]
    for i in range(3):
        for j in range(i):
            assert (pairs[i][0][win] != pairs[j][0][win]).mean() > 0.5
    for w in stereo_strip.J_BATCH[1:]:
        ref = stereo_strip.reference("j", w)[2]
        assert ref["skip"].mean() <= 0.05 and (ref["disparity"] >= 0).mean() > 0.5
