"""Conversion between camera models without a GPU (include/visgeom_amd.h section 20): the numpy reference of the unprojection
(tests/convert_ref.py) against a 50-digit evaluation of the definitions, the header visgeom_amd/csrc/vg_unproject.hpp as a host
program under the address and undefined-behaviour sanitizers against that reference, the default start of the fit, and the refusals
every entry makes before HIP is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import convert_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1280, 800
MODELS = ["eucm", "ucm", "mei", "kb", "ds"]
FOLDED_KB = np.array([-0.4, 0, 0, 0, 380.0, 375.0, 640.0, 400.0])   # d' = 1 - 1.2 theta^2: folds at theta = 0.913, d = 0.609


@pytest.fixture(scope="module")
def S():
    from visgeom_amd import synthetic

    return synthetic


@pytest.fixture(scope="module")
def L():
    from visgeom_amd import capi

    return capi.load()


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def image_pixels(n, seed):
    """the principal point's neighbourhood, the image corners and random pixels of the 1280 x 800 image"""
    rng = np.random.default_rng(seed)
    fixed = [[642.617, 398.42], [0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [640.25, 399.75]]
    return np.concatenate([fixed, np.column_stack([rng.uniform(0, W - 1, n - len(fixed)), rng.uniform(0, H - 1, n - len(fixed))])])


# ------------------------------------------------------------------------------------------ numpy against 50 digits
@pytest.mark.parametrize("model", ["mei", "ucm", "eucm"])
def test_numpy_unprojection_against_mpmath(S, model):
    """Mei with GT_MEI's distortion (the Newton inverse), UCM and EUCM: unit rays to 1e-12, and the same pixels valid"""
    p = S.GT[model]
    if model == "mei":
        assert np.all(p[1:6] != 0)
    uv = image_pixels(60, 3)
    X, ok = ref.unproject_unit(model, p, uv)
    worst, n_valid = 0.0, 0
    for i in range(len(uv)):
        want = ref.mp_unproject(model, p, uv[i])
        assert (want is not None) == bool(ok[i]), (model, uv[i])
        if want is None:
            continue
        n_valid += 1
        worst = max(worst, max(abs(float(ref.mpf(float(X[i, k])) - want[k])) for k in range(3)))
    print(model, "valid", n_valid, "of", len(uv), "worst |ray - mpmath| = %.3e" % worst)
    assert n_valid >= len(uv) // 2
    assert worst <= 1e-12


def test_numpy_mei_round_trip_and_the_reference_form(S):
    """the undistorted Mei ray projects back onto its pixel, and Mei with zero distortion is UCM bit for bit"""
    p = S.GT["mei"]
    uv = image_pixels(200, 4)
    X, ok = ref.unproject_unit("mei", p, uv)
    back, okp = ref.project("mei", p, X[ok])
    assert okp.all()
    err = np.max(np.abs(back - uv[ok]))
    print("mei round trip %.3e px over %d pixels" % (err, int(ok.sum())))
    assert err <= 1e-9
    p0 = np.concatenate([p[:1], np.zeros(5), p[6:]])
    X0, ok0 = ref.unproject("mei", p0, uv)
    Xu, oku = ref.unproject("ucm", S.GT["ucm"], uv)
    assert np.array_equal(ok0, oku) and np.array_equal(X0, Xu)


def test_ucm_domain_is_a_failure_not_a_nan(S):
    """1 + u2 (1 - xi^2) < 0 fails here (the reference returns true and a NaN ray); with GT_UCM that is part of the image"""
    j, i = np.meshgrid(np.arange(0, W, 8.0), np.arange(0, H, 8.0))
    uv = np.stack([j.ravel(), i.ravel()], -1)
    X, ok = ref.unproject_unit("ucm", S.GT["ucm"], uv)
    frac = 1.0 - ok.mean()
    print("GT_UCM: %.1f %% of the image outside the domain" % (100 * frac))
    assert 0.005 < frac < 0.1
    assert np.all(X[~ok] == 0) and np.isfinite(X).all()
    assert np.all(ref.domain_margin("ucm", S.GT["ucm"], uv[~ok]) < 0) and np.all(ref.domain_margin("ucm", S.GT["ucm"], uv[ok]) >= 0)


# ------------------------------------------------------------------------------------------ the header as a host program
def check_cases(S):
    """(model, intrinsics, pixels): the principal point, pixels outside every model's domain, NaN and infinite pixels, the image's
    corners, random pixels; and a folded Kannala-Brandt polynomial"""
    far = [[1e5, 1e5], [-3e4, 7e4], [6e3, 400.0], [640.0, -5e3]]
    odd = [[np.nan, 10.0], [10.0, np.nan], [np.inf, 5.0], [3.0, -np.inf], [np.nan, np.nan]]
    cases = []
    for m in MODELS:
        p = np.array(S.GT[m], float)
        uv = np.concatenate([[p[-2:]], far, odd, image_pixels(40, 11)])
        cases.append((m, p, uv))
    p0 = np.concatenate([S.GT["mei"][:1], np.zeros(5), S.GT["mei"][6:]])
    cases.append(("mei", p0, np.concatenate([[p0[-2:]], far, image_pixels(20, 12)])))
    cases.append(("kb", FOLDED_KB, np.concatenate([[FOLDED_KB[-2:]], far, odd, image_pixels(40, 13)])))
    for m, p, seed in (("eucm", [0.3, 2.0, 300.0, 310.0, 640.0, 400.0], 14), ("ds", [0.1, 0.4, 300.0, 310.0, 640.0, 400.0], 15)):
        cases.append((m, np.array(p), np.concatenate([[p[-2:]], image_pixels(20, seed)])))   # alpha < 0.5: no boundary
    return cases


@pytest.fixture(scope="module")
def host_rows(S, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unproject") / "unproject_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "visgeom_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "unproject_check.cpp"), "-o", exe])
    cases = check_cases(S)
    text = "".join("%d %s %d %s\n" % (ref.MODEL_ID[m], " ".join(repr(float(v)) for v in p), len(uv),
                                     " ".join(repr(float(v)) for v in uv.ravel())) for m, p, uv in cases)
    r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    rows = np.array([[float(t) for t in ln.split()] for ln in r.stdout.decode().splitlines()])
    assert rows.shape == (sum(len(uv) for _, _, uv in cases), 8)
    out, at = [], 0
    for m, p, uv in cases:
        out.append((m, p, uv, rows[at:at + len(uv)]))
        at += len(uv)
    return out


def test_header_under_sanitizers_against_numpy(host_rows):
    """rays to 1e-12, ok flags equal: raw and unit rays of every case"""
    n_failed = 0
    for m, p, uv, rows in host_rows:
        X, ok = ref.unproject(m, p, uv)
        U, oku = ref.unproject_unit(m, p, uv)
        assert np.array_equal(rows[:, 0] != 0, ok), (m, p)
        assert np.array_equal(rows[:, 4] != 0, oku), (m, p)
        scale = np.maximum(1.0, np.abs(X).max(-1, keepdims=True))
        worst = max(np.max(np.abs(rows[:, 1:4] - X) / scale), np.max(np.abs(rows[:, 5:8] - U)))
        print(m, "valid %d of %d, worst %.3e" % (int(ok.sum()), len(uv), worst))
        assert worst <= 1e-12
        assert np.all(rows[~oku, 5:8] == 0)
        n_failed += int((~ok).sum())
    assert n_failed >= 30


def test_header_special_pixels(host_rows, S):
    for m, p, uv, rows in host_rows:
        assert rows[0, 4] == 1 and np.array_equal(rows[0, 5:8], [0, 0, 1]), (m, "the principal point looks along the axis")
        bad = ~np.isfinite(uv).all(-1)
        assert np.all(rows[bad, 0] == 0) and np.all(rows[bad, 4] == 0), (m, "a NaN or infinite pixel fails")
        if np.array_equal(p, S.GT[m]):   # the four far pixels are outside every model's domain
            assert np.all(rows[1:5, 0] == 0), (m, rows[1:5, 0])
    m, p, uv, rows = [c for c in host_rows if c[1] is FOLDED_KB or np.array_equal(c[1], FOLDED_KB)][0]
    rd = np.hypot((uv[:, 0] - p[6]) / p[4], (uv[:, 1] - p[7]) / p[5])
    beyond = np.isfinite(rd) & (rd > 0.6086)   # d(theta) peaks at 0.60858 where d' = 0
    inside = np.isfinite(rd) & (rd < 0.60)
    assert beyond.sum() > 10 and inside.sum() > 3
    assert np.all(rows[beyond, 0] == 0) and np.all(rows[inside, 0] == 1)


# ------------------------------------------------------------------------------------------ the default start
def test_default_start_table(L, S):
    from visgeom_amd import capi

    for src in MODELS:
        p = np.ascontiguousarray(S.GT[src], dtype=np.float64)
        f0 = p[-4:-2] / (1 + p[0]) if src in ("ucm", "mei", "ds") else p[-4:-2]
        c = p[-2:]
        table = {"eucm": [0.5, 1, *f0, *c], "ucm": [1, *(2 * f0), *c], "mei": [1, 0, 0, 0, 0, 0, *(2 * f0), *c],
                 "kb": [0, 0, 0, 0, *f0, *c], "ds": [0, 0.5, *f0, *c]}
        for dst in MODELS:
            out = np.full(ref.K_OF[dst], np.nan)
            assert L.vg_convert_start(capi.MODELS[src], _dp(p), capi.MODELS[dst], _dp(out)) == capi.OK
            assert np.array_equal(out, np.array(table[dst], float)), (src, dst, out)
            assert np.array_equal(out, ref.default_start(src, p, dst))
    out = np.zeros(10)
    for bad in (3, -1, 6):
        assert L.vg_convert_start(bad, _dp(p), 0, _dp(out)) == capi.ERR_INVALID_ARGUMENT
        assert L.vg_convert_start(0, _dp(p), bad, _dp(out)) == capi.ERR_INVALID_ARGUMENT
    assert L.vg_convert_start(0, None, 0, _dp(out)) == capi.ERR_INVALID_ARGUMENT


def test_default_start_sees_the_source_rays(S):
    """the default starts project every ray but the one pointing exactly backwards: here, every kept sample of the five cameras"""
    for src in MODELS:
        rays, uv, _ = ref.fit_samples(src, S.GT[src], (W, H), (16, 10))
        for dst in MODELS:
            _, ok = ref.project(dst, ref.default_start(src, S.GT[src], dst), rays)
            assert ok.all(), (src, dst)


def test_fit_default_options(L):
    from visgeom_amd import capi

    o = capi.ConvertFitOptions()
    L.vg_convert_fit_default_options(ctypes.byref(o))
    assert (o.grid_w, o.grid_h, o.max_iterations, o.use_bounds) == (64, 40, 100, 1)
    assert o.max_angle == np.pi
    assert (o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance) == (1e-6, 1e-10, 1e-8)


# ------------------------------------------------------------------------------------------ refusals before HIP is touched
def test_refusals_come_before_the_device(L, S):
    """device -1 names no HIP device: an entry that reached the device check would answer VG_ERR_NO_DEVICE or complain about the
    index; every call below is refused for its own argument first"""
    from visgeom_amd import capi

    eucm, kb = np.ascontiguousarray(S.GT["eucm"]), np.ascontiguousarray(S.GT["kb"])
    x = np.full(10, np.nan)
    buf = ctypes.c_void_p(256)   # never dereferenced: the calls are refused first
    opt = capi.ConvertFitOptions()

    def options(**kw):
        L.vg_convert_fit_default_options(ctypes.byref(opt))
        for k, v in kw.items():
            setattr(opt, k, v)
        return ctypes.byref(opt)

    def refused(rc, word):
        assert rc == capi.ERR_INVALID_ARGUMENT, (rc, L.vg_last_error())
        assert word.encode() in L.vg_last_error(), L.vg_last_error()

    for bad in (3, -1, 6, 7):
        refused(L.vg_unproject(-1, None, bad, _dp(eucm), 4, buf, buf, buf), "unknown camera model")
        refused(L.vg_convert_map(-1, None, bad, _dp(eucm), 0, _dp(eucm), None, 64, 64, buf, buf), "model")
        refused(L.vg_convert_map(-1, None, 0, _dp(eucm), bad, _dp(eucm), None, 64, 64, buf, buf), "model")
        refused(L.vg_convert_fit(-1, None, bad, _dp(kb), W, H, 0, _dp(x), None, None), "model")
        refused(L.vg_convert_fit(-1, None, 4, _dp(kb), W, H, bad, _dp(x), None, None), "model")
    for side in (0, 16385, -1):
        refused(L.vg_convert_map(-1, None, 0, _dp(eucm), 4, _dp(kb), None, side, 64, buf, buf), "16384")
        refused(L.vg_convert_map(-1, None, 0, _dp(eucm), 4, _dp(kb), None, 64, side, buf, buf), "16384")
        refused(L.vg_convert_fit(-1, None, 4, _dp(kb), side, H, 0, _dp(x), None, None), "16384")
        refused(L.vg_convert_fit(-1, None, 4, _dp(kb), W, side, 0, _dp(x), None, None), "16384")
    refused(L.vg_convert_fit(-1, None, 4, _dp(kb), W, H, 0, _dp(x), options(grid_w=1025, grid_h=1024), None), "2^20")
    refused(L.vg_convert_fit(-1, None, 4, _dp(kb), W, H, 0, _dp(x), options(grid_w=2 ** 20 + 1, grid_h=1), None), "2^20")
    refused(L.vg_convert_fit(-1, None, 4, _dp(kb), W, H, 0, _dp(x), options(grid_w=65536, grid_h=65536), None), "2^20")
    refused(L.vg_convert_fit(-1, None, 4, _dp(kb), W, H, 0, _dp(x), options(grid_w=0), None), "2^20")
    refused(L.vg_convert_fit(-1, None, 4, _dp(kb), W, H, 0, _dp(x), options(max_angle=0.0), None), "max_angle")
    refused(L.vg_convert_fit(-1, None, 4, _dp(kb), W, H, 0, _dp(x), options(max_angle=float("nan")), None), "max_angle")
    refused(L.vg_convert_fit(-1, None, 4, _dp(kb), W, H, 0, _dp(x), options(max_iterations=-1), None), "max_iterations")
    refused(L.vg_convert_fit(-1, None, 4, _dp(kb), W, H, 0, _dp(x), options(gradient_tolerance=-1e-3), None), "tolerances")
    refused(L.vg_unproject(-1, None, 0, _dp(eucm), -1, buf, buf, buf), "2^31")
    refused(L.vg_unproject(-1, None, 0, _dp(eucm), 2 ** 31, buf, buf, buf), "2^31")
    refused(L.vg_unproject(-1, None, 0, None, 4, buf, buf, buf), "NULL")
    refused(L.vg_unproject(-1, None, 0, _dp(eucm), 4, None, buf, buf), "NULL")
    refused(L.vg_convert_map(-1, None, 0, _dp(eucm), 4, _dp(kb), None, 64, 64, None, buf), "NULL")
    refused(L.vg_convert_map(-1, None, 0, _dp(eucm), 4, _dp(kb), _dp(np.array([0.0, np.inf, 0.0])), 64, 64, buf, buf), "rotation")
    refused(L.vg_convert_fit(-1, None, 4, None, W, H, 0, _dp(x), None, None), "NULL")
    assert np.isnan(x).all()   # nothing was written
    # a valid call does reach the device check
    rc = L.vg_convert_map(-1, None, 0, _dp(eucm), 4, _dp(kb), None, 64, 64, buf, buf)
    assert rc in (capi.ERR_NO_DEVICE, capi.ERR_INVALID_ARGUMENT) and b"unknown camera model" not in L.vg_last_error() and b"16384" not in L.vg_last_error()


def test_python_wrappers_check_their_arguments(S):
    from visgeom_amd import convert

    with pytest.raises(KeyError):   # the name table of rectify.py
        convert.convert_maps("eucm", S.GT["eucm"], "pinhole", S.GT["kb"], (64, 64))
    with pytest.raises(ValueError):
        convert.convert_maps("eucm", S.GT["eucm"], 3, S.GT["kb"], (64, 64))
    with pytest.raises(ValueError):
        convert.convert_maps("eucm", S.GT["kb"], "kb", S.GT["kb"], (64, 64))
    with pytest.raises(ValueError):
        convert.convert_maps("eucm", S.GT["eucm"], "kb", S.GT["kb"], (0, 64))
    with pytest.raises(ValueError):
        convert.default_start("kb", S.GT["eucm"], "eucm")
    assert np.array_equal(convert.default_start("kb", S.GT["kb"], "eucm"), ref.default_start("kb", S.GT["kb"], "eucm"))
