"""Rectification (include/visgeom_amd.h section 7) without a GPU: the entries are declared, exported and bound, reject bad
arguments before touching HIP, refuse to compute on the host; the `rectify` program rejects malformed input; the numpy
restatement the GPU tests compare against agrees with hand-computed values."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import rectify_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vg_rectify_map", "vg_remap")


@pytest.fixture(scope="module")
def lib():
    from visgeom_amd import _build, capi

    _build.build()
    return capi.load()


def _no_gpu():
    import torch

    return not torch.cuda.is_available()


def test_entries_declared_exported_and_bound(lib):
    from visgeom_amd import _build, capi

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "visgeom_amd.h")).read(), flags=re.S)
    assert "VG_PIXEL_U8 = 0" in text and "VG_PIXEL_F32 = 1" in text
    libs = [_build.LIB] + ([_build.PRODUCTION_LIB] if os.path.exists(_build.PRODUCTION_LIB) else [])
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in capi.SIGNATURES
        assert getattr(lib, name).restype is ctypes.c_int
        for so in libs:
            out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
            assert re.search(r" T %s$" % name, out, flags=re.M), (name, so)
    assert lib.vg_abi_version() == 1


def _map_call(lib, model=0, intr="default", pinhole="default", xi="default", mx=1, my=1):
    """vg_rectify_map with host arrays for the parameters (None = a NULL pointer) and raw addresses for the maps"""
    dp = ctypes.POINTER(ctypes.c_double)
    vals = {"intr": [0.6, 1.1, 300., 300., 320., 240.], "pinhole": [64., 48., 32., 24., 40.], "xi": np.zeros(6)}
    given = {"intr": intr, "pinhole": pinhole, "xi": xi}
    keep = {k: None if given[k] is None else np.ascontiguousarray(vals[k] if isinstance(given[k], str) else given[k], np.float64)
            for k in vals}
    ptr = {k: None if v is None else v.ctypes.data_as(dp) for k, v in keep.items()}
    return lib.vg_rectify_map(0, None, model, ptr["intr"], ptr["pinhole"], ptr["xi"], ctypes.c_void_p(mx), ctypes.c_void_p(my))


def test_rectify_map_argument_checks(lib):
    from visgeom_amd import capi

    bad = capi.ERR_INVALID_ARGUMENT
    assert _map_call(lib, model=3) == bad
    assert _map_call(lib, model=-1) == bad
    assert _map_call(lib, intr=None) == bad
    assert _map_call(lib, pinhole=None) == bad
    assert _map_call(lib, xi=None) == bad
    assert _map_call(lib, mx=0) == bad
    assert _map_call(lib, my=0) == bad
    for ph in ([0., 48., 32., 24., 40.], [64.5, 48., 32., 24., 40.], [64., 16385., 32., 24., 40.], [64., 48., 32., 24., 0.],
               [64., 48., np.nan, 24., 40.], [np.nan, 48., 32., 24., 40.]):
        assert _map_call(lib, pinhole=np.array(ph)) == bad, ph
    assert b"pinhole" in lib.vg_last_error()


def _remap_call(lib, ptype=0, ch=1, n=2, sw=16, sh=8, src=1, mw=12, mh=4, mx=1, my=1, dst=1):
    return lib.vg_remap(0, None, ptype, ch, n, sw, sh, ctypes.c_void_p(src), mw, mh, ctypes.c_void_p(mx), ctypes.c_void_p(my),
                        0., ctypes.c_void_p(dst))


def test_remap_argument_checks(lib):
    from visgeom_amd import capi

    bad = capi.ERR_INVALID_ARGUMENT
    for kw in ({"ptype": 2}, {"ptype": -1}, {"ch": 2}, {"ch": 0}, {"ch": 5}, {"n": -1}, {"sw": 0}, {"sh": -3}, {"mw": 0},
               {"mh": 16385}, {"sw": 16385}, {"src": 0}, {"dst": 0}, {"mx": 0}, {"my": 0}):
        assert _remap_call(lib, **kw) == bad, kw


def test_no_cpu_fallback(lib):
    """valid arguments without a device: VG_ERR_NO_DEVICE, never a host result (the buffers are host memory and stay as
    they were)"""
    from visgeom_amd import capi

    if not _no_gpu():
        pytest.skip("a GPU is present; the no-device path cannot be exercised")
    mx, my = np.full(64 * 48, 7., np.float32), np.full(64 * 48, 7., np.float32)
    rc = _map_call(lib, mx=mx.ctypes.data, my=my.ctypes.data)
    assert rc == capi.ERR_NO_DEVICE and b"no CPU fallback" in lib.vg_last_error()
    assert (mx == 7.).all() and (my == 7.).all()
    src, dst = np.zeros((2, 8, 16), np.uint8), np.full((2, 4, 12), 9, np.uint8)
    m = np.zeros(48, np.float32)
    rc = _remap_call(lib, src=src.ctypes.data, mx=m.ctypes.data, my=m.ctypes.data, dst=dst.ctypes.data)
    assert rc == capi.ERR_NO_DEVICE
    assert (dst == 9).all()
    from visgeom_amd import rectify

    with pytest.raises((capi.VisgeomError, RuntimeError, AssertionError)):
        rectify.rectify_maps("eucm", [0.6, 1.1, 300., 300., 320., 240.], [64, 48, 32, 24, 40], np.zeros(6))


# ---------------------------------------------------------------------------------------------------------- the CLI
def _run_cli(tmp_path, cfg, files=None):
    from visgeom_amd import _build

    _build.build()
    for name, data in (files or {}).items():
        (tmp_path / name).write_bytes(data)
    path = tmp_path / "r.json"
    path.write_text(cfg if isinstance(cfg, str) else json.dumps(cfg))
    return subprocess.run(["timeout", "-k", "5", "60", _build.RECTIFY_CLI, str(path)], cwd=str(tmp_path), capture_output=True,
                          text=True)


def _pgm(w, h, body=None, maxval=255):
    return b"P5\n%d %d\n%d\n" % (w, h, maxval) + (body if body is not None else bytes(w * h))


GOOD = {"camera_params": [0.6, 1.1, 300., 300., 320., 240.], "pinhole_params": [64, 48, 32, 24, 40],
        "xi_eucm_pinhole": [0, 0, 0, 0, 0, 0], "image_names": ["a.pgm"]}


@pytest.mark.parametrize("cfg", [
    "{ not json",
    {k: v for k, v in GOOD.items() if k != "camera_params"},
    {k: v for k, v in GOOD.items() if k != "image_names"},
    dict(GOOD, camera_params=[0.6, 1.1, 300.]),
    dict(GOOD, camera_model="kannala"),
    dict(GOOD, camera_model="ucm"),                  # six values for a five-parameter model
    dict(GOOD, pinhole_params=[64, 48, 32, 24]),
    dict(GOOD, pinhole_params=[64.5, 48, 32, 24, 40]),
    dict(GOOD, xi_eucm_pinhole=[1, 2, 3, 4]),
    dict(GOOD, image_names=["missing.pgm"]),
])
def test_cli_rejects_malformed_json(tmp_path, cfg):
    r = _run_cli(tmp_path, cfg, {"a.pgm": _pgm(8, 6)})
    assert r.returncode not in (0, 124, 137) and r.returncode > 0, (r.returncode, r.stderr)
    assert r.stderr.startswith("rectify:") and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert not list(tmp_path.glob("img_*.pgm"))


@pytest.mark.parametrize("data", [
    b"P2\n8 6\n255\n" + bytes(48),           # ASCII PGM
    b"P6\n8 6\n255\n" + bytes(144),          # PPM
    _pgm(8, 6, bytes(47)),                   # truncated
    _pgm(8, 6, maxval=65535) + bytes(48),    # 16-bit
    b"P5\n8\n",                              # header cut short
    b"P5\n0 6\n255\n",                       # empty image
    b"P5 8 6 255",                           # no data
    b"",
])
def test_cli_rejects_malformed_pgm(tmp_path, data):
    r = _run_cli(tmp_path, GOOD, {"a.pgm": data})
    assert r.returncode not in (0, 124, 137) and r.returncode > 0, (r.returncode, r.stderr)
    assert r.stderr.startswith("rectify:") and len(r.stderr.strip().splitlines()) == 1, r.stderr


def test_cli_usage():
    from visgeom_amd import _build

    _build.build()
    r = subprocess.run(["timeout", "-k", "5", "60", _build.RECTIFY_CLI], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


# ------------------------------------------------------------------------------------------ the numpy restatement
def test_remap_restatement_hand_values():
    img = np.array([[10, 20, 30], [40, 50, 60]], np.uint8)[None, :, :, None]      # W = 3, H = 2
    cases = [  # (mx, my, fill, expected)
        (0., 0., 0., 10),            # exact integer coordinates: the pixel itself
        (2., 1., 0., 60),
        (1., 0., 7., 20),
        (0.5, 0., 0., 15),           # horizontal midpoint
        (0.5, 0.5, 0., 30),          # (10 + 20 + 40 + 50) / 4
        (0.25, 0., 0., 12),          # 12.5 -> 12 (ties to even)
        (0.75, 0., 0., 18),          # 17.5 -> 18
        (2.5, 0., 100., 65),         # right tap outside: 0.5 * 30 + 0.5 * 100
        (-0.5, 0., 100., 55),        # left tap outside: 0.5 * 100 + 0.5 * 10
        (0., -0.5, 0., 5),           # upper taps outside, fill 0: 0.5 * 10 = 5
        (2., 1.5, 255., 158),        # lower taps outside: 0.5 * 60 + 0.5 * 255 = 157.5 -> 158
        (-1., -1., 9., 9),           # (-1, -1): the failed-projection marker is pure fill
        (-1., 0., 9., 9),            # the border of the open interval is outside
        (3., 0., 9., 9),
        (0., 2., 9., 9),
        (np.nan, 0., 9., 9),
        (0., np.nan, 9., 9),
        (1e30, 0., 9., 9),
        (-1e30, 1e30, 9., 9),
        (0., 0., 300., 10),
    ]
    for mx, my, fill, want in cases:
        got = rectify_ref.remap(img, np.array([mx], np.float32), np.array([my], np.float32), fill)
        assert got.shape == (1, 1, 1) and got[0, 0, 0] == want, (mx, my, fill, got)
    # u8 saturation of the fill itself, and float32 output without rounding
    assert rectify_ref.remap(img, np.float32([-1]), np.float32([-1]), 300.)[0, 0, 0] == 255
    assert rectify_ref.remap(img, np.float32([-1]), np.float32([-1]), -4.)[0, 0, 0] == 0
    f = img.astype(np.float32)
    assert rectify_ref.remap(f, np.float32([0.25]), np.float32([0.]), 0.)[0, 0, 0] == np.float32(12.5)
    assert rectify_ref.remap(f, np.float32([-1]), np.float32([-1]), 0.5)[0, 0, 0] == np.float32(0.5)
    # channels are interpolated independently
    rgb = np.stack([img[..., 0], 2 * img[..., 0], 3 * img[..., 0]], -1).astype(np.float32)
    out = rectify_ref.remap(rgb, np.float32([0.5]), np.float32([0.5]), 0.)
    assert np.array_equal(out[0, 0], np.float32([30, 60, 90]))


def test_map_restatement_identity_camera():
    """an EUCM with alpha = 0 is a pinhole: with the same focal length and centre the map is the pixel grid"""
    pin = [16, 12, 7.5, 5.5, 20.]
    mx, my = rectify_ref.rectify_maps(0, [0., 1., 20., 20., 7.5, 5.5], pin, np.eye(3), np.zeros(3))
    j, i = np.meshgrid(np.arange(16), np.arange(12))
    assert np.allclose(mx, j, atol=1e-5) and np.allclose(my, i, atol=1e-5)
    # a point behind the camera fails: the whole map is (-1, -1)
    mx, my = rectify_ref.rectify_maps(0, [0.6, 1., 20., 20., 7.5, 5.5], pin, np.diag([1., 1., -1.]), np.zeros(3))
    assert (mx == -1).all() and (my == -1).all()
