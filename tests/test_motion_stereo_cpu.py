"""Motion stereo without a GPU: the section 10 entries are declared, exported from both libraries and bound; the defaults are
the reference's; vg_motion_stereo_create checks its arguments before touching HIP; hand values of the temporal filter, the
mask, the too-certain rule and the 2 x cost acceptance rule; the restatement (tests/motion_ref.py) recovers the range of the
synthetic rigs; the `motion_stereo` program rejects malformed input with one line on stderr before any GPU work."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import motion_ref as mr
from tests import motion_scene as ms
from tests import stereo_scene

ENTRIES = ("vg_motion_stereo_params_default", "vg_motion_stereo_create", "vg_motion_stereo_destroy", "vg_motion_stereo_size",
           "vg_motion_stereo_set_base", "vg_motion_stereo_compute", "vg_motion_stereo_mask", "vg_motion_stereo_select")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the restatement's own figures: the comment next to TRUTH_NO_PRIOR in tests/test_gpu_motion_stereo.py; the same bars
TRUTH_NO_PRIOR = {"sideways": (0.0852, 0.690), "vertical": (0.0794, 0.608), "forward": (0.1065, 0.239)}


@pytest.fixture(scope="module")
def lib():
    from visgeom_amd import capi

    return capi.load()


def test_entries_declared_exported_and_bound(lib):
    from visgeom_amd import _build, capi

    header = open(os.path.join(ROOT, "include", "visgeom_amd.h")).read()
    assert re.search(r"#define VG_ABI_VERSION 1\b", header) and lib.vg_abi_version() == 1
    libs = [_build.LIB, _build.PRODUCTION_LIB]
    if not os.path.exists(libs[1]):
        _build.build_production()
    for path in libs:
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in ENTRIES:
            assert re.search(r" T %s$" % name, out, re.M), (path, name)
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.SIGNATURES, name
        assert getattr(lib, name).argtypes is not None


def test_defaults_are_the_reference(lib):
    from visgeom_amd import motion_stereo, stereo

    p = motion_stereo.default_params()
    assert p.gradient_thresh == 2
    d = stereo.default_params()
    assert bytes(p.stereo) == bytes(d)
    sp = json.load(open(os.path.join(ROOT, "tests", "golden", "ex_epipolar_stereo.json")))["stereo_parameters"]
    q = motion_stereo.params_from_json(sp)
    assert q.gradient_thresh == int(sp["motion_stereo_parameters"]["gradient_thresh"])
    assert bytes(q.stereo) == bytes(stereo.params_from_json(sp))
    assert motion_stereo.params_from_json(dict(sp, motion_stereo_parameters={"gradient_thresh": 9})).gradient_thresh == 9


def _create(lib, p, c1=None, c2=None):
    h = ctypes.c_void_p()
    arr = [np.ascontiguousarray(a, dtype=np.float64) for a in (c1 or stereo_scene.CAM1, c2 or stereo_scene.CAM2)]
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.vg_motion_stereo_create(ctypes.byref(h), 0, None, *[a.ctypes.data_as(dp) for a in arr], ctypes.byref(p))
    return rc, h


BAD = [dict(disp_max=3), dict(disp_max=258), dict(desc_length=4), dict(desc_length=33), dict(scales=[1, 17]), dict(hypotheses=2),
       dict(u_max=0), dict(u0=70, equal_margins=1), dict(num_epipolar_planes=3), dict(scale=0), dict(flaw_cost=-1),
       dict(gradient_thresh=-1), dict(gradient_thresh=256)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join("%s=%s" % kv for kv in b.items()) for b in BAD])
def test_create_rejects_bad_parameters_before_hip(lib, bad):
    from visgeom_amd import capi, motion_stereo

    kw = dict(u_max=125, v_max=93, u0=15, v0=15, equal_margins=1, disp_max=32)
    kw.update(bad)
    rc, h = _create(lib, motion_stereo.make_params(**kw))
    assert rc == capi.ERR_INVALID_ARGUMENT and not h.value, lib.vg_last_error()


def test_create_rejects_bad_cameras_before_hip(lib):
    from visgeom_amd import capi, motion_stereo

    p = motion_stereo.make_params(u_max=125, v_max=93, u0=15, v0=15, equal_margins=1, disp_max=32)
    assert _create(lib, p, c1=[0.6, 1., 0., 60., 62., 46.])[0] == capi.ERR_INVALID_ARGUMENT   # fu = 0
    assert _create(lib, p, c2=[0.6, 1., math.nan, 60., 62., 46.])[0] == capi.ERR_INVALID_ARGUMENT
    h = ctypes.c_void_p()
    assert lib.vg_motion_stereo_create(ctypes.byref(h), 0, None, None, None, ctypes.byref(p)) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_motion_stereo_set_base(None, 1, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_motion_stereo_compute(None, 1, None, None, None, None, None, None, None, None, None) == capi.ERR_INVALID_ARGUMENT
    rc, h = _create(lib, p)
    if lib.vg_device_count() == 0:
        assert rc == capi.ERR_NO_DEVICE and not h.value
        assert b"no CPU fallback" in lib.vg_last_error()
    else:
        assert rc == capi.OK
        lib.vg_motion_stereo_destroy(h)


def test_filter_hand_values():
    # K = 1 / (0.2 + 0.6); v = (2.0 * 0.6 + 2.4 * 0.2) / 0.8 = 2.1; s = max(0.2 * 0.6 / 0.8 = 0.15, 0.05 * 2.1 = 0.105)
    v, s = mr.fuse(2.0, 0.2, 2.4, 0.6)
    assert v == pytest.approx(2.1, rel=1e-15) and s == pytest.approx(0.15, rel=1e-15)
    # two tight measurements: s1 s2 K = 0.01 * 0.03 / 0.04 = 0.0075 is below the floor 0.05 v = 0.05 * 4.025 = 0.20125
    v, s = mr.fuse(4.0, 0.01, 4.1, 0.03)
    assert v == pytest.approx(4.025, rel=1e-15) and s == pytest.approx(0.20125, rel=1e-15)
    v, s = mr.fuse(1.0, 0., 2.0, 0.)   # 1 / 0: not a number, as in IEEE arithmetic
    assert v != v


def test_mask_hand_values():
    img = np.full((9, 12), 10, np.uint8)
    img[:, 6:] = 74   # a vertical edge: |gx| = 64 in columns 5 and 6, gy = 0; the 7 x 7 Gaussian has taps (1, 3.5, 7, 9, 7, 3.5, 1) / 32
    m = mr.compute_mask(img, 2)
    # the blurred row is 64 x the sum of the taps that reach columns 5 and 6, the same in every row (reflect-101 borders)
    taps = np.array([1, 3.5, 7, 9, 7, 3.5, 1]) / 32
    want = []
    for x in range(12):
        s = sum(64 * taps[k] for k in range(7) if x + k - 3 in (5, 6))
        want.append(128 if int(np.rint(s)) > 2 else 0)
    assert want == [0, 0, 0, 128, 128, 128, 128, 128, 128, 0, 0, 0]   # columns 2 and 9: 64 / 32 = 2 is not > 2
    for y in range(9):
        assert m[y].tolist() == want
    # border pixels: rows 1.. are 100, row 0 is 10.  Sobel (a central difference) gives |gy| = 90 in row 1 only: row 0 sees
    # I(1) - I(1) (reflect-101).  The blur of row 0 reads rows 3 2 1 0 1 2 3: 90 x (7 + 7) / 32 = 39.4; row 1: 90 x 9 / 32 = 25.3;
    # row 2 reads rows -1 = 1, 0, 1, ...: 90 x (1 + 7) / 32 = 22.5, rounded half to even to 22; row 3: 90 x 3.5 / 32 = 9.8
    img = np.full((9, 12), 100, np.uint8)
    img[0, :] = 10
    assert mr.compute_mask(img, 20)[:, 5].tolist() == [128, 128, 128, 0, 0, 0, 0, 0, 0]
    assert mr.compute_mask(img, 22)[:, 5].tolist() == [128, 128, 0, 0, 0, 0, 0, 0, 0]   # 22 is not > 22


@pytest.fixture(scope="module")
def sideways():
    img1, img2, rng, xi = stereo_scene.make_scene("sideways")
    M = mr.MotionStereo(stereo_scene.CAM1, stereo_scene.CAM2, mr.params(**ms.prm_of("sideways")))
    M.set_base(img1)
    return M, img2, rng, xi, M.compute(xi, img2)


def test_too_certain_rule(sideways):
    """with a prior, a search shorter than 2 samples leaves the pixel alone; without one only an empty search does"""
    M, img2, rng, xi, first = sideways
    dep = np.where(rng > 0, rng, 1.2)
    sig, cst = np.full_like(dep, 1e-9), np.full_like(dep, 40.)
    r = M.compute(xi, img2, (dep, sig, cst))
    st = r["record"][..., mr.STATUS]
    assert (st == mr.TOO_CERTAIN).sum() > 3000 and (st >= mr.REJ_SAMPLE).sum() == 0
    assert (r["record"][..., mr.DISP_MAX][st == mr.TOO_CERTAIN] < 2).all()
    assert r["depth"].tobytes() == dep.tobytes() and r["sigma"].tobytes() == sig.tobytes() and r["cost"].tobytes() == cst.tobytes()
    assert r["counts"].tolist() == [int((st == k).sum()) for k in (1, 2, 3, 4)] + [0, 0]
    wide = M.compute(xi, img2, (dep, np.full_like(dep, 0.3), cst))   # the same map with a wide sigma is searched
    assert wide["counts"][5] > 3000 and (wide["record"][..., mr.DISP_MAX][wide["record"][..., mr.STATUS] == mr.UPDATED] >= 2).all()
    assert (first["record"][..., mr.STATUS] == mr.TOO_CERTAIN).sum() == 0   # without a prior: gdispMax 1 is still searched


def test_acceptance_needs_less_than_twice_the_cost(sideways):
    """reconstruct accepts a match only if its cost is below error_max and below 2 x the pixel's cost"""
    M, img2, rng, xi, first = sideways
    rec = first["record"]
    reached = rec[..., mr.STATUS] >= mr.NOT_UPDATED
    bc = rec[..., mr.BEST_COST].astype(np.float64)
    assert (rec[..., mr.STATUS][reached & (bc < 150)] == mr.UPDATED).all() and (rec[..., mr.STATUS][reached & (bc >= 150)] == mr.NOT_UPDATED).all()
    zero = np.zeros_like(bc)   # depth 0 everywhere: every pixel takes the branch without a prior, the cost comes from the map
    at = M.compute(xi, img2, (zero, zero, bc / 2))
    above = M.compute(xi, img2, (zero, zero, bc / 2 + 0.25))
    live = reached & (bc < 150) & (rec[..., mr.DISP_MAX] >= 2)
    assert live.sum() > 3000
    assert (at["record"][..., mr.STATUS][live] == mr.NOT_UPDATED).all() and (at["depth"][live] == 0).all()
    assert (above["record"][..., mr.STATUS][live] == mr.UPDATED).all()
    assert above["depth"][live].tobytes() == first["depth"][live].tobytes() and (above["cost"][live] == bc[live]).all()


@pytest.mark.parametrize("rig", ["sideways", "vertical", "forward"])
def test_restatement_recovers_range(rig, sideways):
    if rig == "sideways":
        rng, r = sideways[2], sideways[4]
    else:
        img1, img2, rng, xi = stereo_scene.make_scene(rig)
        M = mr.MotionStereo(stereo_scene.CAM1, stereo_scene.CAM2, mr.params(**ms.prm_of(rig)))
        M.set_base(img1)
        r = M.compute(xi, img2)
    m = (r["depth"] > 0) & (rng > 0)
    assert m.sum() >= 1000
    assert np.median(np.abs(r["depth"][m] - rng[m]) / rng[m]) <= TRUTH_NO_PRIOR[rig][0] and m.mean() >= TRUTH_NO_PRIOR[rig][1]
    assert r["counts"][:5].sum() == r["depth"].size and r["counts"][5] == (r["record"][..., mr.STATUS] == mr.UPDATED).sum()


# ---- the motion_stereo program: rejected before any GPU work, one line on stderr

@pytest.fixture(scope="module")
def cli():
    from visgeom_amd import _build

    _build.build()
    return _build.MOTION_STEREO_CLI


def _rejected(r, *words):
    assert r.returncode == 1, (r.returncode, r.stderr)
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("motion_stereo: "), r.stderr
    for w in words:
        assert w in lines[0], lines[0]


def _run(cli, *args):
    return subprocess.run([cli] + list(args), capture_output=True, text=True, timeout=60)


def test_cli_usage(cli):
    r = _run(cli)
    assert r.returncode == 2 and "usage: motion_stereo sequence.json" in r.stderr


def test_cli_rejects_malformed_json(cli, tmp_path):
    path = tmp_path / "bad.json"
    path.write_text('{"camera_params_left": [1, 2, ')
    _rejected(_run(cli, str(path)), "bad.json")
    path.write_text('{"camera_params_left": [0.6, 1, 60, 60, 62, 46]}')
    _rejected(_run(cli, str(path)), "camera_params_right")


def test_cli_rejects_mismatched_counts_and_bad_images(cli, tmp_path):
    params = dict(stereo_scene.SCENE_JSON_PARAMS, motion_stereo_parameters={"gradient_thresh": 2})
    path, images, _ = ms.write_sequence(str(tmp_path), "sideways", params, n_transformations=4)
    _rejected(_run(cli, path), "6 images but 4 transformations")
    assert not (tmp_path / "depth_1.pfm").exists()
    path, _, _ = ms.write_sequence(str(tmp_path), "sideways", params)
    stereo_scene.write_pgm(str(tmp_path / "view_3.pgm"), np.zeros((93, 124), np.uint8))
    _rejected(_run(cli, path), "124 x 93", "125 x 93")
    os.remove(tmp_path / "view_3.pgm")
    _rejected(_run(cli, path), "view_3.pgm")
    bad = dict(params, stereo_parameters=dict(params["stereo_parameters"], hypotheses=2))
    path, _, _ = ms.write_sequence(str(tmp_path), "sideways", bad)
    _rejected(_run(cli, path), "hypotheses")
