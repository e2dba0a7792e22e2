"""Dense stereo on the GPU (vg_stereo_*, visgeom_amd.stereo) against the restatement (tests/stereo_ref.py): per-pixel
geometry, curve cost, aggregation + winner and depth stage by stage, ground truth on three synthetic rigs, batch
equivalence and a call whose cost volume passes 2^31 bytes."""
import numpy as np
import pytest

from tests import stereo_ref as sr
from tests import stereo_scene

pytestmark = pytest.mark.gpu

BASE = dict(u_max=125, v_max=93, u0=15, v0=15, equal_margins=1, disp_max=32, error_max=150, flaw_cost=25, desc_length=5,
            scales=[1, 2, 3, 5], desc_resp_thresh=2, use_uv_cache=0)
EPIPOLE_MARGIN = {"sideways": 2500, "vertical": 2500, "forward": 100}   # 10 px: the forward rig's epipoles are in the image
# thresholds from the restatement on these scenes (96 x 64 depth pixels, disp_max 32): sideways median relative range error
# 0.041 at 0.81 valid, vertical 0.040 at 0.72, forward 0.053 at 0.28
TRUTH = {"sideways": (0.06, 0.7), "vertical": (0.06, 0.6), "forward": (0.08, 0.2)}
SCENES = {}


@pytest.fixture(scope="module")
def torch():
    import torch

    from visgeom_amd import _build

    _build.build()
    return torch


def scene(rig):
    if rig not in SCENES:
        SCENES[rig] = stereo_scene.make_scene(rig)
    return SCENES[rig]


def prm_of(rig, **kw):
    d = dict(BASE, epipole_margin=EPIPOLE_MARGIN[rig])
    d.update(kw)
    return d


def handle(rig, p, torch):
    from visgeom_amd import stereo

    return stereo.Stereo(stereo_scene.CAM1, stereo_scene.CAM2, scene(rig)[3], stereo.make_params(**p))


def cuda(torch, *a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


@pytest.mark.parametrize("rig", ["sideways", "vertical", "forward"])
@pytest.mark.parametrize("extra", [{}, dict(scale=2, u0=11, v0=7, equal_margins=0, x_max=50, y_max=38)])
def test_geometry_bit_exact(torch, rig, extra):
    p = prm_of(rig, **extra)
    G = sr.Geometry(stereo_scene.CAM1, stereo_scene.CAM2, scene(rig)[3], sr.params(**p))
    s = handle(rig, p, torch)
    g = s.geometry().cpu().numpy()
    s.close()
    np.testing.assert_array_equal(g, G.geom)


COST_CASES = [dict(use_uv_cache=0, scales=[1]), dict(use_uv_cache=1, scales=[1]),
              dict(use_uv_cache=0, scales=[1, 2, 3, 5], image_based_cost=0),
              dict(use_uv_cache=1, scales=[1, 2, 3, 5], salient_points_only=0),
              dict(use_uv_cache=0, scales=[2, 4], desc_length=7, salient_points_only=0),
              dict(use_uv_cache=1, scales=[2, 4], desc_length=15, disp_max=48, image_based_cost=0, salient_points_only=0),
              dict(use_uv_cache=1, scales=[4], desc_length=13, disp_max=24, salient_points_only=0)]


@pytest.mark.parametrize("case", COST_CASES, ids=[str(i) for i in range(len(COST_CASES))])
def test_curve_cost_aggregation_depth_bit_exact(torch, case):
    rig = "sideways"
    img1, img2, _, xi = scene(rig)
    p = prm_of(rig, **case)
    ref = sr.stereo(stereo_scene.CAM1, stereo_scene.CAM2, xi, sr.params(**p), img1, img2)
    s = handle(rig, p, torch)
    a, b = cuda(torch, img1, img2)
    err, step, sal, skip = (t.cpu().numpy()[0] for t in s.curve_cost(a, b))
    np.testing.assert_array_equal(skip, ref["skip"])
    np.testing.assert_array_equal(step, ref["step"])
    np.testing.assert_array_equal(sal, ref["salient"])
    np.testing.assert_array_equal(err, ref["err"])
    tot, disp = (t.cpu().numpy()[0] for t in s.aggregate(a, b))
    np.testing.assert_array_equal(tot, ref["total"])
    np.testing.assert_array_equal(disp, ref["disparity"])
    dep, sig, cst, disp2 = (t.cpu().numpy() for t in s.compute(a, b))
    s.close()
    np.testing.assert_array_equal(disp2, ref["disparity"])
    np.testing.assert_array_equal(cst, ref["cost"])
    for got, want in ((dep, ref["depth"]), (sig, ref["sigma"])):
        np.testing.assert_array_equal(got == 0, want == 0)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert (ref["skip"] == 0).mean() > 0.3   # the case is not all skipped pixels


@pytest.mark.parametrize("rig", ["sideways", "vertical", "forward"])
def test_ground_truth(torch, rig):
    img1, img2, rng, xi = scene(rig)
    p = prm_of(rig)
    ref = sr.stereo(stereo_scene.CAM1, stereo_scene.CAM2, xi, sr.params(**p), img1, img2)
    s = handle(rig, p, torch)
    dep, sig, cst, disp = (t.cpu().numpy() for t in s.compute(*cuda(torch, img1, img2)))
    s.close()
    np.testing.assert_array_equal(disp, ref["disparity"])
    np.testing.assert_allclose(dep, ref["depth"], rtol=1e-12, atol=0)
    m = (dep > 0) & (rng > 0)
    med, valid = TRUTH[rig]
    assert m.mean() >= valid
    assert np.median(np.abs(dep[m] - rng[m]) / rng[m]) <= med
    if rig == "forward":   # the epipole paths ran: inverted and too-close pixels on both cameras
        g = sr.Geometry(stereo_scene.CAM1, stereo_scene.CAM2, xi, sr.params(**p)).geom
        assert (g[..., 4] & sr.TOO_CLOSE).any() and (g[..., 5] & sr.INVERTED).any()


def _pairs(n, seed=3):
    """n distinct pairs: the sideways scene with pixel noise and shifts"""
    img1, img2, _, _ = scene("sideways")
    rng = np.random.default_rng(seed)
    a = np.empty((n,) + img1.shape, np.uint8)
    b = np.empty_like(a)
    for i in range(n):
        a[i] = np.clip(img1.astype(int) + rng.integers(-6, 7, img1.shape), 0, 255)
        b[i] = np.clip(np.roll(img2, i % 3 - 1, axis=1).astype(int) + rng.integers(-6, 7, img2.shape), 0, 255)
    return a, b


def test_batch_of_8_equals_single_calls(torch):
    p = prm_of("sideways", use_uv_cache=1)
    s = handle("sideways", p, torch)
    a, b = _pairs(8)
    ta, tb = cuda(torch, a, b)
    batch = [t.cpu().numpy() for t in s.compute(ta, tb)]
    for i in range(8):
        one = [t.cpu().numpy() for t in s.compute(ta[i], tb[i])]
        for got, want in zip(one, batch):
            np.testing.assert_array_equal(got, want[i])
    s.close()


def test_call_past_2_31_bytes_is_chunked_and_equals_its_parts(torch):
    p = prm_of("sideways", disp_max=256, use_uv_cache=1)
    s = handle("sideways", p, torch)
    per_pair = s.x_max * s.y_max * 256
    n = (1 << 31) // per_pair + 8
    assert n * per_pair > 1 << 31 and s.chunk() < n
    a, b = _pairs(8)
    ta, tb = cuda(torch, a, b)
    parts = [t.cpu().numpy() for t in s.compute(ta, tb)]
    idx = torch.arange(n, device=ta.device) % 8
    big = s.compute(ta[idx].contiguous(), tb[idx].contiguous())
    for got_t, want in zip(big, parts):
        got = got_t.cpu().numpy()
        np.testing.assert_array_equal(got, want[np.arange(n) % 8])
    s.close()


def test_cli_end_to_end_equals_wrapper(torch, tmp_path):
    import subprocess

    from visgeom_amd import _build, stereo

    img1, img2, _, xi = scene("sideways")
    path = stereo_scene.write_case(str(tmp_path), "sideways", stereo_scene.SCENE_JSON_PARAMS, scene("sideways"))
    r = subprocess.run([_build.STEREO_CLI, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    import json

    p = stereo.params_from_json(json.load(open(path))["stereo_parameters"])
    dep, sig, _, _ = stereo.stereo(*cuda(torch, img1, img2), stereo_scene.CAM1, stereo_scene.CAM2, xi, p)
    dep, sig = dep.cpu().numpy(), sig.cpu().numpy()
    assert (dep > 0).mean() > 0.5
    for name, want in (("depth.pfm", dep), ("sigma.pfm", sig)):
        got = stereo_scene.read_pfm(str(tmp_path / name))
        np.testing.assert_array_equal(got, want.astype(np.float32))
    data = (tmp_path / "inverse_depth.pgm").read_bytes()
    head = b"P5\n%d %d\n255\n" % (dep.shape[1], dep.shape[0])
    assert data.startswith(head)
    inv = np.frombuffer(data[len(head):], np.uint8).reshape(dep.shape)
    with np.errstate(divide="ignore"):
        f = np.where(dep < 1e-3, np.float32(0), (1 / dep).astype(np.float32))
    want = np.clip(np.rint((f.astype(np.float32).astype(np.float64) * 0.5).astype(np.float32).astype(np.float64) * 255.), 0, 255)
    np.testing.assert_array_equal(inv, want.astype(np.uint8))
