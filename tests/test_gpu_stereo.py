"""Dense stereo on the GPU (vg_stereo_*, visgeom_amd.stereo) against the restatement (tests/stereo_ref.py): per-pixel
geometry, curve cost, aggregation + winner and depth stage by stage, on the three small rigs (up to 48 disparities) and on
the strip scene's cases (tests/stereo_strip.py: 66 ... 256 disparities, where an aggregation lane holds up to four of them);
ground truth on the three rigs, batch equivalence and a call whose cost volume passes 2^31 bytes."""
import numpy as np
import pytest

from tests import stereo_ref as sr
from tests import stereo_scene
from tests import stereo_strip as strip

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


def assert_depth_equal(got, ref):
    """(depth, sigma, cost, disparity) of compute() against a restatement output"""
    dep, sig, cst, disp = got
    np.testing.assert_array_equal(disp, ref["disparity"])
    np.testing.assert_array_equal(cst, ref["cost"])
    for g, want in ((dep, ref["depth"]), (sig, ref["sigma"])):
        np.testing.assert_array_equal(g == 0, want == 0)
        np.testing.assert_allclose(g, want, rtol=1e-12, atol=0)


def assert_stages_equal(s, a, b, ref):
    """every stage of handle `s` on the pair (a, b) against a restatement output"""
    err, step, sal, skip = (t.cpu().numpy()[0] for t in s.curve_cost(a, b))
    np.testing.assert_array_equal(skip, ref["skip"])
    np.testing.assert_array_equal(step, ref["step"])
    np.testing.assert_array_equal(sal, ref["salient"])
    np.testing.assert_array_equal(err, ref["err"])
    tot, disp = (t.cpu().numpy()[0] for t in s.aggregate(a, b))
    np.testing.assert_array_equal(tot, ref["total"])
    np.testing.assert_array_equal(disp, ref["disparity"])
    assert_depth_equal([t.cpu().numpy() for t in s.compute(a, b)], ref)


@pytest.mark.parametrize("case", COST_CASES, ids=[str(i) for i in range(len(COST_CASES))])
def test_curve_cost_aggregation_depth_bit_exact(torch, case):
    rig = "sideways"
    img1, img2, _, xi = scene(rig)
    p = prm_of(rig, **case)
    ref = sr.stereo(stereo_scene.CAM1, stereo_scene.CAM2, xi, sr.params(**p), img1, img2)
    s = handle(rig, p, torch)
    assert_stages_equal(s, *cuda(torch, img1, img2), ref)
    s.close()
    assert (ref["skip"] == 0).mean() > 0.3   # the case is not all skipped pixels


def strip_handle(p, torch):
    from visgeom_amd import stereo

    return stereo.Stereo(strip.S["cam1"], strip.S["cam2"], strip.S["xi12"], stereo.make_params(**p))


@pytest.mark.parametrize("name", [n for n in strip.CASES if n != "j"])
def test_strip_stages_bit_exact(torch, name):
    """Long disparity ranges: the aggregation slots q = 1, 2, 3, the neighbours across d = 63|64, 127|128, 191|192, the tail
    guard d < D at 66 / 120 / 130 / 200 / 254, a winner at d >= 64; the 31-row descriptor (g), a jump cost that wraps at 8
    bits (h), step_cost 0 and a tight error_max (i), one-line grids (k).  Each case first meets its conditions on the
    restatement's output (tests/stereo_strip.py)."""
    img1, img2, ref = strip.reference(name)
    strip.check_conditions(name, ref)
    s = strip_handle(strip.prm_of(name), torch)
    assert_stages_equal(s, *cuda(torch, img1, img2), ref)
    s.close()


def test_strip_odd_pixel_count_single_and_batch(torch):
    """Case j: 95 x 15 depth pixels at 130 disparities.  np (D + 3) is 1 past a multiple of 4 for one pair and 3 past it for
    three, so where the aggregation entry keeps the winner in its own scratch (disparity NULL) that buffer starts 3 and 1
    bytes behind the byte buffers.  Three distinct pairs, each against its restatement, singly and as a batch."""
    from visgeom_amd import capi

    p = strip.prm_of("j")
    P, D = p["x_max"] * p["y_max"], p["disp_max"]
    assert P % 2 == 1 and (P * (D + 3)) % 4 == 1 and (3 * P * (D + 3)) % 4 == 3
    cases = [strip.reference("j", w) for w in strip.J_BATCH]
    strip.check_conditions("j", cases[0][2])
    for _, _, ref in cases:
        assert ref["skip"].mean() <= 0.05 and (ref["disparity"] >= 0).mean() > 0.5
    s = strip_handle(p, torch)
    ta, tb = cuda(torch, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]))
    assert_stages_equal(s, ta[0], tb[0], cases[0][2])
    tot, disp = (t.cpu().numpy() for t in s.aggregate(ta, tb))
    batch = [t.cpu().numpy() for t in s.compute(ta, tb)]
    for i, (_, _, ref) in enumerate(cases):
        np.testing.assert_array_equal(tot[i], ref["total"])
        np.testing.assert_array_equal(disp[i], ref["disparity"])
        assert_depth_equal([t[i] for t in batch], ref)
        assert_depth_equal([t.cpu().numpy() for t in s.compute(ta[i], tb[i])], ref)
    for n in (1, 3):   # the winner in the entry's own scratch: the sums must not change
        own = torch.empty((n, p["y_max"], p["x_max"], D), dtype=torch.int32, device=ta.device)
        capi.check(capi.load().vg_stereo_aggregate(s._h, n, ta.data_ptr(), tb.data_ptr(), own.data_ptr(), None))   # the first n
        np.testing.assert_array_equal(own.cpu().numpy(), tot[:n])
    s.close()


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


def _pairs(n, img1, img2, seed=3):
    """n distinct pairs: a scene's pair with pixel noise and shifts"""
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
    a, b = _pairs(8, *scene("sideways")[:2])
    ta, tb = cuda(torch, a, b)
    batch = [t.cpu().numpy() for t in s.compute(ta, tb)]
    for i in range(8):
        one = [t.cpu().numpy() for t in s.compute(ta[i], tb[i])]
        for got, want in zip(one, batch):
            np.testing.assert_array_equal(got, want[i])
    s.close()


def test_call_past_2_31_bytes_is_chunked_and_equals_its_parts(torch):
    """On the strip scene (96 x 40 depth pixels over rows 4 ... 43), where 256 disparities are not all skipped pixels: the
    eight parts have winners on more than half of their pixels, some of them in the upper slots"""
    p = dict(strip.BASE, disp_max=256, use_uv_cache=1, v0=4, y_max=40)
    s = strip_handle(p, torch)
    per_pair = s.x_max * s.y_max * 256
    n = (1 << 31) // per_pair + 8
    assert n * per_pair > 1 << 31 and s.chunk() < n
    a, b = _pairs(8, *strip.images("steep", "fine")[:2])
    ta, tb = cuda(torch, a, b)
    parts = [t.cpu().numpy() for t in s.compute(ta, tb)]
    disp = parts[3]
    for i in range(8):
        assert (disp[i] >= 0).mean() > 0.5 and (disp[i] >= 128).any(), i
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
