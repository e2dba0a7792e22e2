"""Multi-hypothesis stereo on the GPU (vg_stereo_compute_mh, vg_depth_regularize, vg_depth_pack_mh) against the restatement
(tests/stereo_mh_ref.py): the hypothesis planes of the sideways rig and of the strip scene's cases (up to 256 disparities, where
a lane of the selecting wave holds four of them), batch equivalence, NULL outputs, refusals, regularize and the
all-hypotheses pack.  Each case first asserts on the restatement's own output that it reaches the code it is there for."""
import ctypes

import numpy as np
import pytest

from tests import stereo_mh_ref as smh
from tests import stereo_ref as sr
from tests import stereo_scene
from tests import stereo_strip as strip
from tests.test_gpu_stereo import BASE, EPIPOLE_MARGIN

pytestmark = pytest.mark.gpu

RIG = "sideways"
WIDE = dict(error_max=40, salient_points_only=0, use_uv_cache=1)
_SCENE, _BASE_REF, _MH_REF = {}, {}, {}


@pytest.fixture(scope="module")
def torch():
    import torch

    from visgeom_amd import _build

    _build.build()
    return torch


def scene():
    if RIG not in _SCENE:
        _SCENE[RIG] = stereo_scene.make_scene(RIG)
    return _SCENE[RIG]


def rig_prm(**kw):
    return dict(BASE, epipole_margin=EPIPOLE_MARGIN[RIG], **kw)


def rig_reference(hyp, diff, **kw):
    """(single-hypothesis restatement, multi-hypothesis restatement) of the sideways rig; shared, do not change them"""
    key = tuple(sorted(kw.items()))
    img1, img2, _, xi = scene()
    prm = sr.params(**rig_prm(**kw))
    if key not in _BASE_REF:
        _BASE_REF[key] = sr.stereo(stereo_scene.CAM1, stereo_scene.CAM2, xi, prm, img1, img2)
    if (key, hyp, diff) not in _MH_REF:
        _MH_REF[key, hyp, diff] = smh.stereo_mh(stereo_scene.CAM1, stereo_scene.CAM2, xi, prm, img1, img2, hyp, diff, base=_BASE_REF[key])
    return _BASE_REF[key], _MH_REF[key, hyp, diff]


def strip_reference(name, hyp, diff, world=None):
    img1, img2, base = strip.reference(name, world)
    key = (name, world or strip.CASES[name][:2], hyp, diff)
    if key not in _MH_REF:
        xi = strip.images(*key[1])[3]
        _MH_REF[key] = smh.stereo_mh(strip.S["cam1"], strip.S["cam2"], xi, sr.params(**strip.prm_of(name)), img1, img2, hyp, diff, base=base)
    return img1, img2, base, _MH_REF[key]


def rig_handle(diff, **kw):
    from visgeom_amd import stereo

    return stereo.Stereo(stereo_scene.CAM1, stereo_scene.CAM2, scene()[3], stereo.make_params(hypo_difference=diff, **rig_prm(**kw)))


def strip_handle(name, diff):
    from visgeom_amd import stereo

    return stereo.Stereo(strip.S["cam1"], strip.S["cam2"], strip.S["xi12"], stereo.make_params(hypo_difference=diff, **strip.prm_of(name)))


def cuda(torch, *a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def assert_mh_equal(got, ref):
    """(depth, sigma, cost, disparity, final_cost) of compute_mh() against a restatement output"""
    dep, sig, cst, disp, fin = got
    np.testing.assert_array_equal(disp, ref["disparity"])
    np.testing.assert_array_equal(fin, ref["final_cost"])
    np.testing.assert_array_equal(cst, ref["cost"])
    for g, want in ((dep, ref["depth"]), (sig, ref["sigma"])):
        np.testing.assert_array_equal(g == 0, want == 0)
        np.testing.assert_allclose(g, want, rtol=1e-12, atol=0)


def above_error_max(base, mh, error_max):
    """hypotheses whose reported disparity is itself above error_max (the disparity in front of the next valid one)"""
    d = mh["disparity"]
    e = np.take_along_axis(base["err"][None].repeat(d.shape[0], 0), np.maximum(d, 0)[..., None].astype(np.int64), axis=-1)[..., 0]
    return int(((d >= 0) & (e > error_max)).sum())


def figures(base, mh, prm, diff):
    """what a multi-hypothesis result exercises, counted on the restatement"""
    d, c = mh["disparity"], mh["final_cost"].astype(np.int64)
    two = d[1:] >= 0
    sal = base["salient"] == 1
    return dict(multi=int((d[1] >= 0).sum()), equal=int((two & (c[1:] == c[:-1])).sum()),
                alternate=int(((d[2:] >= 0) & (d[2:] == d[:-2])).sum()), above=above_error_max(base, mh, prm["error_max"]),
                at_gate=int((two & (c[1:] - c[:-1] == diff)).sum()), zero=int((d == 0).sum()),
                differs=float((d[0] != base["disparity"])[sal].mean()) if sal.any() else 0.)


def run(torch, s, img1, img2, hyp):
    return [t.cpu().numpy() for t in s.compute_mh(*cuda(torch, img1, img2), hyp)]


RIG_CASES = [(4, 50), (2, 10), (8, 200)]


@pytest.mark.parametrize("hyp,diff", RIG_CASES, ids=["k%d_d%d" % c for c in RIG_CASES])
def test_sideways_planes_bit_exact(torch, hyp, diff):
    base, ref = rig_reference(hyp, diff)
    if (hyp, diff) == (4, 50):   # measured: 986, 51, 27, 35, 33, 47, 1.2 %
        f = figures(base, ref, rig_prm(), diff)
        print(f)
        assert f["multi"] >= 500 and f["equal"] >= 20 and f["alternate"] >= 10 and f["above"] >= 10, f
        assert f["at_gate"] >= 10 and f["zero"] >= 10 and f["differs"] >= 0.005, f
    s = rig_handle(diff)
    assert_mh_equal(run(torch, s, *scene()[:2], hyp), ref)
    s.close()


def test_sideways_wide_error_max_with_uv_cache(torch):
    base, ref = rig_reference(4, 50, **WIDE)
    n = above_error_max(base, ref, WIDE["error_max"])
    print(n)
    assert n >= 100   # measured 1581
    s = rig_handle(50, **WIDE)
    assert_mh_equal(run(torch, s, *scene()[:2], 4), ref)
    s.close()


STRIP_CASES = [(n, 4, 50) for n in ("a", "d66", "d130", "e", "i1", "j", "k_row", "k_col", "k_one")] + [("a", 8, 200)]


@pytest.mark.parametrize("name,hyp,diff", STRIP_CASES, ids=["%s_k%d" % c[:2] for c in STRIP_CASES])
def test_strip_planes_bit_exact(torch, name, hyp, diff):
    img1, img2, base, ref = strip_reference(name, hyp, diff)
    d = ref["disparity"]
    if name == "i1":
        n = above_error_max(base, ref, strip.prm_of(name)["error_max"])
        print(n)
        assert n >= 100   # measured 256
    if name == "a" and hyp == 4:   # measured 344 / 1402 / 1540 / 1336
        per_slot = [int(((d >= lo) & (d < hi)).sum()) for lo, hi in strip.slots(256)]
        print(per_slot)
        assert min(per_slot) >= 100, per_slot
    s = strip_handle(name, diff)
    assert_mh_equal(run(torch, s, img1, img2, hyp), ref)
    s.close()


def test_batch_of_three_equals_single_calls(torch):
    pairs = [strip.images(*w)[:2] for w in strip.J_BATCH]
    ta, tb = cuda(torch, np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    s = strip_handle("j", 50)
    batch = [t.cpu().numpy() for t in s.compute_mh(ta, tb, 4)]
    assert batch[3].shape == (3, 4, s.y_max, s.x_max) and (batch[3][:, 1] >= 0).any()
    for i in range(3):
        one = [t.cpu().numpy() for t in s.compute_mh(ta[i], tb[i], 4)]
        for got, want in zip(one, batch):
            np.testing.assert_array_equal(got, want[i])
    s.close()


def test_every_output_may_be_null(torch):
    from visgeom_amd import capi

    s = rig_handle(50)
    a, b = cuda(torch, *scene()[:2])
    full = s.compute_mh(a, b, 4)[3]
    only = torch.full_like(full, -7)
    capi.check(capi.load().vg_stereo_compute_mh(s._h, 1, a.data_ptr(), b.data_ptr(), 4, None, None, None, only.data_ptr(), None))
    np.testing.assert_array_equal(only.cpu().numpy(), full.cpu().numpy())
    capi.check(capi.load().vg_stereo_compute_mh(s._h, 1, a.data_ptr(), b.data_ptr(), 4, None, None, None, None, None))
    s.close()


def test_refusals(torch):
    from visgeom_amd import capi

    L = capi.load()
    s = rig_handle(50)
    a, b = cuda(torch, *scene()[:2])
    out = torch.empty((9, s.y_max, s.x_max), dtype=torch.int32, device=a.device)
    for n, hyp in ((1, 1), (1, 9), (1, BASE["disp_max"] + 1), (0, 4), (1, 0), (1, -1)):
        rc = L.vg_stereo_compute_mh(s._h, n, a.data_ptr(), b.data_ptr(), hyp, None, None, None, out.data_ptr(), None)
        assert rc == capi.ERR_INVALID_ARGUMENT, (n, hyp)
    assert L.vg_stereo_compute_mh(s._h, 1, None, b.data_ptr(), 4, None, None, None, out.data_ptr(), None) == capi.ERR_INVALID_ARGUMENT
    s.close()
    s = rig_handle(50, disp_max=4)   # hyp_max may not pass disp_max: the cost of plane h is the error at index h
    assert L.vg_stereo_compute_mh(s._h, 1, a.data_ptr(), b.data_ptr(), 5, None, None, None, out.data_ptr(), None) == capi.ERR_INVALID_ARGUMENT
    assert L.vg_stereo_compute_mh(s._h, 1, a.data_ptr(), b.data_ptr(), 4, None, None, None, out.data_ptr(), None) == capi.OK
    s.close()


def fusion(torch, **kw):
    from visgeom_amd import depth_fusion, stereo

    return depth_fusion.DepthFusion(stereo_scene.CAM1, stereo.make_params(**kw))


def test_regularize_sideways_map(torch):
    _, ref = rig_reference(4, 50)
    n = smh.holes(ref["depth"])
    print(n)
    assert n >= 10   # measured 19
    want = smh.regularize(ref["depth"], ref["sigma"], ref["cost"])
    maps = cuda(torch, ref["depth"], ref["sigma"], ref["cost"])
    f = fusion(torch, **rig_prm())
    assert f.regularize(maps, 4) is maps
    for got, w in zip(maps, want):
        np.testing.assert_array_equal(got.cpu().numpy(), w)
    f.close()


def test_regularize_random_maps(torch):
    rng = np.random.default_rng(5)
    depth = rng.choice([0., 0.1, 0.25, 1., 3.], size=(2, 4, 5, 7))
    sigma, cost = rng.uniform(0.01, 1., depth.shape), rng.integers(0, 255, depth.shape).astype(np.float64)
    assert sum(smh.holes(d) for d in depth) >= 40
    want = [smh.regularize(depth[i], sigma[i], cost[i]) for i in range(2)]
    maps = cuda(torch, depth, sigma, cost)
    f = fusion(torch, u_max=7, v_max=5, x_max=7, y_max=5)
    f.regularize(maps, 4)
    for k, got in enumerate(maps):
        np.testing.assert_array_equal(got.cpu().numpy(), np.stack([w[k] for w in want]))
    one = cuda(torch, depth[1], sigma[1], cost[1])   # one map [4, 5, 7]
    f.regularize(one, 4)
    for k, got in enumerate(one):
        np.testing.assert_array_equal(got.cpu().numpy(), want[1][k])
    f.close()


def test_pack_mh_of_the_regularized_sideways_map(torch):
    from visgeom_amd import capi

    _, ref = rig_reference(4, 50)
    depth, sigma, _ = smh.regularize(ref["depth"], ref["sigma"], ref["cost"])
    prm = sr.params(**rig_prm())
    idx, hyp, cloud, sig = smh.pack_mh(stereo_scene.CAM1, prm, depth, sigma)
    assert (hyp >= 1).sum() >= 100 and len(idx) > (depth[0] >= smh.MIN_DEPTH).sum()
    f = fusion(torch, **rig_prm())
    maps = cuda(torch, depth, sigma)
    cnt = ctypes.c_int64(-1)
    capi.check(capi.load().vg_depth_pack_mh(f._h, 4, maps[0].data_ptr(), maps[1].data_ptr(), ctypes.byref(cnt), None, None, None, None))
    assert cnt.value == len(idx)
    got = [t.cpu().numpy() for t in f.pack_mh(maps, 4)]
    np.testing.assert_array_equal(got[0], idx)
    np.testing.assert_array_equal(got[1], hyp)
    np.testing.assert_array_equal(got[3], sig)
    np.testing.assert_allclose(got[2], cloud, rtol=1e-12, atol=0)
    again = [t.cpu().numpy() for t in f.pack_mh(maps, 4)]   # the same order on every run
    for g, a in zip(got, again):
        np.testing.assert_array_equal(g, a)
    empty = [t.cpu().numpy() for t in f.pack_mh(cuda(torch, np.zeros_like(depth), sigma), 4)]
    assert [len(t) for t in empty] == [0, 0, 0, 0]
    f.close()
