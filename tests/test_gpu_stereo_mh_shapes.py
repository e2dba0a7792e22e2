"""Multi-hypothesis stereo on the GPU across its launch shapes and edge values, on the inputs of tests/stereo_mh_shapes.py against
the restatement (tests/stereo_mh_ref.py) at the bars of tests/test_gpu_stereo_mh.py: integers, passed-through sigma and
regularize exactly, depth, sigma and cloud to 1e-12 with equal zero patterns.
A  vg_depth_pack_mh on maps of 1 ... 513 pixels, on 256, 257 and 520 workgroups (scan runs of 1, 2 and 3) with empty workgroups
   and waves and pixels the camera refuses, with 2048 entries per workgroup, on every fill pattern of 8 planes, at MIN_DEPTH, below
   it, negative and NaN; every output alone, hyp_max 1 ... 8 on one buffer, a handle whose packs shrink and grow.
B  vg_depth_regularize on every pattern of 2 ... 8 planes over {0, 0.1, filled}, at the same edge values, on 1 ... 259 pixels with
   3 and 8 planes, on three items at once; then the chain regularize -> pack.
C  vg_stereo_compute_mh at K = 3, 5, 6, 7, 8, at K = disp_max, at hypo_difference 0, -1 and 1 000 000, with hypotheses of cost 0, in
   a call longer than a chunk, with every output alone, on a handle that alternates with vg_stereo_compute, in a batch at K = 8.
tests/test_stereo_mh_shapes_cpu.py asserts on the restatement alone that the inputs reach what they are there for."""
import ctypes

import numpy as np
import pytest

from tests import stereo_mh_ref as smh
from tests import stereo_mh_shapes as ms
from tests import stereo_scene
from tests import stereo_strip as strip
from tests.test_gpu_stereo import _pairs, assert_depth_equal
from tests.test_gpu_stereo_mh import assert_mh_equal

pytestmark = pytest.mark.gpu
PACK_NAMES = ("indices", "hyp", "cloud", "sigma_out")
MH_NAMES = ("depth", "sigma", "cost", "disparity", "final_cost")


@pytest.fixture(scope="module")
def torch():
    import torch

    from visgeom_amd import _build

    _build.build()
    return torch


def cuda(torch, *a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def host(ts):
    return [t.cpu().numpy() for t in ts]


def fusion(prm, cam=ms.CAM):
    from visgeom_amd import depth_fusion, stereo

    return depth_fusion.DepthFusion(cam, stereo.make_params(equal_margins=0, **prm))


def assert_pack_equal(got, want):
    """(indices, hyp, cloud, sigma) of the library against the restatement's"""
    assert [len(g) for g in got] == [len(w) for w in want]
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(ms.bits(got[3]), ms.bits(want[3]))
    np.testing.assert_array_equal(got[2] == 0, want[2] == 0)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-12, atol=0)


def pack_call(torch, f, K, depth, sigma, m, names):
    """vg_depth_pack_mh with the outputs in `names` alone, each of room for m entries: (count, {name: array})"""
    from visgeom_amd import capi

    kinds = {"indices": ((m,), torch.int32), "hyp": ((m,), torch.int32), "cloud": ((m, 3), torch.float64), "sigma_out": ((m,), torch.float64)}
    out = {k: torch.full(kinds[k][0], -7, dtype=kinds[k][1], device=depth.device) for k in names}
    cnt = ctypes.c_int64(-1)
    capi.check(capi.load().vg_depth_pack_mh(f._h, K, depth.data_ptr(), sigma.data_ptr() if sigma is not None else None, ctypes.byref(cnt),
                                            *[out[k].data_ptr() if k in out else None for k in PACK_NAMES]))
    return cnt.value, {k: v.cpu().numpy() for k, v in out.items()}


def assert_outputs_alone(torch, f, K, maps, full):
    """the count-only call and every output on its own give what the full call gave"""
    m = len(full[0])
    assert pack_call(torch, f, K, maps[0], maps[1], m, ())[0] == m
    for k, want in zip(PACK_NAMES, full):
        cnt, out = pack_call(torch, f, K, maps[0], maps[1], m, (k,))
        assert cnt == m
        np.testing.assert_array_equal(ms.bits(out[k]) if out[k].dtype == np.float64 else out[k], ms.bits(want) if want.dtype == np.float64 else want)


# ---- A: vg_depth_pack_mh ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", sorted(ms.SMALL))
def test_pack_small_maps(torch, P):
    f = fusion(ms.small(P, "random")[0])
    for fill in ms.FILLS:
        prm, depth, sigma = ms.small(P, fill)
        maps = cuda(torch, depth, sigma)
        got = host(f.pack_mh(maps, 4))
        assert_pack_equal(got, smh.pack_mh(ms.CAM, prm, depth, sigma))
        assert_outputs_alone(torch, f, 4, maps, got)
    f.close()


@pytest.mark.parametrize("w,h", ms.BLOCK_SHAPES)
def test_pack_many_workgroups(torch, w, h):
    prm, depth, sigma = ms.blocks(w, h)
    f = fusion(prm)
    maps = cuda(torch, depth, sigma)
    got = host(f.pack_mh(maps, 8))
    assert_pack_equal(got, ms.pack_fast(ms.CAM, prm, depth, sigma))
    assert_outputs_alone(torch, f, 8, maps, got)
    f.close()


def test_pack_full_map(torch):
    prm, depth, sigma = ms.full()
    f = fusion(prm)
    maps = cuda(torch, depth, sigma)
    got = host(f.pack_mh(maps, 8))
    assert len(got[0]) == 8 * 257 * 3
    assert_pack_equal(got, smh.pack_mh(ms.CAM, prm, depth, sigma))
    assert_outputs_alone(torch, f, 8, maps, got)
    f.close()


def test_pack_hole_patterns_and_fewer_planes_of_one_buffer(torch):
    prm, depth, sigma, _ = ms.patterns()
    f = fusion(prm)
    maps = cuda(torch, depth, sigma)
    counts = []
    for K in range(8, 0, -1):   # K < 8 reads the first K planes of the same buffers
        got = host(f.pack_mh([t[:K] for t in maps], K))
        assert_pack_equal(got, smh.pack_mh(ms.CAM, prm, depth[:K], sigma[:K]))
        counts.append(len(got[0]))
    assert counts == sorted(counts, reverse=True) and counts[0] > counts[-1] > 0
    f.close()


def test_pack_edge_values(torch):
    prm, depth, sigma, entries = ms.values()
    f = fusion(prm)
    maps = cuda(torch, depth, sigma)
    got = host(f.pack_mh(maps, 3))
    assert list(zip(got[0].tolist(), got[1].tolist())) == entries
    assert_pack_equal(got, smh.pack_mh(ms.CAM, prm, depth, sigma))
    assert np.isfinite(got[2]).all() and np.isfinite(got[3]).all()
    f.close()


def test_pack_hand_made_map_with_a_refused_row(torch):
    prm, depth, sigma = ms.hand_made()
    f = fusion(prm, ms.HAND_CAM)
    got = host(f.pack_mh(cuda(torch, depth, sigma), 2))
    assert got[0].tolist() == [0, 1, 1, 3, 3] and got[1].tolist() == [0, 0, 1, 0, 1] and got[3].tolist() == [0., 1., 5., 3., 7.]
    assert got[2][0].tolist() == [0., 0., 2.] and (got[2][3:] == 0.).all()
    assert_pack_equal(got, smh.pack_mh(ms.HAND_CAM, prm, depth, sigma))
    f.close()


def test_pack_without_sigma(torch):
    from visgeom_amd import capi

    prm, depth, sigma = ms.small(259, "random")
    f = fusion(prm)
    maps = cuda(torch, depth, sigma)
    full = host(f.pack_mh(maps, 4))
    m = len(full[0])
    cnt, out = pack_call(torch, f, 4, maps[0], None, m, ("indices", "hyp", "cloud"))   # sigma == NULL with sigma_out == NULL
    assert cnt == m
    for k, want in zip(PACK_NAMES[:3], full):
        np.testing.assert_array_equal(out[k], want)
    assert pack_call(torch, f, 4, maps[0], None, m, ())[0] == m
    one = torch.zeros(m, dtype=torch.float64, device=maps[0].device)
    c = ctypes.c_int64()
    rc = capi.load().vg_depth_pack_mh(f._h, 4, maps[0].data_ptr(), None, ctypes.byref(c), None, None, None, one.data_ptr())
    assert rc == capi.ERR_INVALID_ARGUMENT   # sigma_out needs the sigma planes
    f.close()


def test_pack_handle_shrinks_and_grows(torch):
    """a large count, an empty map, a single entry, the large count again on one handle: the block-count buffers only grow, and
    no stale count or offset may be read"""
    w, h = ms.BLOCK_SHAPES[-1]
    prm, depth, sigma = ms.blocks(w, h)
    f = fusion(prm)
    large = cuda(torch, depth, sigma)
    first = host(f.pack_mh(large, 8))
    assert len(first[0]) > 100000
    assert [len(t) for t in f.pack_mh(cuda(torch, np.zeros_like(depth), sigma), 8)] == [0, 0, 0, 0]
    single = ms.one_entry(w, h)
    got = host(f.pack_mh(cuda(torch, single, sigma), 8))
    assert_pack_equal(got, ms.pack_fast(ms.CAM, prm, single, sigma))
    assert got[0].tolist() == [(h // 2) * w + w // 2] and got[1].tolist() == [0]
    again = host(f.pack_mh(large, 8))
    for a, b in zip(first, again):
        np.testing.assert_array_equal(ms.bits(a) if a.dtype == np.float64 else a, ms.bits(b) if b.dtype == np.float64 else b)
    f.close()


# ---- B: vg_depth_regularize ------------------------------------------------------------------------------------------

def regularized(torch, f, arrays, K):
    maps = cuda(torch, *arrays)
    assert f.regularize(maps, K) is maps
    return host(maps)


def assert_bits_equal(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(ms.bits(g), ms.bits(w))


@pytest.mark.parametrize("K", range(2, 9))
def test_regularize_every_pattern(torch, K):
    arrays = ms.exhaustive(K)
    f = fusion(ms.grid(3 ** K, 1))
    assert_bits_equal(regularized(torch, f, arrays, K), smh.regularize(*arrays))
    f.close()


def test_regularize_edge_values(torch):
    depth, sigma, cost, want = ms.regularize_values()
    f = fusion(ms.grid(depth.shape[2], 1))
    got = regularized(torch, f, (depth, sigma, cost), 3)
    np.testing.assert_array_equal(ms.bits(got[0]), ms.bits(want))
    assert_bits_equal(got, smh.regularize(depth, sigma, cost))
    f.close()


@pytest.mark.parametrize("K", (3, 8))
def test_regularize_sizes(torch, K):
    for P in sorted(ms.SMALL)[:-1]:
        arrays = ms.random_map(P, K)
        f = fusion(ms.grid(*ms.SMALL[P]))
        assert_bits_equal(regularized(torch, f, arrays, K), smh.regularize(*arrays))
        f.close()


def test_regularize_three_items(torch):
    arrays = ms.random_map(259, 3, 3)   # the item stride 3 x 259 is no multiple of 64
    f = fusion(ms.grid(*ms.SMALL[259]))
    batch = regularized(torch, f, arrays, 3)
    for i in range(3):
        item = [a[i] for a in arrays]
        want = smh.regularize(*item)
        assert_bits_equal([b[i] for b in batch], want)
        assert_bits_equal(regularized(torch, f, item, 3), want)
    f.close()


def test_regularize_one_plane_and_refusals(torch):
    from visgeom_amd import capi

    L = capi.load()
    arrays = [a[:1] for a in ms.random_map(259, 3)]
    f = fusion(ms.grid(*ms.SMALL[259]))
    assert_bits_equal(regularized(torch, f, arrays, 1), arrays)   # one plane has nothing above it
    d, s, c = cuda(torch, *ms.random_map(259, 3))
    for hyp in (0, 9, -1):
        assert L.vg_depth_regularize(f._h, 1, hyp, d.data_ptr(), s.data_ptr(), c.data_ptr()) == capi.ERR_INVALID_ARGUMENT, hyp
    for args in ((None, s.data_ptr(), c.data_ptr()), (d.data_ptr(), None, c.data_ptr()), (d.data_ptr(), s.data_ptr(), None)):
        assert L.vg_depth_regularize(f._h, 1, 3, *args) == capi.ERR_INVALID_ARGUMENT
    assert L.vg_depth_regularize(None, 1, 3, d.data_ptr(), s.data_ptr(), c.data_ptr()) == capi.ERR_INVALID_ARGUMENT
    both = torch.zeros(2 * 3 * 259 - 8, dtype=torch.float64, device=d.device)   # two maps that share their last and first plane's end
    for args in ((d.data_ptr(), d.data_ptr(), c.data_ptr()), (d.data_ptr(), s.data_ptr(), s.data_ptr()),
                 (both.data_ptr(), both[3 * 259 - 8:].data_ptr(), c.data_ptr()), (d.data_ptr(), both[3 * 259 - 8:].data_ptr(), both.data_ptr())):
        assert L.vg_depth_regularize(f._h, 1, 3, *args) == capi.ERR_INVALID_ARGUMENT
    assert L.vg_depth_regularize(f._h, 1, 1, d.data_ptr(), d.data_ptr(), c.data_ptr()) == capi.ERR_INVALID_ARGUMENT   # with one plane too
    before = host((d, s, c))
    assert_bits_equal(before, ms.random_map(259, 3))   # no refused call has written
    f.close()


def test_regularize_then_pack(torch):
    depth, sigma, cost = (a.reshape(8, 81, 81) for a in ms.exhaustive(8))
    prm = ms.grid(81, 81, -60, -60)
    f = fusion(prm)
    maps = cuda(torch, depth, sigma, cost)
    f.regularize(maps, 8)
    got = host(f.pack_mh(maps, 8))
    d, s, _ = smh.regularize(depth, sigma, cost)
    assert smh.holes(maps[0].cpu().numpy()) == 0 and len(got[0]) == (depth >= smh.MIN_DEPTH).sum()
    assert_pack_equal(got, ms.pack_fast(ms.CAM, prm, d, s))
    f.close()


# ---- C: vg_stereo_compute_mh -----------------------------------------------------------------------------------------

def strip_handle(prm, diff):
    from visgeom_amd import stereo

    return stereo.Stereo(strip.S["cam1"], strip.S["cam2"], strip.S["xi12"], stereo.make_params(hypo_difference=diff, **prm))


def rig_handle(diff, cam2=stereo_scene.CAM2, xi=None, **kw):
    from visgeom_amd import stereo

    return stereo.Stereo(ms.CAM, cam2, ms.rig_scene()[3] if xi is None else xi, stereo.make_params(hypo_difference=diff, **ms.rig_prm(**kw)))


def run(torch, s, img1, img2, hyp):
    return host(s.compute_mh(*cuda(torch, img1, img2), hyp))


def mh_call(torch, s, a, b, K, names):
    """vg_stereo_compute_mh with the outputs in `names` alone: {name: tensor [n][K][y][x]}"""
    from visgeom_amd import capi

    n = a.shape[0]
    out = {k: torch.full((n, K, s.y_max, s.x_max), -7, dtype=torch.float64 if k in MH_NAMES[:3] else torch.int32, device=a.device) for k in names}
    capi.check(capi.load().vg_stereo_compute_mh(s._h, n, a.data_ptr(), b.data_ptr(), K, *[out[k].data_ptr() if k in out else None for k in MH_NAMES]))
    return out


def same_bits(torch, a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("K", ms.STRIP_K + (8,))
def test_strip_j_hypothesis_counts(torch, K):
    img1, img2, _, ref = ms.strip_reference("j", K, 200)
    assert (ref["disparity"][K - 1] >= 0).sum() >= (300 if K < 8 else 1)
    s = strip_handle(strip.prm_of("j"), 200)
    assert_mh_equal(run(torch, s, img1, img2, K), ref)
    s.close()


@pytest.mark.parametrize("D,K", ms.DISP_MAX_CASES)
def test_as_many_hypotheses_as_disparities(torch, D, K):
    """the last plane's cost is the error volume's last index"""
    _, ref = ms.rig_reference(K, 1000000, disp_max=D)
    assert (ref["disparity"][K - 1] >= 0).any() and (ref["cost"][K - 1] != ref["cost"][K - 2]).any()
    s = rig_handle(1000000, disp_max=D)
    assert_mh_equal(run(torch, s, *ms.rig_scene()[:2], K), ref)
    s.close()


@pytest.mark.parametrize("diff", ms.DIFF_CASES)
def test_hypo_difference(torch, diff):
    img1, img2, _, ref = ms.strip_reference("a", 3, diff)
    s = strip_handle(strip.prm_of("a"), diff)
    got = run(torch, s, img1, img2, 3)
    assert_mh_equal(got, ref)
    if diff == -1:
        assert (got[3][1:] == -1).all() and (got[3][0] >= 0).sum() >= 1000
    s.close()


@pytest.mark.parametrize("diff", (50, 1000000))
def test_hypotheses_of_cost_zero(torch, diff):
    _, ref = ms.zero_reference(4, diff)
    s = rig_handle(diff, cam2=ms.CAM, xi=ms.ZERO_XI)
    img1 = ms.rig_scene()[0]
    got = run(torch, s, img1, img1, 4)
    assert ((got[3][0] == 0) & (got[4][0] == 0)).sum() >= 3000
    assert_mh_equal(got, ref)
    s.close()


def test_call_longer_than_a_chunk_equals_its_parts(torch):
    s = strip_handle(ms.CHUNK_PRM, 50)
    n = s.chunk() + 8   # the multi-hypothesis chunk is never larger than the single-hypothesis one
    a, b = _pairs(8, *strip.images("steep", "fine")[:2])
    ta, tb = cuda(torch, a, b)
    parts = [torch.stack(t) for t in zip(*[s.compute_mh(ta[i], tb[i], 2) for i in range(8)])]
    disp = parts[3].cpu().numpy()
    for i in range(8):
        assert (disp[i, 0] >= 0).mean() > 0.5 and (disp[i, 1] >= 0).sum() >= 100, i
    assert all((disp[i] != disp[j]).any() for i in range(8) for j in range(i))
    idx = torch.arange(n, device=ta.device) % 8
    big_a, big_b = ta[idx].contiguous(), tb[idx].contiguous()
    big = s.compute_mh(big_a, big_b, 2)
    for k, (got, want) in enumerate(zip(big, parts)):
        assert same_bits(torch, got, want[idx]), MH_NAMES[k]
    del big
    only = mh_call(torch, s, big_a, big_b, 2, ("depth",))["depth"]   # the disparity planes are in the handle's scratch
    assert same_bits(torch, only, parts[0][idx])
    s.close()


@pytest.mark.parametrize("n", (1, 3))
def test_every_output_alone(torch, n):
    a, b = (t[:n].contiguous() for t in cuda(torch, *ms.rig_pairs()))
    s = rig_handle(50)
    full = s.compute_mh(a, b, 4)
    for i in range(n):
        np.testing.assert_array_equal(full[3][i].cpu().numpy(), ms.rig_pair_reference(i, 4, 50)["disparity"])
    for k, want in zip(MH_NAMES, full):
        assert same_bits(torch, mh_call(torch, s, a, b, 4, (k,))[k], want), k
    s.close()


def test_one_handle_alternating_between_one_and_many_hypotheses(torch):
    """the scratch is carved differently for every K: every call on a used handle gives the bits of a fresh one"""
    img1, img2, base, ref8 = ms.strip_reference("j", 8, 200)
    a, b = cuda(torch, img1, img2)
    fresh = {}
    for K in (1, 8, 2):
        s = strip_handle(strip.prm_of("j"), 200)
        fresh[K] = s.compute(a, b) if K == 1 else s.compute_mh(a, b, K)
        s.close()
    assert_depth_equal(host(fresh[1]), base)
    assert_mh_equal(host(fresh[8]), ref8)
    s = strip_handle(strip.prm_of("j"), 200)
    for step, K in enumerate((1, 8, 1, 2, 8)):
        got = s.compute(a, b) if K == 1 else s.compute_mh(a, b, K)
        for k, (g, want) in enumerate(zip(got, fresh[K])):
            assert same_bits(torch, g, want), (step, K, k)
    s.close()


def test_batch_of_three_with_eight_hypotheses(torch):
    a, b = cuda(torch, *ms.rig_pairs())
    s = rig_handle(200)
    batch = s.compute_mh(a, b, 8)
    assert batch[3].shape == (3, 8, s.y_max, s.x_max)
    for i in range(3):
        assert_mh_equal([t[i].cpu().numpy() for t in batch], ms.rig_pair_reference(i, 8, 200))
        for k, (got, want) in enumerate(zip(s.compute_mh(a[i], b[i], 8), batch)):
            assert same_bits(torch, got, want[i]), (i, k)
    s.close()
