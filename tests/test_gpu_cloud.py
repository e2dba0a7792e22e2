"""Point clouds, the plane prior and the accuracy score on the GPU (vg_depth_reconstruct, vg_depth_generate_plane, vg_depth_compare
and the stereo_accuracy program) against the restatement tests/cloud_ref.py.

What may differ.  Indices, hyp, index_map, item, valid, counts and the inlier mask are integers and compared exactly; `points`
are inputs or small integers passed through and compared exactly.  Cloud, sigma and the plane's depth are +, -, *, /, sqrt in
one order on both sides (FP64, no contraction) and are held to rtol 1e-12 with equal zero patterns, the bar of the depth and
pack tests.  The three sums of compare are added in another order than the restatement's column-major loop, so each is held to
N 2^-53 sum|term| of math.fsum over the restatement's terms: the bound of any summation order of N terms, not a measured figure."""
import ctypes
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cloud_dump
from tests import cloud_ref as cr
from tests import photometric_scene as ps
from tests import stereo_accuracy_scene as sc
from tests import stereo_mh_shapes as ms
from tests.stereo_scene import read_pfm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
CAM = ms.CAM   # alpha = 0.6: the camera refuses pixels further than about 135 px from (62.5, 46.5)
MID = ms.grid(37, 23, 60, 60, 6)     # 851 pixels, 4 workgroups, 369 of them reconstruct
LARGE = ms.grid(67, 131, 30, 0, 2)   # 8777 pixels, 35 workgroups, 5698 of them reconstruct
FIELDS = ("indices", "hyp", "points", "sigma", "index_map", "item", "valid", "cloud")
OUT_NAMES = ("indices", "hyp", "points", "sigma_out", "index_map", "item", "valid", "cloud")
F = cr


@pytest.fixture(scope="module")
def torch():
    import torch

    from visgeom_amd import _build

    _build.build()
    return torch


def cuda(torch, *a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def fusion(prm, cam=CAM):
    from visgeom_amd import depth_fusion, stereo

    return depth_fusion.DepthFusion(cam, stereo.make_params(equal_margins=0, **prm))


def random_maps(prm, K, n=1, seed=0, empty=0.4):
    """(depth, sigma) [n][K][Y][X]: depth from {0, 0.1, below MIN_DEPTH, NaN} with probability `empty`, else in [0.25, 6)"""
    def make():
        rng = np.random.default_rng(1000 * seed + 10 * K + n)
        shape = (n, K, prm["y_max"], prm["x_max"])
        depth = np.where(rng.random(shape) < empty, rng.choice([0., 0.1, ms.BELOW, NAN], size=shape), rng.uniform(0.25, 6., shape))
        depth.reshape(-1)[:2] = [0.25, ms.BELOW]   # MIN_DEPTH itself is a depth
        return depth, rng.uniform(0.01, 2., shape)
    return ms.cached(("cloud", prm["x_max"], prm["y_max"], K, n, seed, empty), make)


def queries(prm, count, seed=3):
    """(points [count][2], indices [count]): a third outside the map or not finite, some exactly between two pixels"""
    rng = np.random.default_rng(seed + count)
    X, Y, s = prm["x_max"], prm["y_max"], prm["scale"]
    pts = np.stack([rng.uniform(-0.3 * X, 1.3 * X, count), rng.uniform(-0.3 * Y, 1.3 * Y, count)], 1)
    half = rng.random(count) < 0.2
    pts[half] = np.floor(pts[half]) + 0.5          # x + 0.5: half away from zero
    pts = pts * s + [prm["u0"], prm["v0"]]
    bad = rng.random(count) < 0.05
    pts[bad, 0] = rng.choice([NAN, math.inf, -math.inf, 1e300], size=int(bad.sum()))
    idx = rng.integers(-X * Y // 4, X * Y + X * Y // 4, count).astype(np.int32)
    if count > 4:
        idx[:4] = [-1, X * Y, X * Y - 1, 0]
        idx[-1] = idx[-2]                           # a duplicate
    return pts, idx


def reference(prm, maps, flags, q=None, poses=None, cam=CAM):
    def make():
        return cr.reconstruct(cam, prm, maps[0], maps[1], flags, None if q is None else q[0], None if q is None else q[1], poses)
    key = ("ref", id(maps[0]), flags, None if q is None else len(q[0]), None if poses is None else np.asarray(poses).tobytes(), tuple(cam))
    return ms.cached(key, make)


def assert_cloud_equal(got, want):
    """a Cloud of the library against the restatement's dict"""
    assert got.counts.tolist() == want["counts"].tolist()
    for k in ("indices", "hyp", "index_map", "item", "valid"):
        g, w = getattr(got, k), want[k]
        assert (g is None) == (w is None), k
        if w is not None:
            np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=k)
    np.testing.assert_array_equal(ms.bits(got.points.cpu().numpy()), ms.bits(want["points"]))
    for k in ("sigma", "cloud"):
        g, w = getattr(got, k), want[k]
        assert (g is None) == (w is None), k
        if w is not None:
            g = g.cpu().numpy()
            assert g.shape == w.shape, k
            np.testing.assert_array_equal(g == 0, w == 0, err_msg=k)
            np.testing.assert_allclose(g, w, rtol=1e-12, atol=0, err_msg=k)


def same_bits(a, b):
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is not None:
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), k
    assert a.counts.tolist() == b.counts.tolist()


def run(torch, f, maps, flags, K, q=None, poses=None):
    d = cuda(torch, *maps)
    qp = cuda(torch, q[0])[0] if q is not None and flags & F.QUERY_POINTS else None
    qi = cuda(torch, q[1])[0] if q is not None and flags & F.QUERY_INDICES else None
    return f.reconstruct(d, flags, K, query_points=qp, query_indices=qi, poses=poses)


# ---- reconstruct at the compaction's edges ---------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", ((255, 1), (16, 16), (257, 1)))
def test_reconstruct_around_one_workgroup(torch, w, h):
    prm = ms.grid(w, h, 0, 0, 1)
    f = fusion(prm)
    maps = random_maps(prm, 4, seed=w)
    for flags in (0, F.ALL_HYPOTHESES | F.SIGMA_VALUE):
        assert_cloud_equal(run(torch, f, maps, flags, 4), reference(prm, maps, flags))
    last = np.zeros((1, 4, h, w))
    last.reshape(4, -1)[:, -1] = [1.5, 0.25, 2., 3.]   # the last pixel alone, every plane
    got = run(torch, f, (last, last + 1.), F.ALL_HYPOTHESES | F.SIGMA_VALUE, 4)
    assert got.counts.tolist() == [4] and got.indices.tolist() == [w * h - 1] * 4 and got.hyp.tolist() == [0, 1, 2, 3]
    f.close()


def test_reconstruct_35_workgroups_with_refused_pixels(torch):
    f = fusion(LARGE)
    maps = random_maps(LARGE, 2, seed=1)
    for flags in (0, F.ALL_HYPOTHESES | F.SIGMA_VALUE | F.MINMAX):
        want = reference(LARGE, maps, flags)
        assert_cloud_equal(run(torch, f, maps, flags, 2), want)
        assert 0 < want["valid"].sum() < len(want["valid"])   # the lower rows of the map are refused, its upper rows are not
    corners = np.array([0, 66, 130 * 67, 131 * 67 - 1], np.int32)   # v = 260 is 213 px below the principal point
    got = run(torch, f, maps, F.QUERY_INDICES | F.DEFAULT_VALUES, 2, q=(None, corners))
    assert got.valid.tolist() == [1, 1, 0, 0] and not got.cloud[2:].any() and got.cloud[:2].any() and got.counts.tolist() == [4]
    f.close()


@pytest.mark.parametrize("K", (1, 2, 3, 8))
def test_every_hole_pattern(torch, K):
    """every fill pattern of the first min(K, 3) planes, one pixel each, over a 257 x 3 map; the planes above are random"""
    prm = ms.grid(257, 3, 0, 0, 1)
    k3 = min(K, 3)
    pats = np.array(list(itertools.product([0., 1.], repeat=k3))).T          # [k3][2^k3]
    depth, sigma = (a.copy() for a in random_maps(prm, K, seed=5))
    flat = depth.reshape(K, -1)
    reps = flat.shape[1] // pats.shape[1]
    flat[:k3, :reps * pats.shape[1]] = np.tile(pats, reps) * np.random.default_rng(K).uniform(0.25, 4., (k3, reps * pats.shape[1]))
    f = fusion(prm)
    everything = (None, np.arange(257 * 3, dtype=np.int32))
    for flags, q in ((F.ALL_HYPOTHESES, None), (F.ALL_HYPOTHESES | F.QUERY_INDICES | F.SIGMA_VALUE, everything),
                     (F.ALL_HYPOTHESES | F.QUERY_INDICES | F.DEFAULT_VALUES | F.SIGMA_VALUE, everything)):
        want = cr.reconstruct(CAM, prm, depth, sigma, flags, query_indices=None if q is None else q[1])
        assert_cloud_equal(run(torch, f, (depth, sigma), flags, K, q=q), want)
    f.close()


def test_empty_and_full_maps(torch):
    prm = ms.grid(257, 3, 0, 0, 1)
    f = fusion(prm)
    empty = np.array([0., 0.1, ms.BELOW, NAN])[np.arange(8 * 771) % 4].reshape(1, 8, 3, 257)
    got = run(torch, f, (empty, empty), F.ALL_HYPOTHESES | F.SIGMA_VALUE, 8)
    assert got.counts.tolist() == [0] and all(len(getattr(got, k)) == 0 for k in FIELDS if getattr(got, k) is not None)
    full = ms.distinct((1, 8, 3, 257))
    got = run(torch, f, (full, full + 1.), F.ALL_HYPOTHESES | F.SIGMA_VALUE, 8)
    assert got.counts.tolist() == [8 * 771]   # 2048 entries in every full workgroup
    assert_cloud_equal(got, cr.reconstruct(CAM, prm, full, full + 1., F.ALL_HYPOTHESES | F.SIGMA_VALUE))
    f.close()


POSES = [[0.3, -0.2, 0.1, 0.02, -0.4, 0.1], [0., 0., 0., 0., 0., 0.], [-1., 2., 0.5, 1.2, 0.3, -0.7]]


def test_three_items_with_and_without_poses(torch):
    f = fusion(MID)
    parts = [random_maps(MID, 3, seed=7, empty=0.1), random_maps(MID, 3, seed=8, empty=0.9), random_maps(MID, 3, seed=9, empty=0.5)]
    maps = tuple(np.concatenate([p[i] for p in parts]) for i in range(2))   # dense, sparse, half
    flags = F.ALL_HYPOTHESES | F.SIGMA_VALUE
    plain = run(torch, f, maps, flags, 3)
    assert_cloud_equal(plain, cr.reconstruct(CAM, MID, maps[0], maps[1], flags))
    assert len(set(plain.counts.tolist())) == 3
    moved = run(torch, f, maps, flags, 3, poses=POSES)
    assert_cloud_equal(moved, cr.reconstruct(CAM, MID, maps[0], maps[1], flags, poses=POSES))
    ok = moved.valid.cpu().numpy().astype(bool)
    assert not moved.cloud.cpu().numpy()[~ok].any() and (~ok).any()          # failed entries stay (0, 0, 0) under a pose
    item1 = moved.item.cpu().numpy() == 1
    assert moved.cloud.cpu().numpy()[item1].tobytes() == plain.cloud.cpu().numpy()[item1].tobytes()   # the zero pose moves nothing
    # a batch equals its single calls; two runs give the same bits
    same_bits(moved, run(torch, f, maps, flags, 3, poses=POSES))
    first = 0
    for k in range(3):
        one = run(torch, f, tuple(m[k:k + 1] for m in maps), flags, 3, poses=POSES[k:k + 1])
        m = int(one.counts[0])
        for name in FIELDS:
            if name != "item" and getattr(one, name) is not None:
                assert getattr(moved, name)[first:first + m].cpu().numpy().tobytes() == getattr(one, name).cpu().numpy().tobytes(), (k, name)
        assert moved.item[first:first + m].tolist() == [k] * m
        first += m
    f.close()


FLAG_CASES = (F.QUERY_POINTS, F.MINMAX, F.ALL_HYPOTHESES, F.DEFAULT_VALUES, F.SIGMA_VALUE, F.QUERY_INDICES,
              F.MINMAX | F.SIGMA_VALUE, F.DEFAULT_VALUES | F.ALL_HYPOTHESES, F.QUERY_POINTS | F.INDEX_MAPPING,
              F.QUERY_INDICES | F.QUERY_POINTS, F.QUERY_INDICES | F.INDEX_MAPPING,
              F.QUERY_POINTS | F.DEFAULT_VALUES | F.ALL_HYPOTHESES | F.MINMAX | F.SIGMA_VALUE | F.INDEX_MAPPING)


@pytest.mark.parametrize("flags", FLAG_CASES)
def test_flags(torch, flags):
    f = fusion(MID)
    maps = random_maps(MID, 3, n=2, seed=11)
    q = queries(MID, 1000) if flags & (F.QUERY_POINTS | F.QUERY_INDICES) else None
    want = reference(MID, maps, flags, q)
    got = run(torch, f, maps, flags, 3, q=q)
    assert_cloud_equal(got, want)
    assert want["counts"].min() > 0
    if q is not None:
        assert want["counts"].max() < 1000 * (3 if flags & F.ALL_HYPOTHESES else 1)   # a share of the queries is outside
    f.close()


def test_index_mapping_without_a_query_is_refused(torch):
    f = fusion(MID)
    with pytest.raises(ValueError):
        f.reconstruct(cuda(torch, *random_maps(MID, 3, n=2, seed=11)), F.INDEX_MAPPING, 3)
    f.close()


@pytest.mark.parametrize("count", (0, 1, 63, 64, 65, 257, 1000))
def test_query_counts(torch, count):
    f = fusion(MID)
    maps = random_maps(MID, 3, n=2, seed=11)
    q = queries(MID, count)
    for flags in (F.QUERY_POINTS | F.INDEX_MAPPING, F.QUERY_INDICES | F.INDEX_MAPPING | F.ALL_HYPOTHESES):
        assert_cloud_equal(run(torch, f, maps, flags, 3, q=q), reference(MID, maps, flags, q))
    f.close()


def raw_call(torch, f, maps, flags, K, names, m, q=None):
    """vg_depth_reconstruct with the outputs in `names` alone, each with room for m entries: (counts, {name: array})"""
    from visgeom_amd import capi

    kinds = {"indices": ((m,), torch.int32), "hyp": ((m,), torch.int32), "points": ((m, 2), torch.float64), "sigma_out": ((m,), torch.float64),
             "index_map": ((m,), torch.int32), "item": ((m,), torch.int32), "valid": ((m,), torch.uint8),
             "cloud": ((m, 2, 3) if flags & F.MINMAX else (m, 3), torch.float64)}
    out = {k: torch.full(kinds[k][0], 7, dtype=kinds[k][1], device=maps[0].device) for k in names}
    n = maps[0].shape[0]
    counts = np.full(n, -1, np.int64)
    qp = q[0] if q is not None and flags & F.QUERY_POINTS and not flags & F.QUERY_INDICES else None
    qi = q[1] if q is not None and flags & F.QUERY_INDICES else None
    nq = 0 if q is None else len(q[0])
    st = capi.ReconOutputs(**{k: v.data_ptr() for k, v in out.items()})
    capi.check(capi.load().vg_depth_reconstruct(f._h, n, K, flags, maps[0].data_ptr(), maps[1].data_ptr(), nq, qp.data_ptr() if qp is not None else None,
                                                qi.data_ptr() if qi is not None else None, None, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                ctypes.byref(st)))
    torch.cuda.synchronize()
    return counts, {k: v.cpu().numpy() for k, v in out.items()}


def test_every_output_alone(torch):
    f = fusion(MID)
    maps = cuda(torch, *random_maps(MID, 3, n=2, seed=11))
    q = cuda(torch, *queries(MID, 257))
    flags = F.QUERY_POINTS | F.INDEX_MAPPING | F.ALL_HYPOTHESES | F.SIGMA_VALUE | F.MINMAX | F.DEFAULT_VALUES
    full = f.reconstruct(maps, flags, 3, query_points=q[0])
    m = int(full.counts.sum())
    counts, _ = raw_call(torch, f, maps, flags, 3, (), m, q)   # all outputs NULL: the call only counts
    assert counts.tolist() == full.counts.tolist() and m > 0
    for name, field in zip(OUT_NAMES, FIELDS):
        counts, out = raw_call(torch, f, maps, flags, 3, (name,), m, q)
        assert counts.tolist() == full.counts.tolist()
        assert out[name].tobytes() == getattr(full, field).cpu().numpy().tobytes(), name
    f.close()


def test_one_handle_alternating_between_small_and_large_calls(torch):
    f = fusion(MID)
    maps1, maps3 = random_maps(MID, 3, n=1, seed=12), random_maps(MID, 3, n=3, seed=13)
    calls = [(maps1, F.QUERY_INDICES, queries(MID, 1)), (maps3, F.ALL_HYPOTHESES | F.SIGMA_VALUE | F.MINMAX, None),
             (maps1, F.QUERY_POINTS | F.INDEX_MAPPING, queries(MID, 1000)), (maps3, F.QUERY_INDICES | F.ALL_HYPOTHESES, queries(MID, 65)),
             (maps1, 0, None)]
    first = [run(torch, f, maps, flags, 3, q=q) for maps, flags, q in calls]
    for (maps, flags, q), got in zip(calls, first):
        assert_cloud_equal(got, reference(MID, maps, flags, q))
    for (maps, flags, q), got in zip(reversed(calls), reversed(first)):   # the scratch has grown: the same bits in another order
        same_bits(run(torch, f, maps, flags, 3, q=q), got)
    f.close()


# ---- consistency with vg_depth_pack_mh -----------------------------------------------------------------------------------

def test_all_hypotheses_with_sigma_is_bit_identical_to_the_pack(torch):
    for prm, K in ((MID, 3), (LARGE, 2), (ms.grid(257, 3, 0, 0, 1), 8)):
        f = fusion(prm)
        maps = cuda(torch, *random_maps(prm, K, seed=21))
        got = f.reconstruct(maps, F.ALL_HYPOTHESES | F.SIGMA_VALUE, K)
        pack = f.pack_mh([m[0] for m in maps], K)
        assert len(pack[0]) == int(got.counts[0]) > 0
        for a, b in zip((got.indices, got.hyp, got.cloud, got.sigma), pack):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        f.close()


# ---- generate_plane --------------------------------------------------------------------------------------------------

PLANES = {"wall": ([0.1, -0.05, 1.5, 0.2, -0.1, 0.05], [[-0.93, -0.71, 0.], [1.07, -0.77, 0.], [1.13, 0.81, 0.], [-0.97, 0.73, 0.]]),
          "triangle": ([0., 0.1, 2., -0.3, 0.2, 0.], [[-1.31, -0.93, 0.], [1.17, -0.52, 0.], [0.13, 1.21, 0.]]),
          "gon16": ([-0.2, 0., 1.2, 0.1, 0.3, -0.2], [[0.83 * math.cos(2 * math.pi * k / 16 + 0.1), 0.61 * math.sin(2 * math.pi * k / 16 + 0.1), 0.]
                                                      for k in range(16)]),
          "edge_on": ([0.3, 0., 1., 0., 1.4, 0.], [[-1.03, -1.07, 0.], [1.01, -1.09, 0.], [1.05, 1.02, 0.], [-1.08, 1.04, 0.]])}


@pytest.mark.parametrize("name", sorted(PLANES))
@pytest.mark.parametrize("grid", ("photometric", "3x3"))
def test_generate_plane(torch, name, grid):
    cam, prm = (ps.CAM, dict(ps.PRM, u_max=ps.W, v_max=ps.H)) if grid == "photometric" else (ps.CAM, dict(scale=90, u0=38, v0=6, x_max=3, y_max=3, u_max=ps.W, v_max=ps.H))
    xi, poly = PLANES[name]
    depth, sigma, cost, margin, zdot = ms.cached(("plane", name, grid), lambda: cr.generate_plane(cam, prm, xi, poly))
    with np.errstate(invalid="ignore"):
        assert int((margin < 1e-9).sum()) == 0 and int((np.abs(zdot - 1e-3) < 1e-9).sum()) == 0   # no pixel sits on a decision
    f = fusion(prm, cam)
    got = [t.cpu().numpy() for t in f.generate_plane(xi, poly)]
    f.close()
    np.testing.assert_array_equal(got[0] == 0, depth == 0)
    np.testing.assert_allclose(got[0], depth, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(got[1], sigma)
    np.testing.assert_array_equal(got[2], cost)
    if grid == "photometric":
        assert 0 < (depth > 0).sum() < depth.size


# ---- compare ---------------------------------------------------------------------------------------------------------

def compare_case(w, h, n, seed, inliers=True):
    """(prm, depth, sigma, truth) with every branch of analyzeError: truth 0 and NaN, depth 0 and NaN, sigma above sigma_max,
    |diff| on both sides of sigma"""
    def make():
        rng = np.random.default_rng(seed)
        prm = dict(scale=2, u0=1, v0=3, x_max=w, y_max=h, u_max=2 * w + 1, v_max=2 * h + 5)
        truth = rng.uniform(0.5, 20., (n, prm["v_max"], prm["u_max"])).astype(np.float32)
        truth[rng.random(truth.shape) < 0.1] = 0.
        truth[rng.random(truth.shape) < 0.02] = NAN
        depth = truth[:, 3:3 + 2 * h:2, 1:1 + 2 * w:2].astype(np.float64) + rng.normal(0., 0.3, (n, h, w))
        depth[rng.random(depth.shape) < 0.2] = 0.
        depth[rng.random(depth.shape) < 0.02] = NAN
        depth = np.where(np.isnan(depth) & (rng.random(depth.shape) < 0.5), 1., depth)   # a depth where the truth is NaN
        sigma = rng.uniform(0.05, 0.8, depth.shape) if inliers else np.full(depth.shape, 1e-6)
        sigma[rng.random(depth.shape) < 0.1] = 11.
        sigma[rng.random(depth.shape) < 0.01] = NAN if inliers else 12.
        return prm, depth, sigma, truth
    return ms.cached(("compare", w, h, n, seed, inliers), make)


def check_compare(torch, w, h, n, seed, inliers=True):
    prm, depth, sigma, truth = compare_case(w, h, n, seed, inliers)
    f = fusion(prm)
    acc = f.compare(cuda(torch, depth, sigma), cuda(torch, truth)[0])
    again = f.compare(cuda(torch, depth, sigma), cuda(torch, truth)[0])
    f.close()
    assert acc.sums.tobytes() == again.sums.tobytes() and acc.counts.tolist() == again.counts.tolist()
    for k in range(n):
        want = cr.compare(prm, depth[k], sigma[k], truth[k])
        print(w, h, k, "counts", acc.counts[k].tolist(), "sums", acc.sums[k].tolist())
        assert acc.counts[k].tolist() == list(want["counts"])
        np.testing.assert_array_equal(acc.inliers[k].cpu().numpy(), want["inliers"])
        for j, name in enumerate(("err", "err2", "dist")):
            terms = want["terms"][name]
            exact, bound = math.fsum(terms), len(terms) * 2. ** -53 * math.fsum(abs(t) for t in terms)
            print("   ", name, acc.sums[k, j], exact, "bound", bound)
            assert abs(acc.sums[k, j] - exact) <= bound, (name, acc.sums[k, j], exact, bound)
        fig = cr.figures(want["counts"], acc.sums[k])
        got = (acc.mean_error_mm[k], acc.rms_error_mm[k], acc.inlier_percent[k], acc.mean_distance[k], acc.coverage[k])
        np.testing.assert_array_equal(np.array(got), np.array(fig))
    return acc


def test_compare_one_workgroup(torch):
    acc = check_compare(torch, 16, 16, 1, 31)
    assert acc.counts[0, 2] > 0


def test_compare_35_workgroups(torch):
    acc = check_compare(torch, 67, 131, 1, 32)
    assert 0 < acc.counts[0, 2] < acc.counts[0, 1] < acc.counts[0, 0]


def test_compare_three_items(torch):
    acc = check_compare(torch, 37, 23, 3, 33)
    assert len({tuple(c) for c in acc.counts.tolist()}) == 3


def test_compare_without_an_inlier(torch):
    acc = check_compare(torch, 37, 23, 1, 34, inliers=False)
    assert acc.counts[0, 2] == 0 and acc.counts[0, 1] > 0 and not acc.inliers.any()
    assert math.isnan(acc.mean_error_mm[0]) and math.isnan(acc.rms_error_mm[0]) and acc.inlier_percent[0] == 0. and acc.coverage[0] == 0.
    assert acc.sums[0, 0] == 0. and acc.sums[0, 1] == 0. and acc.sums[0, 2] > 0.


# ---- the program -------------------------------------------------------------------------------------------------------

def read_pgm(path):
    data = open(path, "rb").read()
    magic, w, h, maxval = data.split(None, 4)[:4]
    assert magic == b"P5" and maxval == b"255"
    return np.frombuffer(data[-int(w) * int(h):], np.uint8).reshape(int(h), int(w))


def run_program(directory, **kw):
    from visgeom_amd import _build

    path = sc.write(directory, **kw)
    res = subprocess.run([_build.STEREO_ACCURACY_CLI, path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    return directory


@pytest.fixture(scope="module")
def program(tmp_path_factory, torch):
    return run_program(tmp_path_factory.mktemp("accuracy"))


@pytest.fixture(scope="module")
def loop(torch):
    """the program's loop through the Python handles: [(image, depth, sigma)] per step, the truth, the cloud of CLOUD_STEP"""
    return cloud_dump.accuracy_loop()


def test_program_files_equal_the_loop_through_the_handles(program, loop):
    steps, truth, cloud = loop
    for i, (img, depth, sigma, acc) in enumerate(steps):
        assert np.array_equal(read_pgm(program / ("img_%d.pgm" % i)), img), i
        assert read_pfm(str(program / ("depth_%d.pfm" % i))).tobytes() == depth.astype(np.float32).tobytes(), i
        assert read_pfm(str(program / ("sigma_%d.pfm" % i))).tobytes() == sigma.astype(np.float32).tobytes(), i
    assert not (program / ("img_%d.pgm" % sc.STEP_COUNT)).exists()
    lines = (program / "cloud.txt").read_text().splitlines()
    assert len(lines) == len(cloud) > 0
    pts = np.array([[float(v) for v in ln.split()] for ln in lines])
    np.testing.assert_allclose(pts, cloud, rtol=1e-5, atol=1e-5)   # six significant digits in the file


def test_program_analysis_is_the_restatement_on_its_own_maps(program, loop):
    steps, truth, _ = loop
    lines = (program / "analysis_output.txt").read_text().splitlines()
    assert len(lines) == sc.STEP_COUNT
    for i, line in enumerate(lines):
        depth, sigma = (read_pfm(str(program / ("%s_%d.pfm" % (k, i)))).astype(np.float64) for k in ("depth", "sigma"))
        want = cr.compare(sc.GRID, depth, sigma, truth)
        ngt, nmax, n = want["counts"]
        print("step", i, line, "counts", want["counts"])
        assert n >= 1, "step %d has no inlier: its statistics are empty" % i
        fig = cr.figures(want["counts"], [math.fsum(want["terms"][k]) for k in ("err", "err2", "dist")])
        got = [float(v) for v in line.split()]
        assert len(got) == 5
        assert got[0] == pytest.approx(0.05 * (i + 1), rel=1e-3)   # the baseline: 5 cm per step
        np.testing.assert_allclose(got[1:], fig[1:], rtol=2e-5)     # six significant digits in the file
        hist = (program / ("hist_0_%d.txt" % (i + 1))).read_text().splitlines()
        assert len(hist) == nmax
        rows = np.array([[float(v) for v in ln.split()] for ln in hist])
        np.testing.assert_allclose(rows, np.array(want["hist"], np.float64), rtol=2e-5, atol=0, equal_nan=True)
        assert steps[i][3].counts.tolist() == [ngt, nmax, n]


def test_program_noise_is_the_restated_generator_and_repeats(program, tmp_path_factory, torch):
    a, b = (run_program(tmp_path_factory.mktemp("noise"), noise=8) for _ in range(2))
    for name in sorted(os.listdir(a)):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    changed = 0
    for i in range(sc.STEP_COUNT):
        clean = read_pgm(program / ("img_%d.pgm" % i))
        val = sc.noise_values(i + 1, 8, clean.size).reshape(clean.shape)
        assert 0 <= val.min() and val.max() == 7
        want = np.maximum(clean.astype(np.int64) - val, 0).astype(np.uint8)
        assert np.array_equal(read_pgm(a / ("img_%d.pgm" % i)), want), i
        changed += int((want != clean).sum())
    assert changed > 0
    assert (a / "depth_0.pfm").read_bytes() != (program / "depth_0.pfm").read_bytes()   # img1 carries noise too


# ---- the production library -----------------------------------------------------------------------------------------

def test_production_library_gives_the_same_bytes(torch, tmp_path):
    from visgeom_amd import _build

    assert os.path.exists(_build.PRODUCTION_LIB), "python -m visgeom_amd._build --production (or __graft_entry__.build())"
    here = cloud_dump.run()
    path = str(tmp_path / "production.npz")
    env = dict(os.environ, VISGEOM_AMD_LIBRARY="production")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "cloud_dump.py"), path], env=env, cwd=ROOT, timeout=300)
    got = np.load(path)
    assert int(got["has_hooks"][0]) == 0 and "production" in str(got["library"][0])
    assert len(here) > 10
    for k, v in here.items():
        assert got[k].tobytes() == np.asarray(v).tobytes(), k
