"""Depth map propagation on the GPU (vg_depth_*, visgeom_amd.depth_fusion) against the restatement (tests/depth_ref.py): the
warp in its three regimes at two scales, its determinism and batching, its edge inputs, merge and the noise filter, the warp
and the key-frame loop against the true range, the `motion_stereo` program with the new keys and the production library."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import depth_ref as dr
from tests import depth_scene as ds
from tests import motion_ref as mr
from tests import motion_scene as ms
from tests import stereo_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIGS = ["sideways", "vertical", "forward"]
SCALE2 = dict(scale=2, u0=11, v0=7, equal_margins=0, x_max=50, y_max=38)
SCALES = {"scale1": {}, "scale2": SCALE2}
# What the restatement alone reaches, measured on the CPU: median relative range error at the share of depth pixels holding a
# depth (their number).  Bars: 1.5 x the error, 0.85 x the share, as the motion stereo tests set theirs (the GPU must equal
# the restatement; the margin only keeps the bar from being a copy).
# The true range map of the scene warped by the pose, against the true range cast from the new pose:
#   sideways  scale 1: 0.00172 at 0.8726 (5 361)   scale 2: 0.00329 at 0.8800 (1 672)
#   backward  scale 1: 0.00153 at 0.6628 (4 072)   scale 2: 0.00326 at 0.6795 (1 291)
#   forward   scale 1: 0.00251 at 0.7412 (4 554)   scale 2: 0.00562 at 0.7611 (1 446)
WARP_TRUTH = {("sideways", "scale1"): (0.00172, 0.8726), ("sideways", "scale2"): (0.00329, 0.8800),
              ("backward", "scale1"): (0.00153, 0.6628), ("backward", "scale2"): (0.00326, 0.6795),
              ("forward", "scale1"): (0.00251, 0.7412), ("forward", "scale2"): (0.00562, 0.7611)}
# The loop of tests/depth_scene.py (96 x 64 depth pixels), against the true range in the new key frame, after the key-frame
# switch and after the motion stereo step that follows it:
#   sideways  0.01272 at 0.8322 (5 113) -> 0.01001 at 0.8291 (5 094)
#   vertical  0.01319 at 0.7716 (4 741) -> 0.01074 at 0.7682 (4 720)
#   forward   0.03258 at 0.8691 (5 340) -> 0.02288 at 0.8527 (5 239)
# (before the switch, in the old key frame: sideways 0.01248 at 0.7554, vertical 0.01454 at 0.6672, forward 0.01646 at 0.2520)
LOOP_TRUTH = {"sideways": ((0.01272, 0.8322), (0.01001, 0.8291)), "vertical": ((0.01319, 0.7716), (0.01074, 0.7682)),
              "forward": ((0.03258, 0.8691), (0.02288, 0.8527))}
_CACHE = {}


@pytest.fixture(scope="module")
def torch():
    import torch

    from visgeom_amd import _build

    _build.build()
    return torch


def cuda(torch, *a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def host(maps):
    return [t.cpu().numpy() for t in maps]


def stereo_params(p):
    from visgeom_amd import stereo

    return stereo.make_params(**{k: v for k, v in p.items() if k != "gradient_thresh"})


def fusion(p):
    from visgeom_amd import depth_fusion

    return depth_fusion.DepthFusion(ds.CAM, stereo_params(p))


def sgm_map(torch, tag):
    """(depth, sigma, cost) numpy maps of vg_stereo_compute on the sideways scene, one camera; computed once per scale"""
    from visgeom_amd import stereo

    if tag not in _CACHE:
        p = ms.prm_of("sideways", **SCALES[tag])
        images, poses = ds.sequence("sideways")
        s = stereo.Stereo(ds.CAM, ds.CAM, poses[1], stereo_params(p))
        _CACHE[tag] = host(s.compute(*cuda(torch, images[0], images[1]))[:3])
        s.close()
    return _CACHE[tag]


def holes_map(prm):
    """the true range with holes, values below MIN_DEPTH and random sigma / cost"""
    rnd = np.random.default_rng(9)
    dep = ds.true_range([0.] * 6, prm)
    dep[rnd.random(dep.shape) < 0.3] = 0.
    dep[rnd.random(dep.shape) < 0.02] = 0.2
    return dep, rnd.uniform(0.01, 0.2, dep.shape), rnd.integers(0, 150, dep.shape).astype(np.float64)


def assert_maps(got, want):
    """depth, sigma to 1e-12 relative with the same zeros, cost exactly"""
    for g, w in zip(got[:2], want[:2]):
        np.testing.assert_array_equal(g == 0, w == 0)
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=0)
    if len(want) > 2:
        np.testing.assert_array_equal(got[2], want[2])


@pytest.mark.parametrize("tag", list(SCALES))
@pytest.mark.parametrize("pose", list(ds.WARP_POSES))
def test_warp_equals_restatement(torch, pose, tag):
    p = ms.prm_of("sideways", **SCALES[tag])
    prm = mr.params(**p)
    h = fusion(p)
    for maps in (sgm_map(torch, tag), holes_map(prm)):
        ref = dr.warp(ds.CAM, prm, ds.WARP_POSES[pose], *maps)
        assert ref["counts"][0] > 1000 and ref["counts"][5] > 500 and ref["counts"][0] == ref["counts"][1:].sum()
        if pose == "backward":
            assert ref["counts"][4] > 100   # many sources share a target: the depth test is exercised
        if pose == "forward":
            inner = ref["depth"][8:-8, 8:-8]
            assert (inner == 0).sum() > 20 and ref["counts"][3] > 100   # the map spreads: holes inside, sources leave the map
        got = host(h.warp(ds.WARP_POSES[pose], cuda(torch, *maps)))
        assert_maps(got, (ref["depth"], ref["sigma"], ref["cost"]))
        np.testing.assert_array_equal(h.counts[0], ref["counts"])
    h.close()


def test_warp_is_deterministic_and_a_batch_equals_single_calls(torch):
    p = ms.prm_of("sideways")
    maps = cuda(torch, *sgm_map(torch, "scale1"))
    back = ds.WARP_POSES["backward"]
    h = fusion(p)
    first = host(h.warp(back, maps))
    c_first = h.counts.copy()
    again = host(h.warp(back, maps))
    assert c_first[0, 4] > 100
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    np.testing.assert_array_equal(h.counts, c_first)
    batch = [t[None].expand(8, -1, -1).contiguous() for t in maps]
    same = host(h.warp([back] * 8, batch))
    for k in range(8):
        for a, b in zip(first, same):
            assert a.tobytes() == b[k].tobytes()
        np.testing.assert_array_equal(h.counts[k], c_first[0])
    poses = list(ds.WARP_POSES.values()) + ms.poses("sideways") + [ms.poses("vertical")[1]]
    assert len(poses) == 8
    src = [torch.stack([t * (1. + 0.01 * k) for k in range(8)]) for t in maps]
    got = host(h.warp(poses, src))
    counts = h.counts.copy()
    one = fusion(p)
    for k in range(8):
        single = host(one.warp(poses[k], [t[k] for t in src]))
        for a, b in zip(single, got):
            assert a.tobytes() == b[k].tobytes()
        np.testing.assert_array_equal(one.counts[0], counts[k])
    one.close()
    h.close()
    assert len({tuple(c) for c in counts}) == 8   # the items differ


def test_warp_edge_inputs(torch):
    from visgeom_amd import capi

    p = ms.prm_of("sideways", **SCALE2)
    h = fusion(p)
    zero = [torch.zeros((38, 50), dtype=torch.float64, device="cuda") for _ in range(3)]
    dep, sig, cst = host(h.warp(ds.WARP_POSES["sideways"], zero))
    assert (dep == 0).all() and (sig == 30.).all() and (cst == 5.).all()
    assert h.counts.tolist() == [[0] * 6]
    maps = cuda(torch, *holes_map(mr.params(**p)))
    out = [torch.empty_like(maps[0]) for _ in range(3)]
    xi = np.array(ds.WARP_POSES["sideways"], dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)

    def call(xi, src, dst):
        return capi.load().vg_depth_warp(h._h, 1, xi.ctypes.data_as(dp), *[t.data_ptr() for t in src], *[t.data_ptr() for t in dst], None)

    assert call(xi, maps, out) == capi.OK
    for dst in ([maps[0], out[1], out[2]], [out[0], maps[2], out[2]], [out[0], out[1], out[0]]):   # aliased outputs
        assert call(xi, maps, dst) == capi.ERR_INVALID_ARGUMENT
    bad = xi.copy()
    bad[4] = np.nan
    assert call(bad, maps, out) == capi.ERR_INVALID_ARGUMENT
    assert "finite" in capi.load().vg_last_error().decode()
    with pytest.raises(ValueError):
        h.warp(bad, maps)
    with pytest.raises(ValueError):
        h.warp(xi, [t[:10] for t in maps])
    h.close()


def test_merge_and_filter_equal_restatement(torch):
    p = ms.prm_of("sideways")
    prm = mr.params(**p)
    a, b = ds.synthetic_maps(prm)
    sgm = sgm_map(torch, "scale1")
    warped = dr.warp(ds.CAM, prm, ds.WARP_POSES["sideways"], *a)
    h = fusion(p)
    for m1, m2 in ((a, b), ((warped["depth"], warped["sigma"], warped["cost"]), sgm)):
        ref = dr.merge(m1[0], m1[1], m2[0], m2[1])
        if m1 is a:
            assert (ref["counts"] > 20).all()   # every outcome of merge
        t1, t2 = cuda(torch, *m1), cuda(torch, *m2)
        back = h.merge(t1, t2)
        assert back is t1
        assert_maps(host(t1), (ref["depth"], ref["sigma"], m1[2]))
        np.testing.assert_array_equal(h.counts[0], ref["counts"])
        assert ref["counts"].sum() == m1[0].size
    for m in (a, sgm):
        ref = dr.filter_noise(m[0], m[1])
        assert ref["counts"][0] > 1000 and ref["counts"][0] == ref["counts"][1:].sum()
        if m is a:
            assert (ref["counts"] > 20).all()   # cleared and smoothed pixels
        t = cuda(torch, *m)
        got = h.filter_noise(t)
        assert_maps(host(got[:2]), (ref["depth"], ref["sigma"]))
        assert got[2] is t[2]
        np.testing.assert_array_equal(h.counts[0], ref["counts"])
        c_out = h.counts.copy()
        h.filter_noise(t, out=t[:2])   # in place: through the handle's copy
        np.testing.assert_array_equal(h.counts, c_out)
        for x, y in zip(host(got[:2]), host(t[:2])):
            assert x.tobytes() == y.tobytes()
    h.close()


def test_filter_passes_a_two_wide_map_through(torch):
    from visgeom_amd import depth_fusion, stereo

    h2 = depth_fusion.DepthFusion(ds.CAM, stereo.make_params(u_max=125, v_max=93, x_max=2, y_max=40))
    rnd = np.random.default_rng(1)
    dep, sig = rnd.uniform(1, 3, (40, 2)), rnd.uniform(0.01, 0.1, (40, 2))
    got = h2.filter_noise(cuda(torch, dep, sig))
    assert got[0].cpu().numpy().tobytes() == dep.tobytes() and got[1].cpu().numpy().tobytes() == sig.tobytes()
    assert h2.counts.tolist() == [[0, 0, 0]]
    h2.close()


@pytest.mark.parametrize("tag", list(SCALES))
@pytest.mark.parametrize("pose", list(ds.WARP_POSES))
def test_warp_of_the_true_range_against_the_range_cast_from_the_new_pose(torch, pose, tag):
    p = ms.prm_of("sideways", **SCALES[tag])
    prm = mr.params(**p)
    rng0 = ds.true_range([0.] * 6, prm)
    h = fusion(p)
    dep = h.warp(ds.WARP_POSES[pose], cuda(torch, rng0, np.full_like(rng0, 0.1), np.full_like(rng0, 7.)))[0].cpu().numpy()
    h.close()
    err, share, n = ds.stat(dep, ds.true_range(ds.WARP_POSES[pose], prm))
    print("warp of the true range, %s %s: median relative range error %.5f, share %.4f, %d pixels" % (pose, tag, err, share, n))
    e0, s0 = WARP_TRUTH[pose, tag]
    assert err <= 1.5 * e0 and share >= 0.85 * s0


class GpuOps:
    """the loop's operations on the library; maps are (depth, sigma, cost) CUDA tensors"""

    def __init__(self, torch, mp):
        from visgeom_amd import depth_fusion, motion_stereo

        self.torch, self.mp = torch, mp   # mp: a vg_motion_stereo_params
        self.M = motion_stereo.MotionStereo(ds.CAM, ds.CAM, mp)
        self.F = depth_fusion.DepthFusion(ds.CAM, mp)

    def close(self):
        self.M.close()
        self.F.close()

    def set_base(self, img):
        self.M.set_base(cuda(self.torch, img)[0])

    def sgm(self, img1, img2, xi):
        from visgeom_amd import stereo

        return stereo.stereo(*cuda(self.torch, img1, img2), ds.CAM, ds.CAM, xi, self.mp.stereo)[:3]

    def motion(self, xi, img, maps):
        return self.M.compute(xi, cuda(self.torch, img)[0], maps)

    def filter_noise(self, maps):
        return self.F.filter_noise(maps)

    def warp(self, xi, maps):
        return self.F.warp(xi, maps)

    def merge(self, maps, maps2):
        return self.F.merge(maps, maps2)


@pytest.mark.parametrize("rig", RIGS)
def test_key_frame_loop_equals_the_restatements_and_recovers_the_range(torch, rig):
    from visgeom_amd import depth_fusion, motion_stereo

    p = ms.prm_of(rig)
    prm = mr.params(**p)
    images, poses = ds.sequence(rig)
    ops = GpuOps(torch, motion_stereo.make_params(**p))
    got = ds.run_loop(ops, images, poses, depth_fusion.pose_in_frame, depth_fusion.pose_inverse)
    ops.close()
    ref = ds.run_loop(ds.RefOps(prm), images, poses, depth_fusion.pose_in_frame, depth_fusion.pose_inverse)
    for k, (g, w) in enumerate(zip(got, ref)):
        assert_maps(host(g), w)
    rng = ds.true_range(poses[ds.KEY_INDEX], prm)
    for k, what in ((3, "after the key-frame switch"), (4, "after the step in the new frame")):
        err, share, n = ds.stat(got[k][0].cpu().numpy(), rng)
        print("%s, %s: median relative range error %.5f, share %.4f, %d pixels" % (rig, what, err, share, n))
        e0, s0 = LOOP_TRUTH[rig][k - 3]
        assert n >= 1000 and err <= 1.5 * e0 and share >= 0.85 * s0


def test_cli_with_filter_noise_and_a_key_frame_equals_the_python_loop(torch, tmp_path):
    from visgeom_amd import _build, depth_fusion, motion_stereo

    rig = "sideways"
    images, poses = ds.sequence(rig)
    names = ["key.pgm"] + ["view_%d.pgm" % i for i in range(1, len(images))]
    for name, im in zip(names, images):
        stereo_scene.write_pgm(str(tmp_path / name), im)
    params = dict(stereo_scene.SCENE_JSON_PARAMS, motion_stereo_parameters={"gradient_thresh": 2})
    doc = {"camera_params_left": ds.CAM, "camera_params_right": ds.CAM, "images": names, "transformations": poses,
           "stereo_parameters": params, "sgm_frames": 1, "filter_noise": True, "key_frames": [ds.KEY_INDEX]}
    path = str(tmp_path / "sequence.json")
    with open(path, "w") as f:
        json.dump(doc, f)
    r = subprocess.run([_build.MOTION_STEREO_CLI, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ops = GpuOps(torch, motion_stereo.params_from_json(params))
    got = ds.run_loop(ops, images, poses, depth_fusion.pose_in_frame, depth_fusion.pose_inverse)
    ops.close()
    for i, maps in enumerate(got, start=1):
        for name, want in (("depth_%d.pfm" % i, maps[0]), ("sigma_%d.pfm" % i, maps[1])):
            np.testing.assert_array_equal(stereo_scene.read_pfm(str(tmp_path / name)), want.cpu().numpy().astype(np.float32))
    assert (got[-1][0] > 0).float().mean() > 0.5


def _dump(tmp_path, which):
    env = dict(os.environ)
    env.pop("VISGEOM_AMD_LIBRARY", None)
    if which == "production":
        env["VISGEOM_AMD_LIBRARY"] = "production"
    path = str(tmp_path / ("%s.npz" % which))
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "depth_dump.py"), path], env=env, cwd=ROOT)
    return np.load(path)


def test_production_library_gives_the_same_bits(tmp_path):
    from visgeom_amd import _build

    assert os.path.exists(_build.PRODUCTION_LIB), "python -m visgeom_amd._build --production (or __graft_entry__.build())"
    a, b = _dump(tmp_path, "hooks"), _dump(tmp_path, "production")
    assert int(a["has_hooks"][0]) == 1 and int(b["has_hooks"][0]) == 0
    keys = sorted(k for k in a.files if k != "has_hooks")
    assert keys == sorted(k for k in b.files if k != "has_hooks") and len(keys) == 10
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert a["warp_counts"][0, 4] > 100 and (a["merge_counts"] > 20).all() and (a["filter_counts"] > 20).all()
