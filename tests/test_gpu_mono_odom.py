"""Monocular odometry on the GPU (include/visgeom_amd.h section 15) on the scene of tests/mono_odom_scene.py, rendered by
visgeom_amd.render.Renderer as the reference's program renders its input.

The loop equals its stages: the same state machine is written out below on the public classes of the stages (SparseOdometry,
Stereo, MotionStereo, DepthFusion, Photometric) with the host arithmetic of visgeom_amd.mono_odom (held to the numpy restatement
in tests/test_mono_odom_cpu.py) and depth_fusion.pose_in_frame.  Every stage is bit-reproducible and batch-independent, so poses, reports and maps are compared
bit for bit after every frame.  set_depth and warp_image are compared bit for bit with tests/mono_odom_ref.py.

Accuracy against the renderer's ground truth is recorded by tools/bench_mono_odom.py, not asserted here."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from tests import mono_odom_ref as mr
from tests import mono_odom_scene as sc
from tests import photometric_ref as pr
from tests.stereo_scene import read_pfm

pytestmark = pytest.mark.gpu
ZERO = np.zeros(6)


def scene_params():
    from visgeom_amd import mono_odom, motion_stereo

    return mono_odom.make_params(motion=motion_stereo.make_params(**sc.STEREO), **sc.THRESHOLDS)


def bits(t):
    import torch

    return t.contiguous().view(torch.int64)


def same_maps(a, b):
    import torch

    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


class StageLoop:
    """MonoOdometry::feedWheelOdometry / feedImage / pushKeyFrame on the stages' own handles"""

    def __init__(self, p):
        from visgeom_amd.depth_fusion import DepthFusion
        from visgeom_amd.motion_stereo import MotionStereo
        from visgeom_amd.photometric import Photometric
        from visgeom_amd.sparse_odom import SparseOdometry

        self.p = p
        self.sparse = SparseOdometry(sc.CAM, sc.XI_BASE_CAM, sc.W, sc.H, p.sparse)
        self.motion = MotionStereo(sc.CAM, sc.CAM, p.motion)
        self.fusion = DepthFusion(sc.CAM, p.motion)
        self.photo = Photometric(sc.CAM, p.motion, sc.XI_BASE_CAM, sc.W, sc.H, p.num_scales)
        self.state, self.local, self.old, self.glob, self.xi_odom = "BEGIN", ZERO, ZERO, ZERO, None
        self.key, self.map, self.transf = None, None, []

    def close(self):
        for h in (self.sparse, self.motion, self.fusion, self.photo):
            h.close()

    def feed_wheel_odometry(self, xi):
        from visgeom_amd import mono_odom

        if self.xi_odom is not None:
            self.local = mono_odom.integrate(self.local, self.xi_odom, xi)
        self.xi_odom = np.array(xi, float)

    def push_keyframe(self, img, rep):
        from visgeom_amd import depth_fusion, mono_odom
        from visgeom_amd.stereo import Stereo

        motion = mono_odom.camera_motion(sc.XI_BASE_CAM, self.local)
        sgm = Stereo(sc.CAM, sc.CAM, depth_fusion.pose_inverse(motion), self.p.motion.stereo)
        new = sgm.compute(img, self.key)[:3]
        sgm.close()
        if self.state == "READY":
            warped = self.fusion.warp(motion, self.map)
            self.fusion.merge(warped[:2], new[:2])
            rep["counts"][:5] = self.fusion.counts[0]
            self.map = warped
        else:
            self.map = new
        self.glob = mono_odom.compose(self.glob, self.local)
        self.transf.append(self.local)
        self.local = ZERO
        self.key = img
        self.motion.set_base(img)

    def feed_image(self, img, samples):
        from visgeom_amd import depth_fusion, mono_odom

        rep = {"state_before": self.state, "action": "WAITING", "K": 0., "length": 0., "length_prior": 0., "iterations": 0, "final_cost": 0.,
               "termination": 0, "counts": np.zeros(6, np.int64)}
        if self.state == "BEGIN":
            self.local = self.glob = ZERO
            self.key = img
            self.transf = [ZERO]
            self.sparse.feed(img, ZERO, samples)
            self.motion.set_base(img)
            self.state, rep["action"] = "SPARSE_INIT", "FIRST"
        elif self.state == "SPARSE_INIT":
            if np.linalg.norm(self.local[:3]) >= self.p.min_init_dist:
                self.local, _ = self.sparse.feed(img, self.local, samples)
                self.old = self.local
                self.push_keyframe(img, rep)
                self.state, rep["action"] = "READY", "SPARSE_INIT_KEYFRAME"
        else:
            self.photo.set_base(self.key, self.map[0])
            self.photo.set_targets(img)
            vo, solve = self.photo.compute_pose(self.local, xi_prior=self.local)
            rep["iterations"], rep["final_cost"], rep["termination"] = int(solve[:, 0].sum()), solve[0, 2], int(solve[0, 3])
            zeta_prior, zeta = depth_fusion.pose_in_frame(self.old, self.local), depth_fusion.pose_in_frame(self.old, vo)
            self.local, rep["K"], discarded = mono_odom.normalize_scale(self.p, self.old, self.local, vo)
            rep["length"], rep["length_prior"] = (math.sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]) for z in (zeta, zeta_prior))
            if discarded:
                rep["action"] = "DISCARDED"
            else:
                self.old = self.local
                if mono_odom.needs_keyframe(self.p, self.local):
                    self.push_keyframe(img, rep)
                    rep["action"] = "KEYFRAME"
                else:
                    rep["action"] = "REFINED"
                    motion = mono_odom.camera_motion(sc.XI_BASE_CAM, self.local)
                    if motion[:3] @ motion[:3] > 1e-10:
                        self.motion.compute(motion, img, prior=self.map, out=self.map)
                        rep["counts"][:] = self.motion.counts[0]
                        self.fusion.filter_noise(self.map[:2], out=self.map[:2])
        rep["state"], rep["keyframes"] = self.state, len(self.transf)
        return rep


def same_report(a, b):
    """every field bit for bit (K is not finite for a pure rotation: equal_nan)"""
    for k in ("state_before", "state", "action", "iterations", "termination", "keyframes"):
        if a[k] != b[k]:
            return False
    numbers = ("K", "final_cost", "length", "length_prior")
    if not np.array_equal(np.array([a[k] for k in numbers]), np.array([b[k] for k in numbers]), equal_nan=True):
        return False
    return np.array_equal(a["counts"], b["counts"])


@pytest.fixture(scope="module")
def frames():
    """the scene's images with the exact depth buffers, rendered once"""
    from visgeom_amd.render import Renderer

    bg, planes = sc.world()
    r = Renderer(sc.CAM, sc.W, sc.H, bg, planes)
    img, depth = r.render(sc.camera_poses(), buffers=True)[:2]
    r.close()
    return img, depth


@pytest.fixture(scope="module")
def samples():
    return np.random.default_rng(5).integers(0, 1 << 20, (200, 2)).astype(np.int32)


@pytest.fixture(scope="module")
def run(frames, samples):
    """the scene through MonoOdometry and through the stages, a snapshot of both after every frame (read only)"""
    from visgeom_amd.mono_odom import MonoOdometry

    p = scene_params()
    odo, loop = MonoOdometry(sc.CAM, sc.XI_BASE_CAM, p), StageLoop(p)
    snaps = []
    for k in range(sc.N_FRAMES):
        for h in (odo, loop):
            h.feed_wheel_odometry(sc.odometry()[k])
        start = odo.xi_local
        ra, rb = odo.feed_image(frames[0][k], samples), loop.feed_image(frames[0][k], samples)
        snaps.append(dict(start=start, report=ra, report_stages=rb, local=odo.xi_local, glob=odo.xi_global, composed=odo.xi_composed,
                          local_stages=np.array(loop.local), glob_stages=np.array(loop.glob), transf=odo.keyframe_increments,
                          transf_stages=np.array(loop.transf), map=odo.map if odo.state == "READY" else None,
                          map_stages=[t.clone() for t in loop.map] if loop.map is not None else None, state=odo.state))
    yield dict(snaps=snaps, odo=odo, loop=loop, params=p)
    odo.close()
    loop.close()


def test_the_loop_equals_its_stages(run):
    from visgeom_amd import mono_odom

    actions = []
    for k, s in enumerate(run["snaps"]):
        print("frame %d: %s" % (k, {key: s["report"][key] for key in ("action", "K", "iterations", "final_cost")}))
        assert same_report(s["report"], s["report_stages"]), (k, s["report"], s["report_stages"])
        for a, b in (("local", "local_stages"), ("glob", "glob_stages"), ("transf", "transf_stages")):
            assert np.array_equal(s[a], s[b]), (k, a, s[a], s[b])
        assert np.array_equal(s["composed"], mono_odom.compose(s["glob"], s["local"])), k
        assert (s["map"] is None) == (s["map_stages"] is None), k
        if s["map"] is not None:
            assert same_maps(s["map"], s["map_stages"]), k
        actions.append(s["report"]["action"])
    # a scene that never reaches a branch fails rather than passes
    assert set(actions) == set(mono_odom.ACTIONS), actions
    assert run["snaps"][-1]["report"]["keyframes"] == len(run["snaps"][-1]["transf"]) >= 3


def test_set_depth_seeds_the_map_and_the_next_frame_localises_from_it(frames, samples):
    import torch

    from visgeom_amd.mono_odom import MonoOdometry

    img, depth = frames
    p = scene_params()
    odo, loop = MonoOdometry(sc.CAM, sc.XI_BASE_CAM, p), StageLoop(p)
    try:
        # a map that did not exist: the depth buffer on the grid, sigma 0.1 and the cost of a fresh DepthMap
        odo.set_depth(depth[0])
        want_d, want_s = mr.set_depth(sc.GRID, depth[0].cpu().numpy())
        d, s, c = (t.cpu().numpy() for t in odo.map)
        assert np.array_equal(d, want_d) and np.array_equal(s, want_s) and (c == mr.DEFAULT_COST).all()
        first_key = sc.ACTIONS.index("SPARSE_INIT_KEYFRAME")
        for k in range(first_key + 1):
            for h in (odo, loop):
                h.feed_wheel_odometry(sc.odometry()[k])
                rep = h.feed_image(img[k], samples)
        assert rep["action"] == "SPARSE_INIT_KEYFRAME" and odo.state == "READY"
        assert same_maps(odo.map, loop.map)   # the seeded map was replaced by the first key frame's SGM map
        cost_before = odo.map[2].clone()
        # an existing map: depth and sigma replaced, the cost left alone
        odo.set_depth(depth[first_key])
        want_d, want_s = mr.set_depth(sc.GRID, depth[first_key].cpu().numpy())
        d, s, c = odo.map
        assert np.array_equal(d.cpu().numpy(), want_d) and np.array_equal(s.cpu().numpy(), want_s) and torch.equal(bits(c), bits(cost_before))
        loop.map = (torch.from_numpy(want_d).to(d.device), torch.from_numpy(want_s).to(d.device), loop.map[2])
        k = first_key + 1
        for h in (odo, loop):
            h.feed_wheel_odometry(sc.odometry()[k])
        ra, rb = odo.feed_image(img[k], samples), loop.feed_image(img[k], samples)
        assert ra["action"] == "REFINED" and same_report(ra, rb), (ra, rb)
        assert np.array_equal(odo.xi_local, loop.local) and same_maps(odo.map, loop.map)
    finally:
        odo.close()
        loop.close()


def warp_case(width, height, grid, cam, seed):
    """(src, depth, poses): a random image, a map with a slanted surface, holes and depths below MIN_DEPTH, and poses of which
    the last moves part of the image outside src"""
    rng = np.random.default_rng(seed)
    src = rng.integers(1, 256, (height, width)).astype(np.uint8)
    yy, xx = np.mgrid[0:grid["y_max"], 0:grid["x_max"]]
    depth = 1. + 0.8 * xx / grid["x_max"] + 0.3 * yy / grid["y_max"]
    pick = rng.random(depth.shape)
    depth[pick < 0.05] = 0.
    depth[(pick >= 0.05) & (pick < 0.08)] = 0.1
    return src, depth, [[0.02, -0.01, 0.05, 0.01, -0.02, 0.005], [0.5, 0.1, -0.3, 0.05, 0.4, -0.1]]


def check_warp(odo, cam, grid, xbc, src, depth, poses):
    import torch

    from visgeom_amd import mono_odom

    h, w = src.shape
    for xi in poses:
        got = odo.warp_image(torch.from_numpy(src).cuda(), xi, torch.from_numpy(depth).cuda()).cpu().numpy()
        want, near = mr.warp_image(cam, grid, src, depth, mono_odom.camera_motion(xbc, xi))
        print("warp %d x %d: %d pixels within 1e-9 of a rounding boundary, %d written" % (w, h, near.sum(), (want != 0).sum()))
        assert near.sum() <= 0.001 * w * h
        assert np.array_equal(got[~near], want[~near]), (xi, int((got != want)[~near].sum()))
        assert 0.02 * w * h < (want != 0).sum() < w * h
    # the second pose leaves part of the image without a source
    covered = mr.warp_image(cam, grid, np.full_like(src, 255), np.where(depth >= mr.MIN_DEPTH, depth, 1.), np.zeros(6))[0] != 0
    lost = covered & (mr.warp_image(cam, grid, np.full_like(src, 255), np.where(depth >= mr.MIN_DEPTH, depth, 1.), mono_odom.camera_motion(xbc, poses[-1]))[0] == 0)
    assert lost.sum() > 0.02 * w * h


def test_warp_image_equals_the_restatement(run):
    from visgeom_amd import mono_odom, motion_stereo
    from visgeom_amd.mono_odom import MonoOdometry

    src, depth, poses = warp_case(sc.W, sc.H, sc.GRID, sc.CAM, 31)
    check_warp(run["odo"], sc.CAM, sc.GRID, sc.XI_BASE_CAM, src, depth, poses)
    # an odd width and a pixel count that is no multiple of the workgroup size
    w, h = 67, 45
    grid = dict(scale=2, u0=5, v0=4, x_max=(w - 10) // 2 + 1, y_max=(h - 8) // 2 + 1)
    cam = [0.6, 1.05, 33., 32., 33.5, 22.5]
    p = mono_odom.make_params(motion=motion_stereo.make_params(u_max=w, v_max=h, **grid), num_scales=1)
    small = MonoOdometry(cam, sc.XI_BASE_CAM, p)
    try:
        assert (w * h) % 256 and (small.x_max, small.y_max) == (grid["x_max"], grid["y_max"])
        check_warp(small, cam, grid, sc.XI_BASE_CAM, *warp_case(w, h, grid, cam, 32))
    finally:
        small.close()


def test_the_photometric_pose_aligns_the_perturbed_frame_better_than_its_odometry(run, frames):
    """the key frame against the new image warped into it, at the pose feed_image started from and at the one it arrived at;
    only pixels written in both warps count"""
    s = run["snaps"][sc.PERTURBED]
    assert s["report"]["action"] == "REFINED"
    off = pr.inverse_compose(sc.true_local(sc.PERTURBED), s["start"])
    print("perturbed frame: start off by %.4f m, %.5f rad; K %.4f" % (np.linalg.norm(off[:3]), np.linalg.norm(off[3:]), s["report"]["K"]))
    odo, img = run["odo"], frames[0]
    key = img[max(k for k, a in enumerate(a["report"]["action"] for a in run["snaps"]) if a.endswith("KEYFRAME"))]
    before, after = odo.warp_image(img[sc.PERTURBED], s["start"]), odo.warp_image(img[sc.PERTURBED], s["local"])
    both = (before != 0) & (after != 0)
    assert both.sum() > 0.05 * sc.W * sc.H
    mad = [float((w[both].double() - key[both].double()).abs().mean()) for w in (before, after)]
    print("mean absolute difference to the key frame: %.3f at the odometry pose, %.3f at the estimated pose, %d pixels" % (mad[0], mad[1], both.sum()))
    assert mad[1] < mad[0]


def test_refusals_and_lifetime(frames):
    import torch

    from visgeom_amd import capi
    from visgeom_amd.mono_odom import MonoOdometry

    img = frames[0]
    p = scene_params()
    a, b = MonoOdometry(sc.CAM, sc.XI_BASE_CAM, p), MonoOdometry(sc.CAM, sc.XI_BASE_CAM, p)
    try:
        with pytest.raises(ValueError):
            a.feed_image(img[0][:, :-1])
        with pytest.raises(ValueError):
            a.feed_image(img[0].cpu())
        with pytest.raises(ValueError):
            a.feed_image(img[:2])
        with pytest.raises(ValueError):
            a.feed_wheel_odometry([0., 0., float("nan"), 0., 0., 0.])
        with pytest.raises(ValueError):
            a.warp_image(img[0], [0., float("inf"), 0., 0., 0., 0.])
        with pytest.raises(ValueError):
            a.set_depth(img[0])
        bad = (ctypes_double6(float("nan")))
        assert capi.load().vg_mono_odom_feed_wheel_odometry(a._h, bad) == capi.ERR_INVALID_ARGUMENT
        with pytest.raises(capi.VisgeomError) as e:   # no map yet
            a.warp_image(img[0])
        assert e.value.code == capi.ERR_STATE
        with pytest.raises(capi.VisgeomError) as e:
            a.map
        assert e.value.code == capi.ERR_STATE
        # an image before any odometry: xi_local = 0
        rep = a.feed_image(img[0])
        assert rep["action"] == "FIRST" and a.state == "SPARSE_INIT" and not a.xi_local.any() and not a.xi_composed.any()
        assert a.feed_image(img[1])["action"] == "WAITING" and b.state == "BEGIN"
        # two handles side by side: b runs on while a waits
        for k in range(4):
            b.feed_wheel_odometry(sc.odometry()[k])
            rep = b.feed_image(img[k])
        assert rep["action"] == "SPARSE_INIT_KEYFRAME" and b.state == "READY" and a.state == "SPARSE_INIT"
        assert len(b.keyframe_increments) == 2 and b.map[0].shape == (b.y_max, b.x_max)
        assert torch.isfinite(b.map[0]).all()
    finally:
        a.close()
        b.close()
    a.close()   # a second close is harmless


def ctypes_double6(v):
    import ctypes

    return (ctypes.c_double * 6)(v, 0., 0., 0., 0., 0.)


def test_the_program_in_both_input_modes(tmp_path):
    """mono_odom on the scene: rendered by the program itself from the world file, and from the frames as PGM files; the
    trajectory's poses are the handle's through the reference's number format, the key frame maps the handle's bit for bit"""
    from tests import render_scene
    from visgeom_amd import _build
    from visgeom_amd.mono_odom import MonoOdometry

    from visgeom_amd import mono_odom
    from visgeom_amd.render import Renderer

    # what the program computes: poses composed by the library, views rendered at them, the library's own draw of the samples
    poses = [np.zeros(6)]
    for _ in range(sc.N_FRAMES - 1):
        poses.append(mono_odom.compose(poses[-1], sc.ZETA))
    bg, planes = sc.world()
    r = Renderer(sc.CAM, sc.W, sc.H, bg, planes)
    views = r.render(np.array([mono_odom.compose(xi, sc.XI_BASE_CAM) for xi in poses]))
    r.close()
    img = views.cpu().numpy()
    odo = MonoOdometry(sc.CAM, sc.XI_BASE_CAM, scene_params())
    lines, maps = [], {}
    try:
        for k in range(sc.N_FRAMES):
            odo.feed_wheel_odometry(poses[k])
            rep = odo.feed_image(views[k])
            lines.append("%d %s %s %s" % (k, rep["state"], rep["action"], " ".join("%g" % v for v in list(odo.xi_composed) + [rep["K"]])))
            if rep["action"].endswith("KEYFRAME"):
                maps[str(rep["keyframes"] - 1)] = [t.cpu().numpy() for t in odo.map[:2]]
        maps["final"] = [t.cpu().numpy() for t in odo.map[:2]]
    finally:
        odo.close()
    assert len(maps) >= 3
    for mode in ("render", "images"):
        d = tmp_path / mode
        d.mkdir()
        doc = sc.json_parameters()
        if mode == "render":
            doc["render"] = sc.write_world(str(d))
            doc["trajectory"] = {"initial": [0.] * 6, "increment": sc.ZETA, "step_count": sc.N_FRAMES}
        else:
            doc["images"] = ["frame_%d.pgm" % k for k in range(sc.N_FRAMES)]
            doc["odometry"] = [list(map(float, xi)) for xi in poses]
            doc["warp"] = True
            for k in range(sc.N_FRAMES):
                render_scene.write_pgm(str(d / ("frame_%d.pgm" % k)), img[k])
        with open(d / "sequence.json", "w") as f:
            json.dump(doc, f)
        res = subprocess.run([_build.MONO_ODOM_CLI, str(d / "sequence.json")], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        assert (d / "trajectory.txt").read_text().splitlines() == lines, mode
        for tag, (depth, sigma) in maps.items():
            assert np.array_equal(read_pfm(str(d / ("depth_%s.pfm" % tag))), depth.astype(np.float32)), (mode, tag)
            assert np.array_equal(read_pfm(str(d / ("sigma_%s.pfm" % tag))), sigma.astype(np.float32)), (mode, tag)
        if mode == "images":
            assert os.path.exists(d / ("warp_%d.pgm" % (sc.N_FRAMES - 1))) and not os.path.exists(d / "warp_0.pgm")
    # a JSON with neither input is refused before the GPU is touched
    with open(tmp_path / "bad.json", "w") as f:
        json.dump(sc.json_parameters(), f)
    res = subprocess.run([_build.MONO_ODOM_CLI, str(tmp_path / "bad.json")], capture_output=True, text=True, timeout=60)
    assert res.returncode == 1 and "exactly one of" in res.stderr
