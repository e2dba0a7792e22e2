"""Monocular odometry without a GPU: section 15 of the C ABI is declared, exported and bound, its defaults are the reference's
constants, every entry refuses bad arguments before HIP is touched, the host arithmetic of the state machine agrees with the
numpy restatement (tests/mono_odom_ref.py) within the project's parity bar, and the scene of the GPU test
(tests/mono_odom_scene.py) satisfies the conditions its branches depend on."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mono_odom_ref as mr
from tests import mono_odom_scene as sc
from tests import photometric_ref as pr
from tests import photometric_scene as ps

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "visgeom_amd.h")
ENTRIES = ("vg_mono_odom_params_default", "vg_mono_odom_create", "vg_mono_odom_destroy", "vg_mono_odom_size", "vg_mono_odom_feed_wheel_odometry",
           "vg_mono_odom_feed_image", "vg_mono_odom_set_depth", "vg_mono_odom_warp_image", "vg_mono_odom_state", "vg_mono_odom_xi_local",
           "vg_mono_odom_xi_global", "vg_mono_odom_xi_composed", "vg_mono_odom_num_keyframes", "vg_mono_odom_keyframe_increment",
           "vg_mono_odom_get_map", "vg_mono_odom_map", "vg_mono_odom_integrate", "vg_mono_odom_normalize_scale", "vg_mono_odom_needs_keyframe",
           "vg_mono_odom_camera_motion", "vg_mono_odom_compose")
RTOL = 1e-10   # the project's parity bar
dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def lib():
    from visgeom_amd import _build, capi

    _build.build()
    return capi.load()


def scene_params(**kw):
    from visgeom_amd import mono_odom, motion_stereo

    return mono_odom.make_params(motion=motion_stereo.make_params(**sc.STEREO), **dict(sc.THRESHOLDS, **kw))


def test_section_15_is_declared_exported_and_bound(lib):
    from visgeom_amd import _build, capi

    declared = set(re.findall(r"\b(vg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    for path in (_build.LIB, _build.build_production()):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = set(re.findall(r" T (vg_[a-z0-9_]+)", out))
        for name in ENTRIES:
            assert name in declared and name in exported and name in capi.SIGNATURES, (name, path)
    assert sorted(s for s in declared if s.startswith("vg_mono_odom_")) == sorted(ENTRIES)
    assert os.path.join(_build.CSRC, "vg_mono_odom_tu.hip") in _build.sources()
    assert os.path.exists(_build.MONO_ODOM_CLI)


def test_defaults_are_the_references_constants(lib):
    from visgeom_amd import capi, mono_odom, motion_stereo, sparse_odom

    p = mono_odom.default_params()
    assert (p.min_init_dist, p.max_dist, p.max_angle, p.min_scale_length, p.max_scale_ratio, p.num_scales) == (0.25, 0.4, math.pi / 4, 1e-2, 1.2, 5)
    assert bytes(p.motion) == bytes(motion_stereo.default_params()) and bytes(p.sparse) == bytes(sparse_odom.default_params())
    assert {k: getattr(p, k) for k in mr.DEFAULTS} == mr.DEFAULTS
    assert (capi.MONO_ODOM_REPORT, capi.MONO_ODOM_READY, capi.MONO_ODOM_DISCARDED) == (16, 2, 5)
    text = open(HEADER).read()
    for i, name in enumerate(mono_odom.ACTIONS):
        assert re.search(r"#define VG_MONO_ODOM_%s %d\b" % (name, i), text), name
    for i, name in enumerate(mono_odom.STATES):
        assert re.search(r"#define VG_MONO_ODOM_%s %d\b" % (name, i), text), name
    q = mono_odom.params_from_json(sc.json_parameters())
    assert list(q[0]) == sc.CAM and np.allclose(q[1], sc.XI_BASE_CAM, rtol=0, atol=1e-15)
    assert bytes(q[2]) == bytes(scene_params())


def test_every_entry_refuses_bad_arguments_before_hip_is_touched(lib):
    from visgeom_amd import capi

    cam, xbc = np.array(sc.CAM, float), np.array(sc.XI_BASE_CAM, float)

    def create(p, cam=cam, xbc=xbc, w=sc.W, h=sc.H):
        hd = ctypes.c_void_p()
        rc = lib.vg_mono_odom_create(ctypes.byref(hd), 0, None, cam.ctypes.data_as(dp) if cam is not None else None,
                                     xbc.ctypes.data_as(dp) if xbc is not None else None, w, h, ctypes.byref(p) if p is not None else None)
        return rc, hd, lib.vg_last_error().decode()

    def refused(word, p=None, **kw):
        rc, hd, msg = create(p if p is not None else scene_params(), **kw)
        assert rc == capi.ERR_INVALID_ARGUMENT and not hd.value and word in msg, (rc, msg, word)

    assert lib.vg_mono_odom_create(None, 0, None, None, None, sc.W, sc.H, None) == capi.ERR_INVALID_ARGUMENT
    assert create(None)[0] == capi.ERR_INVALID_ARGUMENT
    assert create(scene_params(), cam=None)[0] == capi.ERR_INVALID_ARGUMENT
    refused("finite", scene_params(max_dist=float("nan")))
    refused("negative", scene_params(min_init_dist=-1.))
    refused("positive", scene_params(max_scale_ratio=0.))
    refused("uMax x vMax", w=sc.W + 1)
    refused("uMax x vMax", h=sc.H - 1)
    refused("xi_base_cam", xbc=np.array([0., 0., float("inf"), 0., 0., 0.]))
    refused("finite", cam=np.array([0.6, float("nan"), 127., 125., 128., 96.]))
    # the arguments of each of the four pipelines, though the first of them would already miss its device here
    p = scene_params()
    p.motion.gradient_thresh = 300
    refused("gradient_thresh", p)
    p = scene_params()
    p.motion.stereo.disp_max = 5
    refused("disparity_max", p)
    refused("num_scales", scene_params(num_scales=9))
    p = scene_params()
    p.sparse.max_features = 0
    refused("", p)
    import torch

    if not torch.cuda.is_available():
        rc, hd, msg = create(scene_params())
        assert rc == capi.ERR_NO_DEVICE and not hd.value and "no CPU fallback" in msg
    # NULL handles and NULL arguments
    six, n, i64 = (ctypes.c_double * 6)(), ctypes.c_int(), ctypes.c_int64()
    ptr = ctypes.c_void_p()
    for rc in (lib.vg_mono_odom_size(None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)),
               lib.vg_mono_odom_feed_wheel_odometry(None, six), lib.vg_mono_odom_feed_image(None, None, None, None),
               lib.vg_mono_odom_set_depth(None, None), lib.vg_mono_odom_warp_image(None, None, None, None, None),
               lib.vg_mono_odom_state(None, ctypes.byref(n)), lib.vg_mono_odom_xi_local(None, six), lib.vg_mono_odom_xi_global(None, six),
               lib.vg_mono_odom_xi_composed(None, six), lib.vg_mono_odom_num_keyframes(None, ctypes.byref(i64)),
               lib.vg_mono_odom_keyframe_increment(None, 0, six), lib.vg_mono_odom_get_map(None, None, None, None),
               lib.vg_mono_odom_map(None, ctypes.byref(ptr), ctypes.byref(ptr), ctypes.byref(ptr)),
               lib.vg_mono_odom_integrate(six, six, None, six), lib.vg_mono_odom_integrate(six, six, six, None),
               lib.vg_mono_odom_normalize_scale(None, six, six, six, six, None, ctypes.byref(n)),
               lib.vg_mono_odom_normalize_scale(ctypes.byref(scene_params()), six, six, six, six, None, None),
               lib.vg_mono_odom_normalize_scale(ctypes.byref(scene_params(max_scale_ratio=-1.)), six, six, six, six, None, ctypes.byref(n)),
               lib.vg_mono_odom_needs_keyframe(None, six, ctypes.byref(n)), lib.vg_mono_odom_needs_keyframe(ctypes.byref(scene_params()), six, None),
               lib.vg_mono_odom_camera_motion(six, None, six), lib.vg_mono_odom_compose(None, six, six)):
        assert rc == capi.ERR_INVALID_ARGUMENT
    lib.vg_mono_odom_destroy(None)
    lib.vg_mono_odom_params_default(None)


def close(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.allclose(a, b, rtol=RTOL, atol=RTOL * max(1e-3, float(np.abs(b).max())))


POSES = [np.zeros(6), np.array([0.1, -0.2, 0.3, 0., 0., 0.]), np.array([0., 0., 0., 0.3, -0.2, 0.1]), np.array([0.4, 0.1, -0.3, 0.5, 0.2, -0.7]),
         np.array([-0.05, 0.02, 0.03, 1e-7, -2e-7, 1e-7]), np.array(sc.XI_BASE_CAM)]


def test_integrate_camera_motion_and_compose_match_the_restatement(lib):
    from visgeom_amd import mono_odom

    for a in POSES:
        for b in POSES:
            assert close(mono_odom.compose(a, b), pr.compose(a, b))
            assert close(mono_odom.camera_motion(a, b), mr.camera_motion(a, b))
            for c in POSES[1::2]:
                assert close(mono_odom.integrate(a, b, c), mr.integrate(a, b, c))
    z = np.zeros(6)
    assert np.array_equal(mono_odom.integrate(z, z, z), z) and np.array_equal(mono_odom.camera_motion(z, z), z)


def test_normalize_scale_matches_the_restatement_at_its_branches(lib):
    from visgeom_amd import mono_odom

    p, prm = scene_params(), sc.PRM
    old = np.array([0.05, -0.01, 0.08, 0.01, 0.02, -0.015])
    step = np.array([-0.03, 0.005, 0.04, 0.002, 0.004, -0.001])
    unit = step[:3] / np.linalg.norm(step[:3])

    def moved(length, rot=step[3:]):
        return pr.compose(old, np.concatenate([unit * length, rot]))

    cases = {"identity": (np.zeros(6), np.zeros(6), np.zeros(6)),
             "pure rotation": (old, moved(0.), moved(0., rot=[0.01, -0.02, 0.005])),
             "K below": (old, moved(0.05 * 1.19), moved(0.05)), "K above": (old, moved(0.05 * 1.21), moved(0.05)),
             "length below": (old, moved(0.05), moved(0.0099)), "length above": (old, moved(0.05), moved(0.0101)),
             "shorter odometry": (old, moved(0.03), moved(0.05))}
    seen = set()
    for name, (o, prior, vo) in cases.items():
        xi, K, disc = mono_odom.normalize_scale(p, o, prior, vo)
        rxi, rK, rdisc, length, _ = mr.normalize_scale(prm, o, prior, vo)
        assert disc == rdisc, name
        assert close(xi, rxi), name
        assert (not math.isfinite(rK) and not math.isfinite(K)) or abs(K - rK) <= RTOL * abs(rK), (name, K, rK)
        seen.add((disc, length > prm["min_scale_length"], math.isfinite(rK)))
        if name in ("identity", "pure rotation"):   # length 0: K is not finite, no rescale and no discard
            assert not math.isfinite(K) and not disc and close(xi, vo), name
        if name == "K above":   # DISCARDED returns xi_local_old o zetaPrior, the odometry's pose
            assert disc and close(xi, prior) and close(xi, pr.compose(o, pr.inverse_compose(o, prior)))
        if name == "K below":
            assert not disc and abs(np.linalg.norm(pr.inverse_compose(o, xi)[:3]) - 0.05 * 1.19) < 1e-12
        if name == "length below":   # K = 5 but the step is too short to be judged: VO kept as it is
            assert not disc and K > prm["max_scale_ratio"] and close(xi, vo)
        if name == "length above":
            assert disc
    assert seen == {(False, False, False), (True, True, True), (False, True, True), (False, False, True)}


def test_needs_keyframe_is_strict_at_its_thresholds(lib):
    from visgeom_amd import mono_odom

    p, prm = scene_params(max_dist=0.5, max_angle=0.25), dict(sc.PRM, max_dist=0.5, max_angle=0.25)
    for xi, want in (([0.5, 0., 0., 0., 0., 0.], False), ([0., 0., math.nextafter(0.5, 1.), 0., 0., 0.], True),
                     ([0., 0., 0., 0., 0.25, 0.], False), ([0., 0., 0., math.nextafter(0.25, 1.), 0., 0.], True),
                     ([0.3, 0.4, 0., 0.15, 0.2, 0.], False), ([0.3, 0.4, 0.01, 0., 0., 0.], True), ([0., 0., 0., 0., 0., 0.], False)):
        assert mono_odom.needs_keyframe(p, xi) == want == mr.needs_keyframe(prm, xi), xi


def test_the_scene_reaches_every_branch_when_the_estimates_are_the_truth():
    """the state machine of the restatement on the true poses: the actions of the scene's table, K of the two special frames"""
    prm, odo, true = sc.PRM, sc.odometry(), sc.true_poses()
    state, local, old, glob, xi_odom, actions, key = "BEGIN", np.zeros(6), np.zeros(6), np.zeros(6), None, [], 0
    K_of = {}
    for k in range(sc.N_FRAMES):
        local = mr.integrate(local, xi_odom, odo[k]) if xi_odom is not None else local
        xi_odom = odo[k]
        if state == "BEGIN":
            local, glob, state = np.zeros(6), np.zeros(6), "SPARSE_INIT"
            actions.append("FIRST")
        elif state == "SPARSE_INIT":
            if np.linalg.norm(local[:3]) >= prm["min_init_dist"]:
                local = old = pr.inverse_compose(true[key], true[k])   # what sparse odometry is to find
                glob, local, state, key = pr.compose(glob, local), np.zeros(6), "READY", k
                actions.append("SPARSE_INIT_KEYFRAME")
            else:
                actions.append("WAITING")
        else:
            vo = pr.inverse_compose(true[key], true[k])   # what the photometric solve is to find
            local, K, disc, _, _ = mr.normalize_scale(prm, old, local, vo)
            K_of[k] = K
            if disc:
                actions.append("DISCARDED")
                continue
            old = local
            if mr.needs_keyframe(prm, local):
                glob, local, key = pr.compose(glob, local), np.zeros(6), k
                actions.append("KEYFRAME")
            else:
                actions.append("REFINED")
    assert actions == sc.ACTIONS
    assert set(actions) == {"FIRST", "WAITING", "SPARSE_INIT_KEYFRAME", "REFINED", "KEYFRAME", "DISCARDED"}
    assert K_of[sc.INFLATED] > prm["max_scale_ratio"] and abs(K_of[sc.INFLATED] - sc.INFLATION) < 0.01
    # the perturbed frame: not discarded (the offset is perpendicular to the motion), and every other frame far from it
    assert 1.1 < K_of[sc.PERTURBED] < 1.17
    assert all(abs(K - 1.) < 0.02 for k, K in K_of.items() if k not in (sc.PERTURBED, sc.INFLATED))


def test_the_perturbed_frame_starts_within_what_the_photometric_tests_converge_from():
    start, truth = sc.odometry_local(sc.PERTURBED), sc.true_local(sc.PERTURBED)
    d = pr.inverse_compose(truth, start)
    off = np.asarray(ps.START_OFFSET)
    assert 0.5 * np.linalg.norm(off[:3]) < np.linalg.norm(d[:3]) <= 1.001 * np.linalg.norm(off[:3])
    assert 0.5 * np.linalg.norm(off[3:]) < np.linalg.norm(d[3:]) <= 1.001 * np.linalg.norm(off[3:])


def test_the_restatement_of_warp_image_and_set_depth_on_a_small_case():
    """properties of the restatement itself: the identity pose with a full map returns the image where the cell's depth is
    valid, holes and depths below MIN_DEPTH give 0, and set_depth picks the grid's pixels"""
    rng = np.random.default_rng(3)
    w, h = 67, 45
    grid = dict(scale=2, u0=5, v0=4, x_max=(w - 10) // 2 + 1, y_max=(h - 8) // 2 + 1)
    cam = [0.6, 1.05, 33., 32., 33.5, 22.5]
    src = rng.integers(1, 255, (h, w)).astype(np.uint8)
    depth = np.full((grid["y_max"], grid["x_max"]), 1.5)
    depth[3, 4], depth[5, 6] = 0., 0.2
    dst, near = mr.warp_image(cam, grid, src, depth, np.zeros(6))
    vv, uu = np.mgrid[0:h, 0:w]
    xd, yd = mr.c_round((uu - 5) / 2.), mr.c_round((vv - 4) / 2.)
    covered = (xd >= 0) & (xd < grid["x_max"]) & (yd >= 0) & (yd < grid["y_max"])
    hole = covered & (((xd == 4) & (yd == 3)) | ((xd == 6) & (yd == 5)))
    assert hole.sum() >= 6 and (dst[hole] == 0).all() and (dst[~covered] == 0).all()
    good = covered & ~hole & ~near
    assert good.sum() > 0.8 * covered.sum() and np.array_equal(dst[good], src[good])
    image = rng.random((h, w)).astype(np.float32)
    d, s = mr.set_depth(grid, image)
    assert d.shape == (grid["y_max"], grid["x_max"]) and d[2, 3] == np.float64(image[4 + 2 * 2, 5 + 3 * 2]) and (s == 0.1).all()
