"""Trajectory planning without a GPU: section 17 of the C ABI is declared, exported and bound and refuses bad arguments before HIP
is touched; the host arithmetic (the integrated trajectories, the points of a numerical gradient) against the restatement
(tests/trajectory_ref.py); the restatement's own figures on the test scene, which the GPU tests rely on; and the minimiser
(visgeom_amd/csrc/vg_bfgs.hpp) on its own, driven by tests/host/bfgs_check.cpp under a plain host compiler."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import trajectory_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "visgeom_amd.h")
PLAN = os.path.join(ROOT, "tests", "golden", "trajectory_plan.json")
ENTRIES = ("vg_trajectory_default_options", "vg_trajectory_create", "vg_trajectory_destroy", "vg_trajectory_size", "vg_trajectory_evaluate",
           "vg_trajectory_visual_cov", "vg_trajectory_gradient", "vg_trajectory_gradient_points", "vg_trajectory_poses",
           "vg_trajectory_optimize", "vg_trajectory_project_board", "vg_trajectory_launch_count")
dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int)
i32p = ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def lib():
    from visgeom_amd import _build, capi

    _build.build()
    return capi.load()


@pytest.fixture(scope="module")
def scene():
    cam, w, h, q, steps, start = tr.load_plan(PLAN)
    return dict(cam=cam, w=w, h=h, q=q, steps=steps, start=np.array(start))


def test_section_17_is_declared_exported_and_bound(lib):
    from visgeom_amd import _build, capi

    declared = set(re.findall(r"\b(vg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    for path in (_build.LIB, _build.build_production()):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = set(re.findall(r" T (vg_[a-z0-9_]+)", out))
        for name in ENTRIES:
            assert name in declared and name in exported and name in capi.SIGNATURES, (name, path)
    assert sorted(s for s in declared if s.startswith("vg_trajectory_")) == sorted(ENTRIES)
    assert os.path.exists(_build.TRAJECTORY_CLI) and _build.CLI_SOURCES["trajectory"] == "trajectory_main.cpp"
    opt = capi.TrajectoryOptions()
    lib.vg_trajectory_default_options(ctypes.byref(opt))
    assert (opt.function_tolerance, opt.gradient_tolerance, opt.parameter_tolerance, opt.max_iterations) == (1e-6, 1e-10, 1e-8, 1000)


def _create(lib, scene, model=0, cam=None, width=None, height=None, steps=None, **changes):
    from visgeom_amd import trajectory

    q = trajectory.make_quality(scene["q"])
    for k, v in changes.items():
        if isinstance(v, (list, tuple)):
            getattr(q, k)[:] = v
        else:
            setattr(q, k, v)
    c = np.array(scene["cam"] if cam is None else cam, dtype=np.float64)
    s = np.array(scene["steps"] if steps is None else steps, dtype=np.intc)
    h = ctypes.c_void_p()
    rc = lib.vg_trajectory_create(ctypes.byref(h), 0, None, model, c.ctypes.data_as(dp), scene["w"] if width is None else width,
                                  scene["h"] if height is None else height, ctypes.byref(q), s.size, s.ctypes.data_as(ip))
    return rc, h, lib.vg_last_error().decode()


def test_create_refuses_bad_scenes_before_hip_is_touched(lib, scene):
    from visgeom_amd import capi

    def refused(word, **kw):
        rc, h, msg = _create(lib, scene, **kw)
        assert rc == capi.ERR_INVALID_ARGUMENT and not h.value and word in msg, (kw, rc, msg)

    refused("EUCM", model=capi.MODEL_UCM)
    refused("EUCM", model=capi.MODEL_MEI)
    refused("finite", cam=[0.7, float("nan"), 380., 380., 520., 360.])
    refused("non-zero", cam=[0.7, 1., 0., 380., 520., 360.])
    refused("positive", width=0)
    refused("finite", xi_base_cam=[0., 0., float("inf"), 0., 0., 0.])
    refused("cols, rows >= 2", board_cols=1)
    refused("1024 corners", board_cols=33, board_rows=32)
    refused("step", board_step=0.)
    refused("turn_radius", turn_radius=0.)
    refused("prior_variance", prior_variance=[1e-2, 1e-2, 0., 1e-2, 1e-2, 1e-2])
    refused("feature_variance", feature_variance=-1.)
    refused("min_camera_dist", min_margin=float("nan"))
    refused("trajectories", steps=[])
    refused("trajectories", steps=[3] * 9)
    refused("[2, 256]", steps=[4, 1])
    refused("[2, 256]", steps=[257, 4])
    assert lib.vg_trajectory_create(None, 0, None, 0, None, 1, 1, None, 0, None) == capi.ERR_INVALID_ARGUMENT
    import torch

    if not torch.cuda.is_available():   # a good scene: only the device is missing
        for kw in ({}, dict(steps=[256] * 8), dict(board_cols=32, board_rows=32)):
            rc, h, msg = _create(lib, scene, **kw)
            assert rc == capi.ERR_NO_DEVICE and not h.value, (rc, msg)


def test_calls_refuse_bad_arguments_before_hip_is_touched(lib, scene):
    from visgeom_amd import capi

    p = np.zeros((2, 10))
    out = np.zeros(2 * 36)
    inv = np.zeros(2, dtype=np.int32)
    a = lambda x: x.ctypes.data_as(dp)   # noqa: E731
    for n in (-1, 65536):
        assert lib.vg_trajectory_evaluate(None, n, a(p), a(out), None, None) == capi.ERR_INVALID_ARGUMENT
        assert b"[0, 65535]" in lib.vg_last_error()
        assert lib.vg_trajectory_visual_cov(None, n, a(p), a(out), a(out), inv.ctypes.data_as(i32p)) == capi.ERR_INVALID_ARGUMENT
        assert b"pose count must be in [0, 65535]" in lib.vg_last_error()
    for call in (lambda: lib.vg_trajectory_evaluate(None, 2, a(p), a(out), None, None),
                 lambda: lib.vg_trajectory_gradient(None, 2, a(p), a(out), a(out), None),
                 lambda: lib.vg_trajectory_optimize(None, 2, a(p), None, a(out), None, None),
                 lambda: lib.vg_trajectory_visual_cov(None, 2, a(p), a(out), a(out), inv.ctypes.data_as(i32p))):
        assert call() == capi.ERR_INVALID_ARGUMENT and b"handle is NULL" in lib.vg_last_error()
    n = ctypes.c_int()
    c = ctypes.c_int64()
    assert lib.vg_trajectory_size(None, ctypes.byref(n), None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_trajectory_launch_count(None, ctypes.byref(c)) == capi.ERR_INVALID_ARGUMENT
    lib.vg_trajectory_destroy(None)
    # the host-only entries
    steps = np.array([4, 7], dtype=np.intc)
    xi = np.zeros((11, 6))
    bad = p[0].copy()
    bad[3] = np.nan
    assert lib.vg_trajectory_poses(2, steps.ctypes.data_as(ip), a(bad), a(xi), None) == capi.ERR_INVALID_ARGUMENT and b"finite" in lib.vg_last_error()
    assert lib.vg_trajectory_poses(2, steps.ctypes.data_as(ip), None, a(xi), None) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_trajectory_poses(9, steps.ctypes.data_as(ip), a(p), a(xi), None) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_trajectory_gradient_points(0, a(p), a(out), None) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_trajectory_gradient_points(41, a(p), a(out), None) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_trajectory_gradient_points(10, None, a(out), None) == capi.ERR_INVALID_ARGUMENT


def test_the_wrapper_checks_its_arguments_without_the_library(scene):
    from visgeom_amd import trajectory

    with pytest.raises(ValueError, match="trajectories"):
        trajectory.trajectory_poses(np.zeros(45), [3] * 9)
    with pytest.raises(ValueError, match=r"\[2, 256\]"):
        trajectory.trajectory_poses(np.zeros(5), [1])
    with pytest.raises(ValueError, match="10 values"):
        trajectory.trajectory_poses(np.zeros(9), [4, 7])
    with pytest.raises(ValueError, match="prior_variance must have 6"):
        trajectory.make_quality(dict(scene["q"], prior_variance=[1., 2.]))


def test_poses_match_the_restatement(lib, scene):
    """the integrated trajectories and their covariances to 1e-12 of the largest entry; a long trajectory and a straight one
    (alpha = 0, the first-order branches of the rotation code) besides the scene's two"""
    from visgeom_amd import trajectory

    cases = [(scene["start"], scene["steps"]), ([0.3, -0.2, 0.4, 0.05, 0.03, 1., 2., -3., 0.2, 0.], [256, 5]),
             ([0., 0., 0., 0.1, -0.25] * 3, [2, 3, 30])]
    for params, steps in cases:
        xi, cov = trajectory.trajectory_poses(params, steps)
        o = 0
        for t, n in enumerate(steps):
            rxi, rcov = tr.trajectory(np.asarray(params)[5 * t:5 * t + 5], n, np.longdouble)
            assert np.abs(xi[o:o + n] - rxi).max() <= 1e-12 * np.abs(rxi).max(), (steps, t)
            assert np.abs(cov[o:o + n] - rcov).max() <= 1e-12 * np.abs(rcov).max(), (steps, t)
            assert np.array_equal(cov[o], np.eye(6) * 1e-2)
            o += n
        assert o == xi.shape[0]


def test_the_points_of_a_gradient_are_exact(lib, scene):
    """p + delta and p - delta bit for bit, delta = max(|p| 1e-8, 1e-16); zero and tiny parameters take the floor"""
    from visgeom_amd import trajectory

    for p in (scene["start"], np.array([0., 1e-9, -1e-7, 3., -2.5e5]), np.arange(1., 41.) / 7):
        pts, delta = trajectory.gradient_points(p)
        ref_pts, ref_delta = tr.Quality.gradient_points(None, p)
        assert pts.shape == (2 * p.size + 1, p.size)
        assert np.array_equal(pts[0], p) and np.array_equal(delta, ref_delta) and np.array_equal(pts[1:], ref_pts)
        for i in range(p.size):
            assert pts[1 + 2 * i, i] == p[i] + delta[i] and pts[2 + 2 * i, i] == p[i] - delta[i]
            assert np.array_equal(np.delete(pts[1 + 2 * i], i), np.delete(p, i))
        assert delta[p == 0.].tolist() == [1e-8 * 1e-8] * int((p == 0.).sum())   # DIFF_EPS * DIFF_EPS as the reference forms it


def test_the_scene_is_what_the_gpu_tests_take_it_for(scene):
    """the restatement on the scene: all 9 poses valid, trajectory 1 without an active penalty, trajectory 2 with the curvature
    penalty in all 6 poses and the image limits in the last two; the condition numbers behind the visual_cov bound; the float64 /
    long-double spread of the cost"""
    Q = tr.Quality(scene["cam"], scene["w"], scene["h"], scene["q"], scene["steps"])
    cost, terms, invalid, poses = Q.evaluate(scene["start"], detail=True)
    print("cost %.10f terms %s" % (cost, terms))
    assert invalid == 0 and len(poses) == 9
    assert abs(cost - 936.45764055) < 1e-7 and abs(terms[1:].sum() - 970.33220547) < 1e-7 and abs(terms[0] + 33.87456492) < 1e-7
    for p in poses[:3]:
        assert p["penalties"] == [0., 0., 0., 0.]
    for k, p in enumerate(poses[3:]):
        assert abs(p["penalties"][1] - 100.) < 1e-9 and p["penalties"][2] == p["penalties"][3] == 0.
        assert (p["penalties"][0] > 0.) == (k >= 4)
    conds = [np.linalg.cond(p["JtCJ"]) for p in poses]
    assert 7e4 < min(conds) and max(conds) < 4e5 and all(2. < np.linalg.cond(p["C"]) < 3. for p in poses)
    QL = tr.Quality(scene["cam"], scene["w"], scene["h"], scene["q"], scene["steps"], np.longdouble)
    spread = abs(float(QL.evaluate(scene["start"])[0]) - cost) / abs(cost)
    print("float64 / long double spread of the cost: %.3g" % spread)
    assert spread < 1e-14


@pytest.fixture(scope="module")
def bfgs_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bfgs") / "bfgs_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "host", "bfgs_check.cpp"), "-o", exe])
    return exe


def test_bfgs_finds_the_minimum_of_rosenbrock_through_failed_trials(bfgs_check):
    """10 dimensions from (-1.2, 1, ...), +inf outside |x| <= 3, gradient tolerance 1e-8: the run stops on that tolerance.  The
    smallest eigenvalue of the Hessian at the minimum is about 0.4, so |x - 1| <= |g| / 0.4 to first order: far below 1e-6."""
    r = subprocess.run([bfgs_check, "10", "1e-8"], stdout=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stdout.decode()
    head, xs = r.stdout.decode().strip().split("\n")
    term, iterations, failed, evaluations, cost, err, gmax = head.split()
    print(head)
    assert int(term) == 1                              # VG_TERM_CONVERGENCE_GRADIENT
    assert float(gmax) <= 1e-8 and float(err) <= 1e-6 and float(cost) < 1e-12
    assert int(failed) >= 1                            # the wall was met on the way
    assert 1 <= int(iterations) < 1000 and int(evaluations) <= 21 * int(iterations) + 1
    assert np.abs(np.array([float(v) for v in xs.split()]) - 1.).max() == float(err)


def test_bfgs_stops_at_its_cap_and_solves_the_two_dimensional_case(bfgs_check):
    r = subprocess.run([bfgs_check, "10", "1e-8", "3"], stdout=subprocess.PIPE, timeout=60)
    term, iterations = r.stdout.decode().split()[:2]
    assert r.returncode == 0 and int(term) == 3 and int(iterations) == 3   # VG_TERM_NO_CONVERGENCE
    r = subprocess.run([bfgs_check, "2", "1e-8"], stdout=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and int(r.stdout.decode().split()[0]) == 1
