"""Photometric bundle adjustment without a GPU: the restatement (tests/dense_ba_ref.py) against central differences and on its
own solve case (tests/dense_ba_scene.py), the N-parameter trust-region rule (visgeom_amd/csrc/vg_lmn.hpp) against the
6-parameter one through a stand-alone host program, and the library's refusals, which come before HIP is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import dense_ba_ref as br
from tests import dense_ba_scene as bs
from tests import lm6_ref
from tests import photometric_scene as ps
from tests.test_lm6_cpu import problems, to_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = ctypes.POINTER(ctypes.c_double)


def test_jacobians_against_central_differences():
    """step 1e-6, every pose column of every frame and the depth entry: within 1e-4 of the column's largest entry.  The sampler
    is C1, so a difference across a pixel boundary is off by the step times a jump of the second derivative: a prototype measured
    at most 9.2e-6 (pose) and 3.9e-9 (depth) of the largest entry; the bar leaves a factor of ten."""
    p = bs.problem(2)
    x = bs.start_poses(2)
    d = p.pack["d0"]
    r = p.rows(x, d)
    h = 1e-6
    assert r["ok"].all()
    for f in range(2):
        for c in range(6):
            xp, xm = x.copy(), x.copy()
            xp[f, c] += h
            xm[f, c] -= h
            num = (p.rows(xp, d)["res"][f] - p.rows(xm, d)["res"][f]) / (2. * h)
            err = np.abs(num - r["jp"][f][:, c]).max() / np.abs(r["jp"][f][:, c]).max()
            print("frame", f, "column", c, err)
            assert err <= 1e-4
    num = (p.rows(x, d + h)["res"] - p.rows(x, d - h)["res"]) / (2. * h)
    for f in range(2):
        err = np.abs(num[f] - r["jd"][f]).max() / np.abs(r["jd"][f]).max()
        print("frame", f, "depth", err)
        assert err <= 1e-4
    # one frame's residuals do not depend on another frame's pose
    xp = x.copy()
    xp[1] += 1e-3
    assert (p.rows(xp, d)["res"][0] == r["res"][0]).all()


def test_normal_equations_of_the_restatement():
    """S and rhs of the eliminated system against the full (K + m) x (K + m) damped normal equations, solved densely on a cut-down
    pack; the back-substitution gives the same step"""
    p = bs.exact(65)
    r = p.rows(bs.start_poses(2))
    F, m = r["res"].shape
    K = 6 * F
    J = np.zeros((F * m + m, K + m))
    res = np.concatenate([r["res"].ravel(), r["p"]])
    for f in range(F):
        J[f * m:(f + 1) * m, 6 * f:6 * f + 6] = r["jp"][f]
        J[f * m + np.arange(m), K + np.arange(m)] = r["jd"][f]
    J[F * m + np.arange(m), K + np.arange(m)] = p.prior_scale
    assert abs(0.5 * float(res @ res) - r["cost"]) <= 1e-12 * r["cost"]
    for mu in (1e-4, 1.):
        A = J.T @ J
        D = np.clip(np.diag(A), lm6_ref.DIAG_MIN, lm6_ref.DIAG_MAX)
        full = -np.linalg.solve(A + mu * np.diag(D), J.T @ res)
        S, rhs, Dp, _ = p.reduce(r, mu)
        dp = -np.linalg.solve(S, rhs)
        dd, tail = p.back_substitute(r, mu, dp)
        assert np.abs(np.concatenate([dp, dd]) - full).max() <= 1e-9 * np.abs(full).max()
        assert abs(tail[0] - float(D[K:] @ (dd * dd))) <= 1e-12 * tail[0] and abs(tail[1] - float((J.T @ res)[K:] @ dd)) <= 1e-12 * abs(tail[1])


@pytest.mark.parametrize("F", [2, 3])
def test_the_restatement_solves_its_case(F):
    """ends on a tolerance, reduces the cost, the pose errors and the median relative depth error (the prototype of the issue:
    36 .. 56 iterations, function tolerance, 2.8 mm -> 0.1 .. 0.3 mm, 2.1 % -> about 1 %)"""
    p = bs.problem(F)
    x, d, a, rep = bs.reference_solve(F)
    t0, r0, d0 = bs.errors(bs.start_poses(F), p.pack["d0"], p.pack)
    t1, r1, d1 = bs.errors(x, d, p.pack)
    print(F, rep, (t0, r0, d0), (t1, r1, d1))
    assert rep["termination"] in (lm6_ref.TERM_FUNCTION, lm6_ref.TERM_GRADIENT, lm6_ref.TERM_PARAMETER)
    assert 1 <= rep["iterations"] < br.DEFAULTS["max_iterations"]
    assert rep["final_cost"] < rep["initial_cost"] and rep["final_cost"] == p.cost(x, d)
    assert t1 < t0 and r1 < r0 and d1 < d0
    assert (a > 0).all()


def test_the_n_parameter_rule_has_the_bits_of_the_6_parameter_rule(tmp_path):
    """tests/host/lmn_check.cpp on the problems of tests/test_lm6_cpu.py, one per branch of the rule: with m = 0 and F = 1 every
    step, every sum and every verdict of vglmn equals vglm6's bit for bit, and the branches are the ones lm6_ref takes"""
    exe = str(tmp_path / "lmn_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "host", "lmn_check.cpp"), "-o", exe])
    plist = problems()
    r = subprocess.run([exe], input=to_text(plist).encode(), stdout=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stdout.decode()
    rows = [[int(v) for v in line.split()] for line in r.stdout.decode().strip().split("\n")]
    assert len(rows) == len(plist)
    seen = set()
    for prob, (iterations, accepted, term, mismatches) in zip(plist, rows):
        print(prob["name"], iterations, accepted, term, mismatches)
        assert mismatches == 0, prob["name"]
        rule = dict(prob["rule"])
        x, rep = None, None
        with np.errstate(over="ignore", invalid="ignore"):
            from tests.test_lm6_cpu import normal

            x, rep = lm6_ref.solve(lambda v: normal(prob, v), prob["x0"], **rule)
        assert (iterations, term) == (rep["iterations"], rep["termination"]), prob["name"]
        seen.add(term)
    assert seen == {lm6_ref.TERM_FUNCTION, lm6_ref.TERM_GRADIENT, lm6_ref.TERM_PARAMETER, lm6_ref.TERM_NO_CONVERGENCE, lm6_ref.TERM_RADIUS}


def test_the_library_refuses_before_hip_is_touched():
    """no GPU is needed: every check of an argument comes before the device is looked for"""
    from visgeom_amd import _build, capi, stereo

    _build.build()
    L = capi.load()
    cam = np.array(ps.CAM, float)
    xbc = np.array(ps.XI_BASE_CAM, float)
    prm = stereo.make_params(equal_margins=0, **ps.PRM)

    def create(eucm=cam, params=prm, xi=xbc, width=ps.W, height=ps.H, out=True, **opt):
        h = ctypes.c_void_p()
        o = capi.DenseBaOptions(**opt)
        rc = L.vg_dense_ba_create(ctypes.byref(h) if out else None, 0, None, eucm.ctypes.data_as(_dp) if eucm is not None else None,
                                  ctypes.byref(params) if params is not None else None, xi.ctypes.data_as(_dp) if xi is not None else None,
                                  width, height, ctypes.byref(o) if opt else None)
        if h.value:   # a GPU is present and the arguments were good
            L.vg_dense_ba_destroy(h)
        return rc, L.vg_last_error().decode()

    bad = capi.ERR_INVALID_ARGUMENT
    assert create(out=False)[0] == bad
    for k in ("eucm", "params", "xi"):
        assert create(**{k: None}) == (bad, "NULL argument")
    for kw in ({"width": 0}, {"height": 0}, {"width": -3}, {"height": 16385}):
        rc, msg = create(**kw)
        assert rc == bad and "image size" in msg
    empty = stereo.make_params(equal_margins=0, **dict(ps.PRM, x_max=0))
    assert create(params=empty)[0] == bad
    assert create(params=stereo.make_params(equal_margins=0, **dict(ps.PRM, scale=0)))[0] == bad
    rc, msg = create(sigma_grey=-1.)
    assert rc == bad and "sigma_grey" in msg
    assert create(sigma_grey=float("nan"))[0] == bad
    assert create(max_iterations=-1)[0] == bad and create(function_tolerance=-1e-6)[0] == bad
    assert create(eucm=np.array([0.6, 1.05, 0., 125., 128., 96.]))[0] == bad
    # good arguments reach the device: a handle, or the refusal of a machine without a GPU
    rc, msg = create()
    assert rc in (capi.OK, capi.ERR_NO_DEVICE), msg
    # the frame count is checked before the handle
    for F in (0, -1, 9, 1 << 20):
        assert L.vg_dense_ba_set_frames(None, F, None) == bad
        assert "frame count must be in [1, 8]" in L.vg_last_error().decode()
    assert L.vg_dense_ba_set_frames(None, 8, None) == bad and "handle is NULL" in L.vg_last_error().decode()
    assert L.vg_dense_ba_set_base(None, None, None, None) == bad
    assert L.vg_dense_ba_pack(None, None, None, None, None, None, None) == bad
    assert L.vg_dense_ba_evaluate(None, None, None, None, None, None, None, None, None, None) == bad
    assert L.vg_dense_ba_reduce(None, 1., None, None) == bad
    assert L.vg_dense_ba_back_substitute(None, 1., None, None, None) == bad
    assert L.vg_dense_ba_solve(None, None, None, None, None, None) == bad
    L.vg_dense_ba_destroy(None)
