"""The photometric restatement (tests/photometric_ref.py) against hand-worked values and its own finite differences, the
conditions the GPU tests' scene has to meet, and the new symbols of the C ABI.  No GPU."""
import os
import re

import numpy as np

from tests import photometric_ref as pr
from tests import photometric_scene as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vg_photometric_create", "vg_photometric_destroy", "vg_photometric_level_size", "vg_photometric_set_base",
           "vg_photometric_set_targets", "vg_photometric_level", "vg_photometric_pack", "vg_photometric_evaluate",
           "vg_photometric_compute_pose")


def test_pyramid_by_hand():
    """5 rows x 4 columns -> 2 x 2: source row v goes to min(round(v / 2.), 1) = 0, 1, 1, 1, 1 (the last row takes rows 1 to 4:
    the odd size and the clamp), source column u to u / 2 = 0, 0, 1, 1"""
    img = np.arange(20, dtype=np.uint8).reshape(5, 4) * 3
    lv = pr.pyramid(img, 2, gradients=False)
    a = img.astype(float)
    want = np.array([[a[0, 0] + a[0, 1], a[0, 2] + a[0, 3]],
                     [a[1:, 0].sum() + a[1:, 1].sum(), a[1:, 2].sum() + a[1:, 3].sum()]]) * 0.25
    assert want.tolist() == [[0.75, 3.75], [63.0, 75.0]]   # 3 (0 + 1) / 4, 3 (2 + 3) / 4, 3 * 84 / 4, 3 * 100 / 4
    assert lv[1][0].dtype == np.float32 and lv[1][0].tolist() == want.tolist()
    # an odd width: the last column takes three sources
    img = np.arange(15, dtype=np.uint8).reshape(3, 5)
    got = pr.pyramid(img, 2, gradients=False)[1][0]
    assert got.shape == (1, 2)
    assert got.tolist() == [[(0 + 1 + 5 + 6 + 10 + 11) * 0.25, (2 + 3 + 4 + 7 + 8 + 9 + 12 + 13 + 14) * 0.25]]


def test_sobel_by_hand():
    img = np.array([[1, 2, 4], [3, 7, 5], [9, 6, 8]], np.float32)
    gu, gv = pr.sobel(img)
    # centre: [1 2 1] across rows of the column differences, / 8
    assert gu[1, 1] == ((4 - 1) + 2 * (5 - 3) + (8 - 9)) / 8. and gv[1, 1] == ((9 - 1) + 2 * (6 - 2) + (8 - 4)) / 8.
    # BORDER_REFLECT_101: column -1 is column 1, so the u difference vanishes on the left border; row -1 is row 1
    assert gu[1, 0] == 0. and gv[0, 1] == 0.
    assert gv[1, 0] == ((6 - 2) + 2 * (9 - 1) + (6 - 2)) / 8.


def test_bicubic_reproduces_a_bicubic_polynomial():
    """Catmull-Rom reproduces cubics: f(r, c) = sum a_ij r^i c^j, i, j <= 2 (exact in float32 on the grid), away from the border"""
    rr, cc = np.mgrid[0:12, 0:14].astype(float)
    coef = np.array([[3., 0.5, -0.25], [1., -0.125, 0.0625], [0.5, 0.25, -0.03125]])
    f = lambda r, c: sum(coef[i, j] * r ** i * c ** j for i in range(3) for j in range(3))
    img = f(rr, cc).astype(np.float32)
    assert (img.astype(float) == f(rr, cc)).all()
    rnd = np.random.default_rng(3)
    r, c = rnd.uniform(2., 9., 200), rnd.uniform(2., 11., 200)
    val, dr, dc = pr.bicubic(img, r, c)
    dfdr = sum(coef[i, j] * i * r ** max(i - 1, 0) * c ** j for i in range(1, 3) for j in range(3))
    dfdc = sum(coef[i, j] * j * r ** i * c ** max(j - 1, 0) for i in range(3) for j in range(1, 3))
    scale = np.abs(f(r, c)).max()
    assert np.abs(val - f(r, c)).max() <= 1e-12 * scale
    assert np.abs(dr - dfdr).max() <= 1e-12 * scale and np.abs(dc - dfdc).max() <= 1e-12 * scale


def test_bicubic_clamps_at_the_border():
    img = np.arange(12, dtype=np.float32).reshape(3, 4)
    val, _, _ = pr.bicubic(img, np.array([0.]), np.array([0.]))
    assert val[0] == 0.   # row -1 and column -1 are row 0 and column 0; at an integer position the spline returns the sample


def test_jacobian_matches_central_differences():
    """the analytic rows against central differences of the restatement's own residual, at points that stay strictly inside
    one pixel cell and inside the interior for both displaced poses"""
    loc = ps.localizer()
    xi = np.array(ps.start_pose(0))
    h = 1e-7   # truncation h^2 f''' / 6 and rounding 1e-16 |r| / h both stay below 1e-6 of the largest row entry
    for scale in range(ps.NUM_SCALES):
        e0 = loc.evaluate(scale, xi, 0)
        num = np.zeros_like(e0["jac"])
        sc = float(1 << scale)
        ok = e0["state"] == 0
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            ep, em = loc.evaluate(scale, xi + d, 0, want_jac=False), loc.evaluate(scale, xi - d, 0, want_jac=False)
            num[:, k] = (ep["res"] - em["res"]) / (2 * h)
            for e in (ep, em):   # same cell, same branch
                ok &= (e["state"] == 0) & (np.floor(e["u"] / sc) == np.floor(e0["u"] / sc)) & (np.floor(e["v"] / sc) == np.floor(e0["v"] / sc))
        # the residual is C1 across cells but its second derivative jumps: stay 1e-3 px away from the cell borders
        fu, fv = e0["u"] / sc - np.floor(e0["u"] / sc), e0["v"] / sc - np.floor(e0["v"] / sc)
        ok &= (np.minimum(fu, 1 - fu) > 1e-3) & (np.minimum(fv, 1 - fv) > 1e-3)
        # lossFunction cuts exp(-|x| / 3) to 0 at |x| = 15: a jump of 0.002 in the residual; and its rows vanish beyond
        ok &= np.abs(e0["err"]) < 15. - 1e-2
        assert ok.sum() >= 100
        err = np.abs(num[ok] - e0["jac"][ok]).max()
        assert err <= 1e-6 * np.abs(e0["jac"][ok]).max(), (scale, err)


def test_scene_conditions():
    loc = ps.localizer()
    poses, targets = ps.eval_poses()
    for scale in range(ps.NUM_SCALES):
        pack = loc.packs[scale]
        assert len(pack["idx"]) >= 200
        assert pack["dropped_depth"] >= 1   # a gradient pixel fails DIST_MAX or OUT_OF_RANGE
        assert (np.diff(pack["idx"]) > 0).all()   # raster order
        frac = (loc.evaluate(scale, ps.start_pose(0), 0, want_jac=False)["state"] == 2).mean()
        assert 0.1 <= frac <= 0.9, frac
        for xi, k in zip(poses, targets):   # the evaluate test's poses stay under its cap of left-out points without any
            assert near_boundary(loc, scale, loc.evaluate(scale, xi, int(k), want_jac=False)).mean() <= 0.005


def near_boundary(loc, scale, e, tol=1e-9):
    """points whose projection lies within tol px (level pixels) of a pixel boundary or a margin edge"""
    sc = float(1 << scale)
    h, w = loc.targets[0][scale][0].shape
    u, v, m = e["u"] / sc, e["v"] / sc, pr.MARGIN_PIXELS / sc
    near = (np.abs(u - np.round(u)) < tol) | (np.abs(v - np.round(v)) < tol)
    for edge in (m, w - m - 1):
        near |= np.abs(u - edge) < tol
    for edge in (m, h - m - 1):
        near |= np.abs(v - edge) < tol
    return near


def test_reference_solver_reduces_the_cost_and_the_error():
    x, rep = ps.reference_solve(0)
    loc = ps.localizer()
    assert rep[0]["final_cost"] == loc.cost(0, x, 0) < 0.2 * loc.cost(0, ps.start_pose(0), 0)
    e0, e1 = ps.pose_error(ps.start_pose(0)), ps.pose_error(x)
    assert e1[0] < 0.1 * e0[0] and e1[1] < 0.1 * e0[1]
    assert all(r["iterations"] <= pr.MAX_ITERATIONS for r in rep)


def test_prior_pulls_towards_the_prior():
    x0 = np.array(ps.start_pose(0))
    free, _ = ps.reference_solve(0)
    held, _ = ps.reference_solve(0, prior=True)
    assert np.linalg.norm(held - x0) < np.linalg.norm(free - x0)
    r, J = pr.OdometryPrior(x0).evaluate(x0)
    assert np.abs(r).max() < 1e-12 and np.linalg.matrix_rank(J) == 6


def test_symbols_declared_exported_bound():
    from visgeom_amd import _build, capi

    with open(os.path.join(ROOT, "include", "visgeom_amd.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"\b(vg_photometric_\w+)\s*\(", header))
    assert declared == set(SYMBOLS)
    for name in SYMBOLS:
        assert name in capi.SIGNATURES
    with open(os.path.join(ROOT, "visgeom_amd", "csrc", "vg_photometric_tu.hip")) as fh:
        tu = fh.read()
    for name in SYMBOLS:
        assert re.search(r"^(int|void) %s\(" % name, tu, re.M), name
    assert os.path.join(_build.CSRC, "vg_photometric_tu.hip") in _build.sources()
    L = capi.load()
    for name in SYMBOLS:
        assert hasattr(L, name)
