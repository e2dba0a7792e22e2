"""Sparse visual odometry on the GPU (include/visgeom_amd.h section 13) against tests/sparse_odom_ref.py on the scene of
tests/sparse_odom_scene.py.

Integer stages (response, key points, match indices, inlier counts, masks) must be identical.  Descriptors: 1 float ulp (one
rounding of a double product).  Distances: 1e-10 relative, and bit-equal for the minimum and the runner-up of every
nearest-neighbour decision (the sums are exact: tests/test_sparse_odom_cpu.py).  Score residuals: 1e-10 relative, see test_score.

Solve margin: measured on the restatement, per problem, as 100 x its own spread -- its result at the default tolerances against
its result with function and parameter tolerance tightened 100 x and 75 iterations -- with the floor 1e-7
(sparse_odom_scene.solve_margin).  Measured spreads: the 95-point block 8.1e-7 (margin 8.1e-5); the 2- and 3-point
hypotheses from below 1e-9 (margin: the floor) up to 0.58 for samples that hold a wrong pair, whose problems are not settled
after 25 iterations -- for those the margin says only that the result is finite, and tests/test_sparse_odom_cpu.py asserts
that at least half of each table is held to better than 1e-4.  What IS well defined for every problem of a table, settled or
not, is compared as well: the initial cost, and the pose after 3 iterations (test_solve_hypotheses; measured difference
5.2e-14 for the 2-point and 2.0e-13 for the 3-point table, against the floor 1e-7)."""
import ctypes

import numpy as np
import pytest

from tests import sparse_odom_ref as sr
from tests import sparse_odom_scene as sc

pytestmark = pytest.mark.gpu
PARITY = 1e-10


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def make(torch, w=sc.W, h=sc.H, **changes):
    from visgeom_amd import sparse_odom

    return sparse_odom.SparseOdometry(sc.CAM, sc.XI_BASE_CAM, w, h, sparse_odom.default_params(**changes))


def dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def points(torch):
    s = sc.points_set()
    return {k: dev(torch, s[k]) for k in ("x1", "x2", "p2", "size")}


def test_response_bit_equal(torch):
    imgs = sc.images()
    got = make(torch).response(dev(torch, imgs)).cpu().numpy()   # the batch of 3
    for k in range(3):
        assert np.array_equal(got[k], sr.response(imgs[k]))
    one = make(torch).response(dev(torch, imgs[1])).cpu().numpy()
    assert np.array_equal(one[0], got[1])
    rnd = np.random.default_rng(3).integers(0, 256, (101, 150), dtype=np.uint8)
    assert np.array_equal(make(torch, 150, 101).response(dev(torch, rnd)).cpu().numpy()[0], sr.response(rnd))


@pytest.mark.parametrize("max_features", [sc.SMALL_FEATURES, 500])
def test_detect(torch, max_features):
    imgs = sc.images()
    count, kp, desc = make(torch, max_features=max_features).detect(dev(torch, imgs))
    kp, desc = kp.cpu().numpy(), desc.cpu().numpy()
    for k in range(3):
        rkp, n_max, rdesc = sc.detection(k, max_features)
        assert count[k] == min(n_max, max_features) == len(rkp)
        assert np.array_equal(kp[k, :count[k]], rkp)
        ulp = np.spacing(np.abs(rdesc))
        assert (np.abs(desc[k, :count[k]] - rdesc) <= ulp).all()


def test_detect_flat_and_ties(torch):
    flat = np.full((48, 48), 90, np.uint8)
    tile = np.zeros((16, 16), np.uint8)
    tile[5:10, 5:10] = 255
    rep = np.tile(tile, (3, 3))
    count, kp, _ = make(torch, 48, 48).detect(dev(torch, np.stack([flat, rep])))
    rkp, n_max = sr.detect(rep)
    assert count[0] == 0 and count[1] == n_max == len(rkp) and n_max >= 2
    R = sr.response(rep)
    assert len({int(R[v, u]) for u, v in rkp}) < len(rkp)   # the pattern does produce equal responses
    assert np.array_equal(kp.cpu().numpy()[1, :count[1]], rkp)
    # with fewer features than maxima the cut goes through a group of equal responses: the tie rule decides who stays
    few = max(1, n_max - 1)
    c2, kp2, _ = make(torch, 48, 48, max_features=few).detect(dev(torch, rep))
    assert c2[0] == few and np.array_equal(kp2.cpu().numpy()[0, :few], sr.detect(rep, few)[0])


def test_match(torch):
    odo = make(torch)
    sets = [sc.detection(k, 500) for k in range(3)]
    F = 500

    def padded(d):
        out = np.zeros((F, 81), np.float32)
        out[:len(d)] = d
        return out

    d1 = dev(torch, np.stack([padded(sets[0][2]), padded(sets[1][2]), padded(sets[0][2])]))
    d2 = dev(torch, np.stack([padded(sets[1][2]), padded(sets[2][2]), padded(sets[1][2])]))
    c1 = [len(sets[0][0]), len(sets[1][0]), len(sets[0][0])]
    c2 = [len(sets[1][0]), len(sets[2][0]), 0]   # the third pair has an empty side
    mc, matches, dist = odo.match(c1, d1, c2, d2)
    matches, dist = matches.cpu().numpy(), dist.cpu().numpy()
    for k in range(2):
        pairs, rd, _ = sr.match(sets[k][2], sets[k + 1][2])
        assert mc[k] == len(pairs) >= 40
        assert np.array_equal(matches[k, :mc[k]], pairs)
        assert np.allclose(dist[k, :mc[k]], rd, rtol=PARITY, atol=0.)
        assert np.array_equal(dist[k, :mc[k]], rd)   # the sums are exact on both sides
    assert mc[2] == 0
    # the minimum and the runner-up of EVERY nearest-neighbour decision, both directions, bit-equal to the restatement's: one
    # pair of single descriptors per probe, through the same kernel, with the threshold out of the way
    a, b, want = [], [], []
    for k in range(2):
        D = sr.distance_matrix(sets[k][2], sets[k + 1][2])
        for M, first in ((D, True), (D.T, False)):
            two = np.argsort(M, axis=1, kind="stable")[:, :2]
            for i in range(M.shape[0]):
                for j in two[i]:
                    a.append(sets[k][2][i] if first else sets[k][2][j])
                    b.append(sets[k + 1][2][j] if first else sets[k + 1][2][i])
                    want.append(M[i, j])
    n = len(want)
    assert 2000 < n < 65535
    probe = make(torch, max_features=1, match_threshold=1e30)
    one = np.ones(n, np.int32)
    mc1, _, dist1 = probe.match(one, dev(torch, np.stack(a)[:, None, :]), one, dev(torch, np.stack(b)[:, None, :]))
    assert (mc1 == 1).all() and np.array_equal(dist1.cpu().numpy()[:, 0], np.array(want))


def test_score(torch, points):
    """Residuals to 1e-10 relative where finite.  The residual is the difference of an observation of some 200 px and a
    projection through a triangulation whose determinant cancels, so its own FP64 rounding is not 1e-10 of a 0.01 px residual:
    the restatement against itself in extended precision (sparse_odom_ref.score with np.longdouble) differs by up to 8.4e-8 of
    the residual (1.0e-9 px at a residual of 0.012 px; 5 of the 23987 finite entries above 1e-10), and by 9.7e-13 in the
    project's norm-wise metric (tests/parity.py: |difference| / |reference| over the set, here each hypothesis' row).  Both
    are asserted: every row norm-wise to 1e-10, and every single residual to 1e-10 of ITSELF plus 100 x the restatement's own
    rounding error at that entry (the reference's own error: an entry it cannot place, nobody can).  Measured on an MI355X:
    row-wise 7.3e-13; per entry at the most 4.3e-9 of the residual, 6 entries above 1e-10."""
    s, r = sc.points_set(), sc.reference_ransac(2)
    inl, res = make(torch).score(r["hypotheses"], points["x1"], points["x2"], points["p2"])
    res = res.cpu().numpy()
    ref = r["residuals"]
    assert np.isinf(ref).any() and np.array_equal(np.isinf(res), np.isinf(ref))
    fin = np.isfinite(ref)
    assert np.finfo(np.longdouble).eps < 1e-18
    xbc = np.asarray(sc.XI_BASE_CAM, float)
    ext = np.array([sr.score(sc.CAM, xbc, xi, s["x1"], s["x2"], s["p2"], np.longdouble) for xi in r["hypotheses"]])
    with np.errstate(invalid="ignore"):
        own = np.where(fin, np.abs(ext - ref), 0.).astype(np.float64)
        err = np.where(fin, np.abs(res - ref), 0.)
    rows = [np.linalg.norm(err[k]) / np.linalg.norm(ref[k][fin[k]]) for k in range(len(ref))]
    rel = err[fin] / ref[fin]
    print("score: row-wise |res - ref| / |ref| max %.3e; per entry max %.3e (restatement's own %.3e), entries above 1e-10: %d (own %d)"
          % (max(rows), rel.max(), (own[fin] / ref[fin]).max(), (rel > PARITY).sum(), (own[fin] / ref[fin] > PARITY).sum()))
    assert max(rows) <= PARITY
    assert (err[fin] <= PARITY * ref[fin] + 100. * own[fin]).all()
    assert np.array_equal(res < sr.INLIER_THRESHOLD, ref < sr.INLIER_THRESHOLD)
    assert np.array_equal(inl, (ref < sr.INLIER_THRESHOLD).sum(1))
    assert s["x1"].shape[0] == res.shape[1]


@pytest.mark.parametrize("pts", [2, 3])
def test_solve_hypotheses(torch, points, pts):
    s = sc.points_set()
    tab = s["samples%d" % pts].ravel()
    idx = torch.from_numpy(tab.astype(np.int64)).cuda()
    odo = make(torch, num_ransac_points=pts)
    args = [points[k][idx].contiguous() for k in ("x1", "x2", "p2", "size")]
    xi, rep = odo.solve(np.arange(201) * pts, *args, s["xi_odom"])
    ref, margin = sc.hypothesis_solves(pts)
    assert np.isfinite(xi).all() and (rep[:, 0] <= 25).all()
    assert (np.abs(xi - ref).max(1) <= margin).all(), np.abs(xi - ref).max(1)[np.abs(xi - ref).max(1) > margin]
    # every problem, settled after 25 iterations or not: the cost at the start, and the pose after 3 iterations (three
    # decisions of the acceptance and radius rule from the same start; the floor of the margin, relative to the step taken)
    short = sc.short_solves(pts)
    assert np.allclose(rep[:, 1], short["initial_cost"], rtol=PARITY, atol=0.)
    xi3, rep3 = make(torch, num_ransac_points=pts, max_lm_iterations=3).solve(np.arange(201) * pts, *args, s["xi_odom"])
    step = np.maximum(1., np.abs(short["xi"] - s["xi_odom"]).max(1))
    d3 = np.abs(xi3 - short["xi"]).max(1) / step
    print("solve %d points: pose after 3 iterations, max difference %.3e" % (pts, d3.max()))
    assert (rep3[:, 0] == short["iterations"]).all() and (d3 <= sc.SOLVE_FLOOR).all(), d3[d3 > sc.SOLVE_FLOOR]
    assert (rep[:, 2] <= rep[:, 1]).all()   # no accepted step raises the cost
    # one block alone gives the bits it has inside the batch
    for b in (0, 57, 199):
        one, rep1 = odo.solve([0, pts], *[a[b * pts:(b + 1) * pts].contiguous() for a in args], s["xi_odom"])
        assert np.array_equal(one[0], xi[b]) and np.array_equal(rep1[0], rep[b])


def test_solve_block_of_95(torch, points):
    s = sc.points_set()
    sel = sc.clean_block()
    idx = torch.from_numpy(sel).cuda()
    args = [points[k][idx].contiguous() for k in ("x1", "x2", "p2", "size")]
    xi, rep = make(torch).solve([0, len(sel)], *args, s["xi_odom"])
    ref, margin = sc.solve_margin(s["x1"][sel], s["x2"][sel], s["p2"][sel], s["size"][sel], s["xi_odom"], key="block95")
    assert np.abs(xi[0] - ref).max() <= margin, (xi[0] - ref, margin)
    assert rep[0, 2] < rep[0, 1]


def test_solve_without_iterations(torch, points):
    """max_lm_iterations = 0: the start is evaluated and returned"""
    s = sc.points_set()
    idx = torch.from_numpy(s["samples2"][0].astype(np.int64)).cuda()
    args = [points[k][idx].contiguous() for k in ("x1", "x2", "p2", "size")]
    xi, rep = make(torch, max_lm_iterations=0).solve([0, 2], *args, s["xi_odom"])
    assert np.array_equal(xi[0], np.asarray(s["xi_odom"], float))
    assert rep[0, 0] == 0 and rep[0, 2] == rep[0, 1] > 0. and rep[0, 3] == sr.pr.TERM_NO_CONVERGENCE


def test_solve_empty_block_between_two(torch, points):
    """offsets [0, 2, 2, 4]: the middle block has the prior alone, and its neighbours do not notice it"""
    s = sc.points_set()
    idx = torch.from_numpy(s["samples2"][:2].ravel().astype(np.int64)).cuda()
    args = [points[k][idx].contiguous() for k in ("x1", "x2", "p2", "size")]
    odo = make(torch)
    xi, rep = odo.solve([0, 2, 2, 4], *args, s["xi_odom"])
    ref, ref_rep = sr.solve(sc.CAM, sc.XI_BASE_CAM, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0), s["xi_odom"])
    assert np.array_equal(xi[1], ref) and rep[1, 0] == ref_rep["iterations"] and rep[1, 3] == ref_rep["termination"]
    for b, block in ((0, 0), (1, 2)):
        one, rep1 = odo.solve([0, 2], *[a[2 * b:2 * b + 2].contiguous() for a in args], s["xi_odom"])
        assert np.array_equal(one[0], xi[block]) and np.array_equal(rep1[0], rep[block])


def test_ransac(torch, points):
    s, r = sc.points_set(), sc.reference_ransac(2)
    xi, mask, rep = make(torch).ransac(points["x1"], points["x2"], points["p2"], points["size"], s["xi_odom"], s["samples2"])
    assert (rep["status"], rep["best"], rep["inliers"], rep["kept"]) == (sr.STATUS_OK, r["best"], r["inliers"], r["kept"])
    assert np.array_equal(mask.cpu().numpy().astype(bool), r["mask"])
    sel = np.flatnonzero(r["mask"])[r["gate_err"] < r["gate_bound"]]
    _, margin = sc.solve_margin(s["x1"][sel], s["x2"][sel], s["p2"][sel], s["size"][sel], s["xi_odom"], key="ransac_final")
    assert np.abs(xi - r["xi_incr"]).max() <= margin
    # fewer matches than points per hypothesis: the odometry increment, and the report says so
    xi, mask, rep = make(torch).ransac(points["x1"][:1], points["x2"][:1], points["p2"][:1], points["size"][:1], s["xi_odom"])
    assert rep["status"] == sr.STATUS_TOO_FEW and np.array_equal(xi, s["xi_odom"]) and not mask.any()


def test_own_draw(torch, points):
    """the documented generator against its restatement, and ransac / feed with samples = None"""
    s = sc.points_set()
    odo, ref = make(torch), sr.Draw()
    for m in (120, 120, 7, 2):   # the index vector persists while m stays the same and starts again when it changes
        tab, want = odo.draw_samples(m), ref.table(m)
        assert np.array_equal(tab, want)
        assert tab.min() >= 0 and tab.max() < m and (tab[:, 0] != tab[:, 1]).all()
    three = make(torch, num_ransac_points=3).draw_samples(5)
    assert np.array_equal(three, sr.Draw().table(5, points=3)) and all(len(set(row)) == 3 for row in three.tolist())
    # a fresh handle draws the first table itself: the same as being given it
    table = sr.Draw().table(120)
    xi_a, mask_a, rep_a = make(torch).ransac(points["x1"], points["x2"], points["p2"], points["size"], s["xi_odom"])
    xi_b, mask_b, rep_b = make(torch).ransac(points["x1"], points["x2"], points["p2"], points["size"], s["xi_odom"], table)
    assert rep_a == rep_b and np.array_equal(xi_a, xi_b) and bool((mask_a == mask_b).all())
    assert rep_a["status"] == sr.STATUS_OK and rep_a["inliers"] >= 80
    odo = make(torch)
    states = [odo.feed(dev(torch, img), xi)[1]["state"] for img, xi in zip(sc.images(), sc.odometry_poses())]
    assert states == sc.reference_feed()["states"] and np.isfinite(odo.integrated).all() and np.abs(odo.integrated).max() > 0.


def test_refusals_behind_the_handle(torch, points):
    """what section 13's entries refuse once they have a handle; every one returns before anything is launched"""
    from visgeom_amd import capi

    lib = capi.load()
    odo = make(torch, max_features=64)
    h, bad = odo._h, capi.ERR_INVALID_ARGUMENT
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    D = lambda a: a.ctypes.data_as(dp)
    I = lambda a: a.ctypes.data_as(ip)
    x1, x2, p2, size = (points[k].data_ptr() for k in ("x1", "x2", "p2", "size"))
    m = 120
    six, nan6, inf6 = np.array(sc.points_set()["xi_odom"]), np.full(6, np.nan), np.array([0., 0., np.inf, 0., 0., 0.])
    out, rep = np.zeros(12), np.zeros(16)
    img = dev(torch, sc.images()[0])
    i64 = torch.zeros((sc.H, sc.W), dtype=torch.int64, device="cuda")
    cnt = np.zeros(4, np.int32)
    # sizes
    assert lib.vg_sparse_odom_response(h, 0, img.data_ptr(), i64.data_ptr()) == bad
    assert lib.vg_sparse_odom_response(h, 65536, img.data_ptr(), i64.data_ptr()) == bad
    assert lib.vg_sparse_odom_response(h, 1, None, i64.data_ptr()) == bad and lib.vg_sparse_odom_response(h, 1, img.data_ptr(), None) == bad
    assert lib.vg_sparse_odom_detect(h, 0, img.data_ptr(), I(cnt), i64.data_ptr(), i64.data_ptr()) == bad
    assert lib.vg_sparse_odom_detect(h, 1, img.data_ptr(), None, i64.data_ptr(), i64.data_ptr()) == bad
    desc = torch.zeros((1, 64, 81), dtype=torch.float32, device="cuda")
    mt = torch.zeros((1, 64, 2), dtype=torch.int32, device="cuda")
    ds = torch.zeros((1, 64), dtype=torch.float64, device="cuda")
    for c1, c2 in ((65, 3), (3, 65), (-1, 3), (3, -1)):   # counts above max_features, negative counts
        a, b = np.array([c1], np.int32), np.array([c2], np.int32)
        assert lib.vg_sparse_odom_match(h, 1, I(a), desc.data_ptr(), I(b), desc.data_ptr(), I(cnt), mt.data_ptr(), ds.data_ptr()) == bad, (c1, c2)
    a = np.array([3], np.int32)
    assert lib.vg_sparse_odom_match(h, 0, I(a), desc.data_ptr(), I(a), desc.data_ptr(), I(cnt), mt.data_ptr(), ds.data_ptr()) == bad
    assert lib.vg_sparse_odom_match(h, 1, I(a), desc.data_ptr(), I(a), None, I(cnt), mt.data_ptr(), ds.data_ptr()) == bad

    def solve(n, offsets, xi=six, xo=out):
        off = np.array(offsets, np.int64)
        return lib.vg_sparse_odom_solve(h, n, off.ctypes.data_as(lp), x1, x2, p2, size, D(xi), D(xo) if xo is not None else None, D(rep))

    assert solve(0, [0, 2]) == bad                      # n < 1
    assert solve(2, [1, 2, 4]) == bad                   # offsets[0] != 0
    assert solve(2, [0, 4, 2]) == bad                   # decreasing offsets
    assert solve(1, [0, (1 << 20) + 1]) == bad          # too many points
    assert solve(1, [0, 2], xi=nan6) == bad and solve(1, [0, 2], xi=inf6) == bad
    assert solve(1, [0, 2], xo=None) == bad
    assert lib.vg_sparse_odom_solve(h, 1, np.array([0, 2], np.int64).ctypes.data_as(lp), None, x2, p2, size, D(six), D(out), D(rep)) == bad
    assert solve(1, [0, 2]) == capi.OK                  # the same call with nothing wrong is taken

    def score(n, xi, mm=m, a=x1):
        return lib.vg_sparse_odom_score(h, n, D(xi), mm, a, x2, p2, None, I(cnt))

    two = np.stack([six, six])
    assert score(0, two) == bad and score(2, two, mm=-1) == bad and score(2, two, a=None) == bad
    twobad = two.copy()
    twobad[1, 4] = np.nan                               # the second pose: every pose is looked at
    assert score(2, twobad) == bad
    assert score(2, two) == capi.OK

    def ransac(samples, xi=six, mm=m, a=x1):
        return lib.vg_sparse_odom_ransac(h, mm, a, x2, p2, size, D(xi), I(samples) if samples is not None else None, D(out), None, D(rep))

    good = sc.points_set()["samples2"].copy()
    assert ransac(good, xi=nan6) == bad and ransac(good, mm=-1) == bad and ransac(good, a=None) == bad
    for row, value in ((0, m), (199, m), (57, -1), (3, 2 ** 31 - 1)):   # sample index out of range: first and last row, below and above
        t = good.copy()
        t[row, 1] = value
        assert ransac(t) == bad, (row, value)
        assert b"sample index" in lib.vg_last_error()
    assert ransac(good) == capi.OK

    assert lib.vg_sparse_odom_draw_samples(h, 1, I(good)) == bad and lib.vg_sparse_odom_draw_samples(h, m, None) == bad
    assert lib.vg_sparse_odom_draw_samples(h, (1 << 20) + 1, I(good)) == bad

    def feed(xi, samples=None, im=img.data_ptr()):
        return lib.vg_sparse_odom_feed(h, im, D(xi), I(samples) if samples is not None else None, D(out), D(rep))

    t = good.copy()
    t[199, 1] = -1
    assert feed(nan6) == bad and feed(inf6) == bad and feed(np.zeros(6), im=None) == bad and feed(np.zeros(6), samples=t) == bad
    assert lib.vg_sparse_odom_feed(h, img.data_ptr(), None, None, D(out), D(rep)) == bad
    assert lib.vg_sparse_odom_increment(h, None) == bad and lib.vg_sparse_odom_integrated(h, None) == bad
    # a refused feed left no frame behind: the next one is the first
    assert feed(np.zeros(6)) == capi.OK and rep[0] == sr.STATE_FIRST


def run_feed(torch, **changes):
    odo = make(torch, **changes)
    out = []
    for img, xi in zip(sc.images(), sc.odometry_poses()):
        incr, rep = odo.feed(dev(torch, img), xi, sc.points_set()["samples2"])
        out.append((incr, rep, odo.integrated))
    return out


def test_feed(torch):
    f = sc.reference_feed()
    got = run_feed(torch)
    assert [g[1]["state"] for g in got] == f["states"]
    total = 0.
    truth = sc.true_poses()
    for k, log in enumerate(f["odo"].log):
        incr, rep, integ = got[k + 1]
        r = log["ransac"]
        assert (rep["matches"], rep["best"], rep["inliers"], rep["kept"]) == (len(log["pairs"]), r["best"], r["inliers"], r["kept"])
        x1, x2, p2, size = sr.rays(sc.CAM, log["kp1"], log["kp2"], log["pairs"])
        sel = np.flatnonzero(r["mask"])[r["gate_err"] < r["gate_bound"]]
        incr_odom = sr.pr.inverse_compose(sc.odometry_poses()[k], sc.odometry_poses()[k + 1])
        _, margin = sc.solve_margin(x1[sel], x2[sel], p2[sel], size[sel], incr_odom, key=("feed_final", k))
        total += margin
        assert np.abs(incr - f["increments"][k + 1]).max() <= margin
        assert np.abs(integ - f["integrated"][k + 1]).max() <= 2. * total   # composed increments: rotation couples into translation
        for got_xi, ref_xi in ((integ, f["integrated"][k + 1]),):
            eg, er = sc.pose_error(got_xi, truth[k + 1]), sc.pose_error(ref_xi, truth[k + 1])
            assert eg[0] <= er[0] + 2. * total and eg[1] <= er[1] + 2. * total
    again = run_feed(torch)
    for a, b in zip(got, again):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


def test_feed_skip_rule(torch):
    got = run_feed(torch, min_stereo_base=1.)   # above the 0.15 m steps
    assert [g[1]["state"] for g in got] == [sr.STATE_FIRST, sr.STATE_SKIPPED, sr.STATE_SKIPPED]
    assert all(np.array_equal(g[0], np.zeros(6)) and np.array_equal(g[2], np.zeros(6)) for g in got)
    # a skipped frame leaves the state untouched: with the base between one step and two, the second frame is skipped and
    # the third is estimated against the FIRST -- the bits of a handle that never saw the second frame
    odom, xbc = sc.odometry_poses(), np.asarray(sc.XI_BASE_CAM, float)
    base = [np.linalg.norm(sr.camera_motion(xbc, sr.pr.inverse_compose(odom[a], odom[b]))[:3]) for a, b in ((0, 1), (0, 2))]
    assert base[0] < 0.22 < base[1]
    got = run_feed(torch, min_stereo_base=0.22)
    assert [g[1]["state"] for g in got] == [sr.STATE_FIRST, sr.STATE_SKIPPED, sr.STATE_ESTIMATED]
    assert np.array_equal(got[1][0], np.zeros(6)) and np.array_equal(got[1][2], np.zeros(6))
    odo = make(torch)
    imgs, table = sc.images(), sc.points_set()["samples2"]
    odo.feed(dev(torch, imgs[0]), odom[0], table)
    incr, rep = odo.feed(dev(torch, imgs[2]), odom[2], table)
    assert rep["state"] == sr.STATE_ESTIMATED and rep["matches"] >= 2 and np.abs(incr).max() > 0.
    assert rep == got[2][1] and np.array_equal(incr, got[2][0]) and np.array_equal(odo.integrated, got[2][2])
