"""Sparse visual odometry on the GPU (include/visgeom_amd.h section 13) against tests/sparse_odom_ref.py on the cases of
tests/sparse_odom_shapes.py: the feature, match and point counts at which the kernels of vg_sparse_odom.hpp take the paths that
the scene of tests/test_gpu_sparse_odom.py leaves out.  tests/test_sparse_odom_shapes_cpu.py shows that each case is live.

The comparison rules are those of tests/test_gpu_sparse_odom.py, stage by stage, and no tolerance is new: integer outputs
(response, key points, counts, match pairs, inlier counts, masks, statuses) identical; descriptors within 1 float ulp; distances
bit-equal (the sums are exact: the CPU module asserts two other summation orders for every descriptor set used here); score
residuals row-wise 1e-10 and per entry 1e-10 of itself plus 100 x the restatement's own long-double error; solves within
sparse_odom_scene.solve_margin, the initial cost within 1e-10 relative, the pose after 3 iterations within SOLVE_FLOOR of the step.

The mistakes each case is there to catch, by reading the kernels against the cases:
  select_kernel's candidate loops stop after one trip      many_candidates (1889 and 2013 maxima), the batch of three
  a selected key lost at max_features = kMaxFeatures       many_candidates at 1024 and 1023
  a digit of the index half of the radix key ignored       wide_index_ties (one response, indices to 74231), wide_index_ties_cut
                                                           (the cut between indices 65543 and 65527)
  the response compared on its raw bits                    negative_responses (441 positive, 312 negative maxima, cut at 597 and none)
  a border or a capacity off by one on the smallest image  min_image: 15 x 15, 15 x 41 and 41 x 15
  the batch's largest counts taken for a pair's own        count_edges; tile (16) and wave (64) edges of distance and compaction
  <= for < in the nearest-neighbour search                 nearest_tie, either side
  >= for > in the threshold test                           threshold_equal: at the distance, one double below, and zero
  inliers counted by the first block of a hypothesis only  score_blocks (m to 1000), ransac_limits big, feed_many_matches
  lanes of the solve beyond the block's size               solve_sizes: 1, 63, 64, 65, 128, 129, 1000, 0, 2 in one call
  an aligned 16-byte load of the caller's p2 or x1         test_solve_unaligned_points
  scratch kept from a larger call                          handle_reuse

Measured on an MI355X (every integer output, every descriptor and every distance as the rule demands; no kernel was found wrong):
  score residuals, m = 1 .. 1000   row-wise at the most 1.1e-13 (m = 1), 3.7e-15 at m = 1000; per entry at the most 4.0e-11 of the
                                   residual where the restatement's own error reaches 2.7e-10; no entry above 1e-10
  solve_sizes                      difference / margin at the most 3.9e-12 (margins 1e-7 .. 2.4e-4, 3 or 4 iterations, 1 for the
                                   empty block); pose after 3 iterations at the most 9.5e-17 of the step, against the floor 1e-7
  ransac_limits                    increment off by 1.1e-16 (big, margin 2.1e-4), 9.6e-17 (sixteen_17, 4.6e-5), 7.2e-17
                                   (one_iteration, 1e-7); bit-equal to solve() on the kept points in all three
  feed_many_matches                1013 matches, 1013 inliers, 925 kept; increment off by 1.5e-16 against the margin 1e-7
Each of these value-only changes to vg_sparse_odom.hpp failed the tests named, and none but the fourth failed
tests/test_gpu_sparse_odom.py (its test_feed):
  select_kernel's two candidate loops end after one trip   test_detect[many], test_detect_batch_of_unequal_lists, test_feed_many_matches
  index bits 16 .. 23 masked out of the radix passes       test_detect[ties], test_detect[ties_cut]
  bias = 0                                                 test_detect[signs]
  score_kernel adds its ballot only in block 0             test_score_blocks[1000], test_ransac_limits[big], test_feed_many_matches
  nearest_kernel with d <= bd                              test_match_nearest_tie[1], [2]
  cross_check_kernel with !(d >= threshold)                test_match_threshold_equal"""
import numpy as np
import pytest

from tests import sparse_odom_ref as sr
from tests import sparse_odom_scene as sc
from tests import sparse_odom_shapes as ss

pytestmark = pytest.mark.gpu
PARITY = 1e-10
REPORT_WITHOUT_HYPOTHESIS = {"best": -1, "inliers": 0, "kept": 0, "refine_cost": 0., "refine_termination": sr.pr.TERM_NO_CONVERGENCE,
                             "final_cost": 0., "final_termination": sr.pr.TERM_NO_CONVERGENCE, "status": sr.STATUS_NO_HYPOTHESIS}


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def make(torch, w=sc.W, h=sc.H, **changes):
    from visgeom_amd import sparse_odom

    return sparse_odom.SparseOdometry(ss.CAM, ss.XBC, w, h, sparse_odom.default_params(**changes))


def dev(torch, a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True)).cuda()   # the inputs are frozen: torch wants a writable array
    return t if dtype is None else t.to(dtype)


def assert_detection(count, kp, desc, name, f):
    """one image's key points and descriptors against the restatement at max_features = f"""
    rkp, n_max, rdesc = ss.detection(name, f)
    assert count == min(n_max, f) == len(rkp)
    assert np.array_equal(kp[:count], rkp), "%s at %d: first difference at feature %d" % (name, f, int(np.flatnonzero((kp[:count] != rkp).any(1))[0]))
    assert (np.abs(desc[:count] - rdesc) <= np.spacing(np.abs(rdesc))).all()


# ---- detection -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ss.DETECT_IMAGES)
def test_detect(torch, name):
    img = ss.image(name)
    h, w = img.shape
    for f in ss.detect_features(name):
        count, kp, desc = make(torch, w, h, max_features=f).detect(dev(torch, img))
        print(name, "%d x %d" % (w, h), "max_features", f, "count", int(count[0]), "of", ss.detection(name, f)[1], "maxima")
        assert_detection(int(count[0]), kp.cpu().numpy()[0], desc.cpu().numpy()[0], name, f)
    if min(h, w) == 15:   # the smallest sides: the response as well
        assert np.array_equal(make(torch, w, h).response(dev(torch, img)).cpu().numpy()[0], ss.response(name))


@pytest.mark.parametrize("f", [ss.MAX, 64])
def test_detect_batch_of_unequal_lists(torch, f):
    imgs = np.stack([ss.image(name) for name in ss.BATCH])
    count, kp, desc = make(torch, 256, 192, max_features=f).detect(dev(torch, imgs))
    kp, desc = kp.cpu().numpy(), desc.cpu().numpy()
    assert count[1] == 0
    for k, name in enumerate(ss.BATCH):
        assert_detection(int(count[k]), kp[k], desc[k], name, f)


# ---- matching --------------------------------------------------------------------------------------------------------------

def run_match(torch, d1, d2, c1=None, c2=None, **changes):
    """sets [n][F][81] (or one pair [k][81], padded with zeros to F = max_features) through vg_sparse_odom_match"""
    F = changes["max_features"]
    if d1.ndim == 2:
        c1, c2 = [len(d1)], [len(d2)]
        pad = lambda d: np.concatenate([d, np.zeros((F - len(d), 81), np.float32)])[None]
        d1, d2 = pad(d1), pad(d2)
    mc, matches, dist = make(torch, **changes).match(c1, dev(torch, d1), c2, dev(torch, d2))
    return mc, matches.cpu().numpy(), dist.cpu().numpy()


def assert_match(mc, matches, dist, ref):
    pairs, rd = ref[0], ref[1]
    assert mc == len(pairs)
    assert np.array_equal(matches[:mc], pairs)
    assert np.array_equal(dist[:mc], rd)   # the sums are exact on both sides


def test_match_full_1024(torch):
    d1, d2 = ss.full_sets()
    mc, matches, dist = run_match(torch, d1, d2, max_features=ss.MAX)
    ref = ss.reference_match("full", d1, d2)
    print("full_1024: %d matches of %d" % (mc[0], len(ref[0])))
    assert_match(int(mc[0]), matches[0], dist[0], ref)


def test_match_count_edges(torch):
    c = ss.count_edges()
    mc, matches, dist = run_match(torch, c["d1"], c["d2"], c["c1"], c["c2"], max_features=ss.SMALL)
    print("count_edges: matches", mc.tolist())
    for k, (n1, n2) in enumerate(ss.COUNT_EDGES):
        assert_match(int(mc[k]), matches[k], dist[k], sr.match(c["d1"][k, :n1], c["d2"][k, :n2]))


@pytest.mark.parametrize("side", [1, 2])
def test_match_nearest_tie(torch, side):
    d1, d2, a, b = ss.nearest_tie(side)
    mc, matches, dist = run_match(torch, d1, d2, max_features=ss.SMALL)
    assert_match(int(mc[0]), matches[0], dist[0], sr.match(d1, d2))
    named = matches[0, :mc[0], side - 1].tolist()
    assert a in named and b not in named   # the lowest index on ties


def test_match_threshold_equal(torch):
    d1, d2, t, pair = ss.threshold_sets()
    counts = []
    for threshold in (t, ss.nextbelow(t), 0.):
        mc, matches, dist = run_match(torch, d1, d2, max_features=ss.SMALL, match_threshold=threshold)
        assert_match(int(mc[0]), matches[0], dist[0], sr.match(d1, d2, threshold))
        counts.append(int(mc[0]))
        assert (list(pair) in matches[0, :mc[0]].tolist()) == (threshold == t)
    print("threshold_equal: %d matches at the distance, %d one double below, %d at zero" % tuple(counts))
    assert counts[0] == counts[1] + 1 and counts[2] == ss.IDENTICAL


# ---- geometry --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", ss.SCORE_M)
def test_score_blocks(torch, m):
    """test_score's two-part rule on m of the 1000 points; the counts also without the residuals"""
    hyp = ss.score_hypotheses()[1]
    ref, own = ss.score_reference(m)
    odo = make(torch)
    args = [dev(torch, a) for a in ss.score_points(m)]
    inl, res = odo.score(hyp, *args)
    res = res.cpu().numpy()
    assert res.shape == ref.shape and np.array_equal(np.isinf(res), np.isinf(ref))
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(res - ref), 0.)
    rows = [np.linalg.norm(err[k]) / np.linalg.norm(ref[k][fin[k]]) for k in range(len(ref))]
    rel = err[fin] / ref[fin]
    print("score m = %d: row-wise max %.3e; per entry max %.3e (restatement's own %.3e), entries above 1e-10: %d (own %d); inliers %s"
          % (m, max(rows), rel.max(), (own[fin] / ref[fin]).max(), (rel > PARITY).sum(), (own[fin] / ref[fin] > PARITY).sum(), inl.tolist()))
    assert max(rows) <= PARITY
    assert (err[fin] <= PARITY * ref[fin] + 100. * own[fin]).all()
    assert np.array_equal(res < sr.INLIER_THRESHOLD, ref < sr.INLIER_THRESHOLD)
    assert np.array_equal(inl, (ref < sr.INLIER_THRESHOLD).sum(1))
    bare, none = odo.score(hyp, *args, residuals=False)
    assert none is None and np.array_equal(bare, inl)


def solve_args(torch):
    return [dev(torch, a) for a in ss.solve_points()]


def unaligned(torch, t):
    """a contiguous copy of t whose first element lies 8 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 8
    return out


def test_solve_sizes(torch):
    off, ref = ss.solve_blocks()["offsets"], ss.solve_reference()
    xo = sc.points_set(ss.SOLVE_POOL)["xi_odom"]
    args = solve_args(torch)
    odo = make(torch)
    xi, rep = odo.solve(off, *args, xo)
    d = np.abs(xi - ref["xi"]).max(1)
    print("solve sizes", ss.SOLVE_SIZES, "difference / margin", (d / ref["margin"]).tolist(), "iterations", rep[:, 0].tolist())
    assert np.isfinite(xi).all() and (rep[:, 0] <= 25).all()
    assert (d <= ref["margin"]).all(), (d, ref["margin"])
    assert np.allclose(rep[:, 1], ref["initial_cost"], rtol=PARITY, atol=0.)
    xi3, rep3 = make(torch, max_lm_iterations=3).solve(off, *args, xo)
    step = np.maximum(1., np.abs(ref["xi3"] - xo).max(1))
    d3 = np.abs(xi3 - ref["xi3"]).max(1) / step
    print("solve sizes: pose after 3 iterations, difference per block", d3.tolist())
    assert (rep3[:, 0] == ref["iterations3"]).all() and (d3 <= sc.SOLVE_FLOOR).all(), d3
    assert (rep[:, 2] <= rep[:, 1]).all()
    for b in range(len(ss.SOLVE_SIZES)):   # every block alone gives the bits it has inside the batch
        one, rep1 = odo.solve([0, off[b + 1] - off[b]], *[a[off[b]:off[b + 1]].contiguous() for a in args], xo)
        assert np.array_equal(one[0], xi[b]) and np.array_equal(rep1[0], rep[b]), b


@pytest.mark.parametrize("which", ["p2", "x1"])
def test_solve_unaligned_points(torch, which):
    off = ss.solve_blocks()["offsets"]
    xo = sc.points_set(ss.SOLVE_POOL)["xi_odom"]
    args = solve_args(torch)
    odo = make(torch)
    xi, rep = odo.solve(off, *args, xo)
    k = ("x1", "x2", "p2", "size").index(which)
    args[k] = unaligned(torch, args[k])
    xi_u, rep_u = odo.solve(off, *args, xo)
    assert np.array_equal(xi_u, xi) and np.array_equal(rep_u, rep)


@pytest.mark.parametrize("name", ss.RANSAC_CASES)
def test_ransac_limits(torch, name):
    c, r = ss.ransac_case(name), ss.ransac_reference(name)
    changes = dict(num_ransac_points=c["points"], ransac_iterations=len(c["samples"]))
    pts = [dev(torch, c[k]) for k in ("x1", "x2", "p2", "size")]
    xi, mask, rep = make(torch, **changes).ransac(*pts, c["xi_odom"], c["samples"])
    mask = mask.cpu().numpy().astype(bool)
    print("ransac", name, rep)
    assert (rep["status"], rep["best"], rep["inliers"], rep["kept"]) == (r["status"], r["best"], r["inliers"], r["kept"])
    assert np.array_equal(mask, r["mask"])
    if r["status"] != sr.STATUS_OK:
        assert rep == REPORT_WITHOUT_HYPOTHESIS and np.array_equal(xi, np.asarray(c["xi_odom"], float)) and not mask.any()
        return
    sel = ss.kept_points(name)
    _, margin = sc.solve_margin(c["x1"][sel], c["x2"][sel], c["p2"][sel], c["size"][sel], c["xi_odom"], key=("shapes_final", name))
    d = np.abs(xi - r["xi_incr"]).max()
    print("ransac", name, "increment: difference %.3e, margin %.3e" % (d, margin))
    assert d <= margin
    # the last solve reads its points through the index list; solve() on the same points gathered reads them directly
    idx = torch.from_numpy(sel.astype(np.int64)).cuda()
    direct, rep_d = make(torch, **changes).solve([0, len(sel)], *[p[idx].contiguous() for p in pts], c["xi_odom"])
    assert np.array_equal(direct[0], xi) and (rep_d[0, 2], rep_d[0, 3]) == (rep["final_cost"], rep["final_termination"])


@pytest.mark.parametrize("kind", ["given", "drawn"])
def test_feed_many_matches(torch, kind):
    f = ss.feed_reference(kind)
    log = f["odo"].log[0]
    r = log["ransac"]
    odo = make(torch, 256, 192, max_features=ss.MAX)
    got = [odo.feed(dev(torch, ss.image(name)), xi, ss.feed_table(kind)) for name, xi in zip(ss.FEED_IMAGES, ss.FEED_ODOMETRY)]
    print("feed", kind, got[1][1])
    assert [g[1]["state"] for g in got] == f["states"]
    assert [g[1]["keypoints"] for g in got] == [len(log["kp1"]), len(log["kp2"])]
    rep = got[1][1]
    assert (rep["matches"], rep["status"], rep["best"], rep["inliers"], rep["kept"]) == (len(log["pairs"]), r["status"], r["best"], r["inliers"], r["kept"])
    x1, x2, p2, size = sr.rays(ss.CAM, log["kp1"], log["kp2"], log["pairs"])
    sel = np.flatnonzero(r["mask"])[r["gate_err"] < r["gate_bound"]]
    incr_odom = sr.pr.inverse_compose(ss.FEED_ODOMETRY[0], ss.FEED_ODOMETRY[1])
    _, margin = sc.solve_margin(x1[sel], x2[sel], p2[sel], size[sel], incr_odom, key=("shapes_feed", kind))
    d = np.abs(got[1][0] - r["xi_incr"]).max()
    print("feed", kind, "increment: difference %.3e, margin %.3e" % (d, margin))
    assert d <= margin and np.array_equal(got[0][0], np.zeros(6))


def test_handle_reuse(torch):
    """one handle used small, large, small in every stage: scratch that grew must not change a later, smaller call"""
    s, r = sc.points_set(), sc.reference_ransac(2)
    pts = {k: dev(torch, s[k]) for k in ("x1", "x2", "p2", "size")}
    c = ss.count_edges()
    imgs = sc.images()
    table = np.concatenate([s["samples2"], s["samples2"][:100]])   # 300 blocks of 2 points
    idx = torch.from_numpy(table.ravel().astype(np.int64)).cuda()
    gathered = [pts[k][idx].contiguous() for k in ("x1", "x2", "p2", "size")]
    new = lambda: make(torch, max_features=ss.SMALL)

    def score(odo, n):
        inl, res = odo.score(r["hypotheses"][:n], pts["x1"], pts["x2"], pts["p2"])
        return [inl, res.cpu().numpy()]

    def match(odo, n):
        mc, matches, dist = odo.match(c["c1"][:n], dev(torch, c["d1"][:n]), c["c2"][:n], dev(torch, c["d2"][:n]))
        return [mc, matches.cpu().numpy(), dist.cpu().numpy()]

    def solve(odo, n):
        return list(odo.solve(np.arange(n + 1) * 2, *[a[:2 * n].contiguous() for a in gathered], s["xi_odom"]))

    def detect(odo, n):
        count, kp, desc = odo.detect(dev(torch, imgs[:n]))
        return [count, kp.cpu().numpy(), desc.cpu().numpy()]

    odo = new()
    for stage, sizes in ((score, (2, 200, 2)), (match, (1, 9, 1)), (solve, (1, 300, 1)), (detect, (1, 3, 1))):
        for n in sizes:
            got, fresh = stage(odo, n), stage(new(), n)
            for a, b in zip(got, fresh):
                assert a.tobytes() == b.tobytes(), (stage.__name__, n)
