"""The conditions the cases of tests/sparse_odom_shapes.py have to meet for tests/test_gpu_sparse_odom_shapes.py to test what it
says, asserted on the restatement alone (tests/sparse_odom_ref.py): conditions on the cases, not measurements.  If a seed breaks
one, change the seed, never the condition.  No GPU."""
import numpy as np

from tests import sparse_odom_ref as sr
from tests import sparse_odom_scene as sc
from tests import sparse_odom_shapes as ss


def test_every_case_has_its_check():
    assert set(ss.NEED) == {name[len("test_"):] for name in globals() if name.startswith("test_")} - {"every_case_has_its_check", "default_points_set_is_unchanged"}


def test_default_points_set_is_unchanged():
    """points_set(n) at n = 120 is the set the scene tests always had: 25 wrong from 10 on, 6 far from 100 on, one generator"""
    s = sc.points_set()
    assert s is sc.points_set(120) and s["x1"].shape == (120, 3)
    assert s["wrong"].tolist() == list(range(10, 35)) and s["far"].tolist() == list(range(100, 106))
    assert sc.clean_block().size == 95
    big = sc.points_set(ss.BIG)
    assert (len(big["wrong"]), len(big["far"])) == (208, 50) and big["samples2"].max() >= 990   # the shares of 25 and 6 in 120


def test_many_candidates():
    need = ss.NEED["many_candidates"]
    counts = [ss.maxima(name)[0].size for name in ss.BATCH]
    print("maxima of the batch", counts)
    assert counts[0] > need["maxima_over"] and counts[2] > need["maxima_over"]   # a second trip of the candidate loops
    assert counts[1] == 0 and counts[0] != counts[2]
    for f in (ss.MAX, ss.MAX - 1, 64):
        kp, n_max, desc = ss.detection("many", f)
        assert n_max == counts[0] > f == len(kp) == len(desc)   # the radix selection, not the shortcut, up to kMaxFeatures itself
    # the candidates beyond the first 1024 of the raster order matter: some of them are selected
    idx = ss.maxima("many")[0]
    late = set(idx[ss.SELECT:].tolist())
    kp = ss.detection("many", 64)[0]
    assert any(int(v) * 256 + int(u) in late for u, v in kp)


def _tie_case(case, name):
    need = ss.NEED[case]
    idx, val = ss.maxima(name)
    assert need["equal_responses"] and len(set(val.tolist())) == 1
    assert idx.min() < need["indices_astride"] < idx.max()
    assert (idx >> 24).max() == 0 and len(set((idx >> 16).tolist())) == 2   # digit 9 of the key differs, digit 8 does not
    features = list(ss.detect_features(name))
    assert len(features) >= 2 and all(0 < f < idx.size for f in features)
    return np.sort(idx)[::-1], features


def test_wide_index_ties():
    idx, features = _tie_case("wide_index_ties", "ties")
    assert idx.size == 300 and idx[0] == 74231 and features == [1, 150, 299]
    for f in features:   # the tie rule alone: the f largest raster indices, descending
        kp = ss.detection("ties", f)[0]
        assert (kp[:, 1].astype(np.int64) * 320 + kp[:, 0]).tolist() == idx[:f].tolist()
    # the cuts at 150 and 299 fall inside a group that digit 9 alone cannot tell from the rest of the list
    assert idx[149] >> 16 == idx[150] >> 16 and (idx >> 16 == idx[149] >> 16).sum() < idx.size


def test_wide_index_ties_cut():
    idx, features = _tie_case("wide_index_ties_cut", "ties_cut")
    f = ss.tie_cut()
    within = ss.NEED["wide_index_ties_cut"]["cut_within"]
    print("cut at", f, "keeps", int(idx[f - 1]), "drops", int(idx[f]))
    assert f in features and idx[f - 1] >= 1 << 16 > idx[f] and idx[f - 1] - (1 << 16) < within and (1 << 16) - idx[f] < within
    kp = ss.detection("ties_cut", f)[0]
    assert (kp[:, 1].astype(np.int64) * 304 + kp[:, 0]).tolist() == idx[:f].tolist()


def test_negative_responses():
    need = ss.NEED["negative_responses"]
    idx, val = ss.maxima("signs")
    pos, neg = int((val > 0).sum()), int((val < 0).sum())
    print("maxima: %d positive, %d negative" % (pos, neg))
    assert pos >= need["each_sign"] and neg >= need["each_sign"]
    cut = ss.sign_cut()
    assert pos < cut < idx.size < ss.MAX and idx.size > cut + 10   # the cut among the negative ones; 1024 keeps all
    kp, n_max, _ = ss.detection("signs", cut)
    R = ss.response("signs")
    kept = np.array([int(R[v, u]) for u, v in kp])
    assert (kept[:pos] > 0).all() and (kept[pos:] < 0).all() and (np.diff(kept) <= 0).all()
    assert len(ss.detection("signs", ss.MAX)[0]) == idx.size
    # a selection on the raw bits would put every negative response above every positive one
    raw = sorted(zip(val.astype(np.uint64).tolist(), idx.tolist()), reverse=True)
    assert [i for _, i in raw[:cut]] != (kp[:, 1].astype(np.int64) * 256 + kp[:, 0]).tolist()


def test_min_image():
    need = ss.NEED["min_image"]
    kp, n_max, _ = ss.detection("min", 500)
    assert ss.image("min").shape == (15, 15) and kp.tolist() == [list(need["one_keypoint_at"])] and n_max == 1
    assert ss.detection("min_flat", 500)[1] == 0
    for name, shape in (("wide", (15, 41)), ("tall", (41, 15))):
        kp, n_max, desc = ss.detection(name, 500)
        print(name, kp.tolist())
        assert ss.image(name).shape == shape and n_max >= need["strips_have"] and len(desc) == n_max
        cap = ((shape[1] - 13) // 2) * ((shape[0] - 13) // 2)   # the handle's candidate capacity
        assert n_max <= cap
    # a key point on row or column 7: its patch reaches pixel row or column 3 = 7 - 4
    assert (ss.detection("wide", 500)[0][:, 1] - sr.PATCH == need["patch_reaches"]).all()
    assert (ss.detection("tall", 500)[0][:, 0] - sr.PATCH == need["patch_reaches"]).all()


def _exact_sums(d1, d2, D):
    """the conditions of test_conditions_the_gpu_tests_rely_on under which every order of the 81 terms gives the same bits"""
    assert np.array_equal(sr.distance_matrix(d1, d2, range(80, -1, -1)), D)
    assert np.array_equal(sr.distance_matrix(d1, d2, np.random.default_rng(1).permutation(81)), D)
    for d in (d1, d2):
        assert np.abs(d).max() < 256. and np.spacing(np.abs(d[d != 0.]).min()) >= 2. ** -29


def _decisions_clear(D, threshold, rel, ties_allowed=False):
    for M in (D, D.T):
        if M.shape[1] > 1 and not ties_allowed:
            srt = np.sort(M, axis=1)
            assert (srt[:, 1] > srt[:, 0]).all()
    if D.size:
        assert (np.abs(D.min(1) - threshold) >= rel * threshold).all() and (np.abs(D.min(0) - threshold) >= rel * threshold).all()


def test_full_1024():
    need = ss.NEED["full_1024"]
    d1, d2 = ss.full_sets()
    pairs, dist, D = ss.reference_match("full", d1, d2)
    print("full_1024: %d matches, distances %.1f .. %.1f" % (len(pairs), dist.min(), dist.max()))
    assert d1.shape == d2.shape == (need["counts"], 81) and len(pairs) > need["matches_over"]
    assert (np.diff(pairs[:, 0]) > 0).all() and pairs[-1, 0] >= 960   # accepted matches in the last wave of the compaction
    _decisions_clear(D, sr.MATCH_THRESHOLD, need["threshold_clear"])
    _exact_sums(d1, d2, D)


def test_count_edges():
    need = ss.NEED["count_edges"]
    c = ss.count_edges()
    assert list(zip(c["c1"].tolist(), c["c2"].tolist())) == list(ss.COUNT_EDGES) and c["d1"].shape == (9, ss.SMALL, 81)
    for k, (n1, n2) in enumerate(ss.COUNT_EDGES):
        pairs, _, D = sr.match(c["d1"][k, :n1], c["d2"][k, :n2])
        whole = sr.match(c["d1"][k], c["d2"][k])[0]
        print("pair", k, (n1, n2), "matches", len(pairs), "of", len(whole), "with all 65")
        assert (len(pairs) >= 1) == (min(n1, n2) > 0)
        assert pairs.tobytes() != whole.tobytes()   # a kernel that took the batch's largest counts for this pair would differ
        _decisions_clear(D, sr.MATCH_THRESHOLD, need["threshold_clear"])
    _exact_sums(c["d1"][0], c["d2"][0], sr.distance_matrix(c["d1"][0], c["d2"][0]))


def test_nearest_tie():
    for side in (1, 2):
        d1, d2, a, b = ss.nearest_tie(side)
        pairs, _, D = sr.match(d1, d2)
        M = D if side == 2 else D.T   # rows: the side that chooses among the repeated descriptors
        assert a < b and np.array_equal(M[:, a], M[:, b])
        i = int(M[:, a].argmin())
        assert M[i, a] == M[i].min() and (M[i] == M[i].min()).sum() == 2   # the restatement reports the tie
        want = [i, a] if side == 2 else [a, i]
        other = [i, b] if side == 2 else [b, i]
        assert want in pairs.tolist() and other not in pairs.tolist()
        last = ss.match_last(d1, d2)
        print("side", side, "tie between", a, b, "for", i, ":", len(pairs), "matches; with the last index", len(last))
        assert other in last.tolist() and want not in last.tolist() and last.tobytes() != pairs.tobytes()
        _exact_sums(d1, d2, D)


def test_threshold_equal():
    d1, d2, t, pair = ss.threshold_sets()
    at, dist_at, D = sr.match(d1, d2, t)
    below = sr.match(d1, d2, ss.nextbelow(t))[0]
    zero, dist_zero, _ = sr.match(d1, d2, 0.)
    print("threshold %r: %d matches, one double below %d, at zero %d" % (t, len(at), len(below), len(zero)))
    assert D[pair] == t == dist_at.max() and list(pair) in at.tolist() and (dist_at == t).sum() == 1
    assert [p for p in at.tolist() if p != list(pair)] == below.tolist()
    assert 1 < len(at) < len(sr.match(d1, d2)[0])   # the threshold drops others above it as well
    assert len(zero) == ss.IDENTICAL and (dist_zero == 0.).all() and all(np.array_equal(d1[i], d2[j]) for i, j in zero)
    _exact_sums(d1, d2, D)


def test_score_blocks():
    need = ss.NEED["score_blocks"]
    rows, hyp = ss.score_hypotheses()
    assert hyp.shape == (ss.SCORE_HYPOTHESES, 6) and len(set(rows.tolist())) == ss.SCORE_HYPOTHESES
    ref, own = ss.score_reference(ss.BIG)
    inl = ref < sr.INLIER_THRESHOLD
    blocks = [sorted(set((np.flatnonzero(r) // ss.BLOCK).tolist())) for r in inl]
    print("inliers", inl.sum(1).tolist(), "blocks", blocks, "+inf entries", int(np.isinf(ref).sum()))
    assert all(len(b) >= need["blocks_with_inliers"] for b in blocks)
    assert np.isinf(ref).any() and all(ss.BIG // ss.BLOCK in b for b in blocks) and ss.BIG % ss.BLOCK
    assert len(set(inl.sum(1).tolist())) > 1
    print("inliers at position", need["inlier_at"], inl[:, need["inlier_at"]].tolist())
    assert inl[:, need["inlier_at"]].sum() > ss.SCORE_HYPOTHESES // 2   # m = 257: the one lane of the second block adds to most counts
    for m in ss.SCORE_M:
        r = ss.score_reference(m)[0]
        assert r.shape == (ss.SCORE_HYPOTHESES, m) and np.allclose(r, ref[:, :m], rtol=1e-6, atol=0.)   # the same points: a head of the 1000
        assert np.abs(r[np.isfinite(r)] - sr.INLIER_THRESHOLD).min() > need["threshold_clear"]


def test_solve_sizes():
    need = ss.NEED["solve_sizes"]
    b = ss.solve_blocks()
    assert tuple(np.diff(b["offsets"]).tolist()) == need["sizes"] == ss.SOLVE_SIZES
    wrong = set(sc.points_set(ss.SOLVE_POOL)["wrong"].tolist())
    assert not wrong & set(b["index"].tolist())
    for k in range(len(ss.SOLVE_SIZES)):
        own = b["index"][b["offsets"][k]:b["offsets"][k + 1]]
        assert len(set(own.tolist())) == len(own)
    ref = ss.solve_reference()
    print("solve margins", ref["margin"].tolist(), "iterations of the short solves", ref["iterations3"].tolist())
    assert np.isfinite(ref["xi"]).all() and (ref["margin"] < 1e-3).all()   # settled problems: the margin means something


def test_ransac_limits():
    need = ss.NEED["ransac_limits"]
    want = {"big": sr.STATUS_OK, "sixteen_16": sr.STATUS_NO_HYPOTHESIS, "sixteen_17": sr.STATUS_OK, "one_iteration": sr.STATUS_OK,
            "all_wrong": sr.STATUS_NO_HYPOTHESIS}
    for name in ss.RANSAC_CASES:
        c, r = ss.ransac_case(name), ss.ransac_reference(name)
        m = len(c["x1"])
        print(name, "m", m, "status", r["status"], "best", r["best"], "inliers", r["inliers"], "kept", r["kept"])
        assert r["status"] == want[name] and c["samples"].max() < m and c["samples"].shape[1] == c["points"]
        res = r["residuals"]
        assert np.abs(res[np.isfinite(res)] - sr.INLIER_THRESHOLD).min() > need["threshold_clear"]
        if r["status"] == sr.STATUS_OK:
            assert np.abs(r["gate_err"] / r["gate_bound"] - 1.).min() > need["gate_clear"]
            assert r["kept"] == len(ss.kept_points(name)) > 2
        else:
            assert r["best"] == -1 and not r["mask"].any() and np.array_equal(r["xi_incr"], c["xi_odom"])
    big = ss.ransac_reference("big")
    assert big["inliers"] > 2 * ss.BLOCK and big["kept"] < big["inliers"]   # the mask and the gate across several blocks
    assert ss.ransac_case("sixteen_16")["x1"].shape[0] == 16 and ss.ransac_case("sixteen_17")["x1"].shape[0] == 17
    assert ss.ransac_reference("sixteen_17")["inliers"] == 17   # more than 16 points: every one of the 17
    assert ss.ransac_case("one_iteration")["samples"].shape == (1, 2)
    wrong = ss.ransac_reference("all_wrong")["residuals"]
    assert wrong.shape == (200, ss.ALL_WRONG) and (wrong < sr.INLIER_THRESHOLD).sum(1).max() == 2   # hypotheses that fit their own two points


def test_feed_many_matches():
    need = ss.NEED["feed_many_matches"]
    m = ss.feed_matches()
    table = ss.feed_table("given")
    folded = table % m
    assert m > need["matches_over"] and (table >= m).mean() > 0.5 and (folded[:, 0] != folded[:, 1]).all()
    assert np.array_equal(folded, sc.sample_table(2, m))
    for kind in ("given", "drawn"):
        f = ss.feed_reference(kind)
        log = f["odo"].log[0]
        r = log["ransac"]
        print(kind, "key points", len(log["kp1"]), len(log["kp2"]), "matches", len(log["pairs"]), "best", r["best"], "inliers", r["inliers"], "kept", r["kept"])
        assert f["states"] == [sr.STATE_FIRST, sr.STATE_ESTIMATED] and len(log["pairs"]) == m
        assert len(log["kp1"]) == len(log["kp2"]) == ss.MAX and r["status"] == sr.STATUS_OK and r["inliers"] > need["matches_over"]
        res = r["residuals"]
        assert np.abs(res[np.isfinite(res)] - sr.INLIER_THRESHOLD).min() > need["threshold_clear"]
        assert np.abs(r["gate_err"] / r["gate_bound"] - 1.).min() > need["gate_clear"]
        _decisions_clear(log["D"], sr.MATCH_THRESHOLD, 1e-3)
        _exact_sums(log["desc1"], log["desc2"], log["D"])


def test_handle_reuse():
    """small, large, small on one handle: the large call of every stage is larger than either small one"""
    assert ss.NEED["handle_reuse"]["sizes_rise_and_fall"]
    assert sc.reference_ransac(2)["hypotheses"].shape[0] == 200 > 2 and len(ss.COUNT_EDGES) == 9 > 1 and sc.images().shape[0] == 3 > 1
    assert sc.points_set()["samples2"].shape[0] + sc.points_set()["samples3"].shape[0] >= 300
