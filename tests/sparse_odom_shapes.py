"""Inputs of the sparse odometry shape tests (tests/test_gpu_sparse_odom_shapes.py, tests/test_sparse_odom_shapes_cpu.py): the
smallest images, descriptor sets and point sets at which the kernels of vg_sparse_odom.hpp take the paths that the scene of
tests/sparse_odom_scene.py leaves out -- a candidate list longer than the selection's workgroup, max_features at its maximum,
raster indices on both sides of 2^16 in a group of equal responses, responses of both signs, the smallest image, 1024 x 1024
distances, counts at the edges of the distance tile and of the compaction's wave, a tied nearest neighbour, a distance equal to
the threshold, point counts across the scoring blocks and the solve's lanes, and every ransac status.  Each case names the
conditions (NEED) that the restatement (tests/sparse_odom_ref.py) must meet for the case to be live: conditions on the case, not
measurements.  Everything is built once per process, frozen and left unchanged; nothing here needs a GPU."""
import math

import numpy as np

from tests import sparse_odom_ref as sr
from tests import sparse_odom_scene as sc

SELECT, BLOCK, LANES, TILE = 1024, 256, 64, 16   # the selection's workgroup, the scoring block, a wave, the distance tile
MAX = 1024                                        # kMaxFeatures
SMALL = 65                                        # max_features of the count-edge handle: one over a wave
CAM, XBC = sc.CAM, sc.XI_BASE_CAM

# What the restatement must show for a case to be live (tests/test_sparse_odom_shapes_cpu.py asserts every entry):
NEED = {
    "many_candidates": dict(maxima_over=SELECT, batch_counts_differ=True),
    "wide_index_ties": dict(equal_responses=True, indices_astride=1 << 16, features_below_maxima=True),
    "wide_index_ties_cut": dict(equal_responses=True, indices_astride=1 << 16, features_below_maxima=True, cut_within=256),
    "negative_responses": dict(each_sign=50, cut_among_negative=True, keeps_all=True),
    "min_image": dict(one_keypoint_at=(7, 7), flat_has_none=True, strips_have=3, patch_reaches=3),
    "full_1024": dict(counts=MAX, matches_over=BLOCK, no_tie=True, threshold_clear=1e-3, exact_sums=True),
    "count_edges": dict(matches_everywhere=True, own_counts_matter=True, no_tie=True, threshold_clear=1e-3),
    "nearest_tie": dict(tie_reported=True, last_index_differs=True),
    "threshold_equal": dict(kept_at_equality=True, only_it_dropped_below=True, zero_keeps_identical=True),
    "score_blocks": dict(blocks_with_inliers=3, some_inf=True, inlier_in_last_block=True, inlier_at=BLOCK, threshold_clear=1e-5),
    "solve_sizes": dict(sizes=(1, 63, 64, 65, 128, 129, 1000, 0, 2), clean_only=True),
    "ransac_limits": dict(statuses=True, threshold_clear=1e-5, gate_clear=1e-6),
    "feed_many_matches": dict(matches_over=BLOCK, table_folds=True, threshold_clear=1e-5, gate_clear=1e-6),
    "handle_reuse": dict(sizes_rise_and_fall=True),
}

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _frozen(a):
    a.setflags(write=False)
    return a


def _freeze_all(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- detection -------------------------------------------------------------------------------------------------------------

def _random(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _tile():
    tile = np.zeros((16, 16), np.uint8)   # the tile of test_detect_flat_and_ties: one maximum at (7, 7), the same in every copy
    tile[5:10, 5:10] = 255
    return tile


def _signs():
    """stripes of period 12 with a little noise (an edge everywhere: every maximum negative) beside a random block (positive)"""
    rng = np.random.default_rng(11)
    stripes = ((np.arange(128) // 6) % 2 * 200)[None, :] + rng.integers(0, 8, (96, 128))
    return np.hstack([stripes, rng.integers(0, 256, (96, 128))]).astype(np.uint8)


def _noisy():
    return np.clip(image("many").astype(np.int64) + np.random.default_rng(8).integers(-6, 7, image("many").shape), 0, 255).astype(np.uint8)


def _shifted(first):
    big = _random(16, 192, 258)   # two views of one texture, 2 px apart
    return np.ascontiguousarray(big[:, :256] if first else big[:, 2:])


IMAGES = {
    "many": lambda: _random(7, 192, 256),             # more maxima than the selection has threads
    "many_b": lambda: _random(9, 192, 256),
    "many_flat": lambda: np.full((192, 256), 90, np.uint8),
    "many_noisy": _noisy,
    "ties": lambda: np.tile(_tile(), (15, 20)),       # 240 x 320 (height x width)
    "ties_cut": lambda: np.tile(_tile(), (15, 19)),   # 240 x 304: the row v = 215 starts at raster index 65360 and crosses 2^16
    "signs": _signs,
    "min": lambda: _random(72, 15, 15),
    "min_flat": lambda: np.full((15, 15), 90, np.uint8),
    "wide": lambda: _random(6, 15, 41),
    "tall": lambda: _random(1, 41, 15),
    "shift_a": lambda: _shifted(True),
    "shift_b": lambda: _shifted(False),
}


def image(name):
    """u8 [height][width]"""
    return cached(("image", name), lambda: _frozen(IMAGES[name]()))


def response(name):
    return cached(("response", name), lambda: _frozen(sr.response(image(name))))


def maxima(name):
    """(raster indices, responses) of the image's maxima, in raster order"""
    def make():
        idx = sr.maxima(response(name))
        return _frozen(idx), _frozen(response(name).ravel()[idx])
    return cached(("maxima", name), make)


def detection(name, max_features):
    """the restatement's (key points, number of maxima, descriptors) of an image, cached"""
    def make():
        kp, n_max = sr.detect(image(name), max_features)
        return _frozen(kp), n_max, _frozen(sr.descriptors(image(name), kp))
    return cached(("detect", name, max_features), make)


def tie_cut():
    """a max_features of "ties_cut" whose last kept and first dropped raster index lie on either side of 2^16, both within 256"""
    idx = np.sort(maxima("ties_cut")[0])[::-1]
    return int((idx >= 1 << 16).sum())


def sign_cut():
    """a max_features of "signs" that keeps every positive maximum and half of the negative ones"""
    val = maxima("signs")[1]
    return int((val > 0).sum() + (val < 0).sum() // 2)


DETECT_IMAGES = ("many", "ties", "ties_cut", "signs", "min", "min_flat", "wide", "tall")


def detect_features(name):
    """the max_features at which an image of DETECT_IMAGES is detected alone"""
    if name == "ties_cut":
        return tie_cut(), 284
    if name == "signs":
        return sign_cut(), MAX   # among the negative maxima; all of them
    return {"many": (MAX, MAX - 1, 64), "ties": (1, 150, 299)}.get(name, (500,))


BATCH = ("many", "many_flat", "many_b")   # candidate lists of very different lengths under one launch


# ---- matching --------------------------------------------------------------------------------------------------------------

def full_sets():
    """(descriptors of "many", of "many_noisy"), 1024 each"""
    return detection("many", MAX)[2], detection("many_noisy", MAX)[2]


def reference_match(key, d1, d2, threshold=sr.MATCH_THRESHOLD):
    """the restatement's (pairs, distance, D), cached under key and frozen"""
    return cached(("match", key), lambda: tuple(_frozen(a) for a in sr.match(d1, d2, threshold)))


def match_last(d1, d2, threshold=sr.MATCH_THRESHOLD):
    """sr.match with the LAST index on ties: what a nearest-neighbour search with <= for < computes"""
    D = sr.distance_matrix(d1, d2)
    nn1 = D.shape[1] - 1 - D[:, ::-1].argmin(1)
    nn2 = D.shape[0] - 1 - D[::-1].argmin(0)
    return np.array([(i, j) for i, j in enumerate(nn1) if nn2[j] == i and not D[i, j] > threshold], np.int32).reshape(-1, 2)


def small_sets():
    """(A, B) [65][81]: the two sides of the first 65 matches of the full sets, side B shuffled -- every A has its partner in B"""
    def make():
        d1, d2 = full_sets()
        pairs = reference_match("full", d1, d2)[0][:SMALL]
        perm = np.random.default_rng(31).permutation(SMALL)
        return _frozen(d1[pairs[:, 0]].copy()), _frozen(d2[pairs[perm, 1]].copy())
    return cached("small_sets", make)


COUNT_EDGES = ((1, 65), (65, 1), (15, 17), (16, 16), (17, 15), (63, 65), (64, 64), (65, 63), (0, 64))


def count_edges():
    """dict(d1, d2 [9][65][81], c1, c2 [9]): every pair holds all 65 descriptors (rolled by 7 per pair), the counts take a head"""
    def make():
        A, B = small_sets()
        d1 = np.stack([np.roll(A, 7 * k, axis=0) for k in range(len(COUNT_EDGES))])
        d2 = np.stack([np.roll(B, 7 * k, axis=0) for k in range(len(COUNT_EDGES))])
        c = np.array(COUNT_EDGES, np.int32)
        return _freeze_all({"d1": d1, "d2": d2, "c1": c[:, 0].copy(), "c2": c[:, 1].copy()})
    return cached("count_edges", make)


def nearest_tie(side):
    """(d1, d2, a, b): the small sets with descriptor a of `side` (1 or 2) repeated at b > a; a is half of an accepted match"""
    def make():
        A, B = (x.copy() for x in small_sets())
        pairs = sr.match(A, B)[0]
        col = side - 1
        a = int(pairs[pairs[:, col] < SMALL - 10][5, col])
        b = a + 3
        (A if side == 1 else B)[b] = (A if side == 1 else B)[a]
        return _frozen(A), _frozen(B), a, b
    return cached(("nearest_tie", side), make)


IDENTICAL = 3


def threshold_sets():
    """(d1, d2, threshold, pair): the small sets with IDENTICAL partners on side 2 replaced by exact copies; threshold is the
    exact double of the distance of the accepted match `pair`, the median one"""
    def make():
        A, B = (x.copy() for x in small_sets())
        pairs = sr.match(A, B)[0]
        for i, j in pairs[:IDENTICAL]:
            B[j] = A[i]
        pairs, dist, _ = sr.match(A, B)
        k = int(np.argsort(dist, kind="stable")[len(dist) // 2])
        return _frozen(A), _frozen(B), float(dist[k]), (int(pairs[k, 0]), int(pairs[k, 1]))
    return cached("threshold_sets", make)


# ---- geometry --------------------------------------------------------------------------------------------------------------

SCORE_M = (1, 63, 64, 65, 255, 256, 257, 1000)
SCORE_HYPOTHESES = 7
SCORE_ORDER_SEED = 61
SOLVE_SIZES = (1, 63, 64, 65, 128, 129, 1000, 0, 2)
BIG, SOLVE_POOL = 1000, 1280   # 1280 points hold 1014 clean ones: a block of 1000 without a repeat
ALL_WRONG = 8


def ransac_big():
    """the restatement's ransac on the 1000 points, 2 per hypothesis (case 11 a), cached and left unchanged"""
    def make():
        s = sc.points_set(BIG)
        return sr.ransac(CAM, XBC, s["x1"], s["x2"], s["p2"], s["size"], s["xi_odom"], s["samples2"], 2)
    return cached("ransac_big", make)


def score_hypotheses():
    """(rows, [7][6]): of ransac_big's hypotheses with 30 inliers or more the best, the first with points that do not project,
    and the first five others"""
    def make():
        r = ransac_big()
        counts = (r["residuals"] < sr.INLIER_THRESHOLD).sum(1)
        ok = [k for k in range(len(counts)) if counts[k] >= 30]
        rows = [r["best"]] + [k for k in ok if np.isinf(r["residuals"][k]).any()][:1]
        rows += [k for k in ok if k not in rows][:SCORE_HYPOTHESES - len(rows)]
        return _frozen(np.array(rows)), _frozen(r["hypotheses"][rows].copy())
    return cached("score_hypotheses", make)


def score_points(m):
    """(x1, x2, p2) of the first m of the 1000 points in a fixed shuffled order: the wrong pairs (83 to 290 in the set's own order)
    spread over all blocks, and an inlier of most hypotheses at position 256, alone in the second block when m = 257"""
    def make():
        s, order = sc.points_set(BIG), np.random.default_rng(SCORE_ORDER_SEED).permutation(BIG)[:m]
        return tuple(_frozen(np.ascontiguousarray(s[k][order])) for k in ("x1", "x2", "p2"))
    return cached(("score_points", m), make)


def score_reference(m):
    """(residuals [7][m] of the restatement on score_points(m), the restatement's own rounding error there)"""
    def make():
        x1, x2, p2 = score_points(m)
        xbc, hyp = np.asarray(XBC, float), score_hypotheses()[1]
        ref = np.array([sr.score(CAM, xbc, xi, x1, x2, p2) for xi in hyp])
        ext = np.array([sr.score(CAM, xbc, xi, x1, x2, p2, np.longdouble) for xi in hyp])
        with np.errstate(invalid="ignore"):
            own = np.where(np.isfinite(ref), np.abs(ext - ref), 0.).astype(np.float64)
        return _frozen(ref), _frozen(own)
    return cached(("score", m), make)


def solve_blocks():
    """dict(index [1452] into the 1280 points, offsets [10]): every block its own draw, without a repeat, from the clean points"""
    def make():
        rng, clean = np.random.default_rng(21), sc.clean_block(SOLVE_POOL)
        idx = [rng.choice(clean, size=n, replace=False) for n in SOLVE_SIZES]
        return _freeze_all({"index": np.concatenate(idx).astype(np.int64), "offsets": np.concatenate([[0], np.cumsum(SOLVE_SIZES)]).astype(np.int64)})
    return cached("solve_blocks", make)


def solve_points():
    """(x1, x2, p2, size) of solve_blocks, gathered"""
    s, idx = sc.points_set(SOLVE_POOL), solve_blocks()["index"]
    return cached("solve_points", lambda: tuple(_frozen(np.ascontiguousarray(s[k][idx])) for k in ("x1", "x2", "p2", "size")))


def solve_reference():
    """per block: (xi, margin) of sc.solve_margin, and the restatement stopped after 3 iterations"""
    def make():
        off, pts, xo = solve_blocks()["offsets"], solve_points(), sc.points_set(SOLVE_POOL)["xi_odom"]
        full, short = [], []
        for b in range(len(SOLVE_SIZES)):
            args = [a[off[b]:off[b + 1]] for a in pts]
            full.append(sc.solve_margin(*args, xo))
            short.append(sr.solve(CAM, XBC, *args, xo, 3))
        return {"xi": np.array([f[0] for f in full]), "margin": np.array([f[1] for f in full]), "xi3": np.array([s[0] for s in short]),
                "iterations3": np.array([s[1]["iterations"] for s in short]), "initial_cost": np.array([s[1]["initial_cost"] for s in short])}
    return cached("solve_reference", make)


def ransac_case(name):
    """dict(x1, x2, p2, size, xi_odom, samples, points, iterations) of a ransac case:
      big        the 1000 points, 2 per hypothesis
      sixteen_16 / sixteen_17   16 points per hypothesis on 16 / 17 near, clean points of the 120
      one_iteration   the 120 points and the one row of their table that the full run found best
      all_wrong  eight of the 120 points with every second pixel moved far off"""
    def make():
        if name == "big":
            s = sc.points_set(BIG)
            return dict(s, samples=s["samples2"], points=2)
        s = sc.points_set()
        if name.startswith("sixteen"):
            m = int(name[-2:])
            sel = np.setdiff1d(sc.clean_block(), s["far"])[:m]
            out = {k: np.ascontiguousarray(s[k][sel]) for k in ("x1", "x2", "p2", "size")}
            return dict(out, xi_odom=s["xi_odom"], samples=sc.sample_table(16, m), points=16)
        if name == "one_iteration":
            best = sc.reference_ransac(2)["best"]
            return dict(s, samples=s["samples2"][best:best + 1].copy(), points=2)
        if name == "all_wrong":
            # A pair is an inlier of a hypothesis whenever its second pixel lies within the threshold of the epipolar LINE, and
            # two points leave a hypothesis free to turn: of many wrong pairs some always agree with some hypothesis (120 random
            # pairs: up to 17 inliers).  Eight pairs, each second pixel 15 to 40 px off in u and in v, and a seed for which the
            # restatement finds no third inlier in any of the 200 hypotheses.
            rng, sel = np.random.default_rng(41), sc.clean_block()[:ALL_WRONG]
            p2 = s["p2"][sel] + rng.uniform(15, 40, (ALL_WRONG, 2)) * rng.choice([-1., 1.], (ALL_WRONG, 2))
            x2, _ = sr.pr.reconstruct(CAM, p2[:, 0], p2[:, 1])
            return dict(x1=s["x1"][sel], x2=np.ascontiguousarray(x2), p2=p2, size=np.ones(ALL_WRONG), xi_odom=s["xi_odom"],
                        samples=sc.sample_table(2, ALL_WRONG), points=2)
        raise KeyError(name)
    return cached(("ransac_case", name), lambda: _freeze_all({k: v.copy() if isinstance(v, np.ndarray) else v for k, v in make().items()}))


RANSAC_CASES = ("big", "sixteen_16", "sixteen_17", "one_iteration", "all_wrong")


def ransac_reference(name):
    """the restatement's ransac of a case, cached and left unchanged"""
    def make():
        if name == "big":
            return ransac_big()
        c = ransac_case(name)
        return sr.ransac(CAM, XBC, c["x1"], c["x2"], c["p2"], c["size"], c["xi_odom"], c["samples"], c["points"])
    return cached(("ransac_ref", name), make)


def kept_points(name):
    """indices of the points the final solve of a case runs on"""
    r = ransac_reference(name)
    return np.flatnonzero(r["mask"])[r["gate_err"] < r["gate_bound"]]


# ---- feed ------------------------------------------------------------------------------------------------------------------

FEED_ODOMETRY = (np.zeros(6), np.array([0.05, 0., 0., 0., 0., 0.01]))
FEED_IMAGES = ("shift_a", "shift_b")


def feed_matches():
    """the number of matches of the two frames at max_features = 1024"""
    d = [detection(name, MAX)[2] for name in FEED_IMAGES]
    return len(reference_match("feed", d[0], d[1])[0])


def feed_table(kind):
    """the sample table handed to feed: "given" -- distinct indices below m per row, raised by multiples of m so that most
    entries are above the match count and only the fold brings them back; "drawn" -- None, the handle draws its own"""
    if kind == "drawn":
        return None
    m = feed_matches()
    return cached("feed_table", lambda: _frozen(sc.sample_table(2, m) + m * np.random.default_rng(51).integers(0, 4, (sr.RANSAC_ITERATIONS, 2)).astype(np.int32)))


def feed_reference(kind):
    """the restatement fed the two frames: dict(states, odo); "drawn" uses sr.Draw's first table for the match count"""
    def make():
        odo = sr.SparseOdometry(CAM, XBC, max_features=MAX)
        table = feed_table(kind) if kind == "given" else sr.Draw().table(feed_matches())
        states = [odo.feed(image(name), xi, table) for name, xi in zip(FEED_IMAGES, FEED_ODOMETRY)]
        return {"states": states, "odo": odo}
    return cached(("feed", kind), make)


def nextbelow(x):
    return math.nextafter(x, -math.inf)
