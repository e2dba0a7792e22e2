"""Restatement of the reference's point clouds, plane prior and accuracy score, on top of tests/stereo_ref.py:
DepthMap::reconstruct(pack, flags) (depth_map.cpp:532-635) with getIdxVec (:508-529), DepthMap::generatePlane (:762-803) and
analyzeError of test/reconstruction/stereo_test.cpp:32-84.  Plain Python, a loop per query, plane and pixel, written from the
rule and not from the kernels.  Where the library deviates from the reference the restatement follows the library's contract
("Point clouds and accuracy"): NaN counts as below MIN_DEPTH, index x_max y_max is skipped, a query point
is compared with the map in double, and `poses` moves the items' points."""
import math

import numpy as np

from tests import stereo_ref as sr

MIN_DEPTH = 0.25
DEFAULT_DEPTH, DEFAULT_SIGMA = 5., 30.
QUERY_POINTS, IMAGE_VALUES, MINMAX, ALL_HYPOTHESES, DEFAULT_VALUES, SIGMA_VALUE, QUERY_INDICES, INDEX_MAPPING = 1, 2, 4, 8, 16, 32, 64, 128
FIELDS = ("indices", "hyp", "points", "sigma", "index_map", "item", "valid", "cloud", "counts")


def cround_f(x):
    """C round() of a finite double, as a float: half away from zero"""
    if abs(x) >= 2. ** 52:
        return x
    r = float(math.trunc(x))
    if abs(x - r) >= 0.5:   # exact: x - trunc(x) has no rounding
        r += math.copysign(1., x)
    return math.copysign(r, x)


def transform(xi, X):
    """Transformation::transform: rotMat X + trans"""
    R = sr.rotation_matrix(xi[3:6], 1.)
    w = sr.mat_vec(R, X)
    return tuple(w[i] + xi[i] for i in range(3))


def queries(prm, depth0, flags, query_points, query_indices):
    """[(pixel index or -1, image point)] of one map: getIdxVec / getPointVec"""
    X, Y, sc, u0, v0 = prm["x_max"], prm["y_max"], prm["scale"], prm["u0"], prm["v0"]

    def pixel_point(i):
        return (float((i % X) * sc + u0), float((i // X) * sc + v0))

    out = []
    if flags & QUERY_INDICES:
        for q in query_indices:
            q = int(q)
            out.append((q, pixel_point(q)) if 0 <= q < X * Y else (-1, None))
    elif flags & QUERY_POINTS:
        for u, v in query_points:
            u, v = float(u), float(v)
            ok = math.isfinite(u) and math.isfinite(v)
            if ok:
                fx, fy = cround_f((u - u0) / sc), cround_f((v - v0) / sc)
                ok = 0 <= fx < X and 0 <= fy < Y
            out.append((int(fy) * X + int(fx), (u, v)) if ok else (-1, None))
    else:
        flat = depth0.reshape(-1)
        out = [(i, pixel_point(i)) for i in range(X * Y) if flat[i] >= MIN_DEPTH]
    return out


def reconstruct(cam, prm, depth, sigma=None, flags=0, query_points=None, query_indices=None, poses=None):
    """dict of FIELDS.  depth, sigma: [n][hyp_max][Y][X]; sigma may be None when no flag reads it"""
    assert not flags & IMAGE_VALUES
    depth = np.asarray(depth, dtype=np.float64)
    n, H = depth.shape[:2]
    num_hyps = H if flags & ALL_HYPOTHESES else 1
    idx, hyp, pts, sig, imap, item, valid, cloud, counts = [], [], [], [], [], [], [], [], []
    for k in range(n):
        d, s = depth[k].reshape(H, -1), (None if sigma is None else np.asarray(sigma)[k].reshape(H, -1))
        before = len(idx)
        for i, (q, pt) in enumerate(queries(prm, depth[k, 0], flags, query_points, query_indices)):
            if q < 0:
                continue
            ray = sr.reconstruct(cam, pt[0], pt[1])
            if ray is not None:
                nrm = math.sqrt(sr.dot3(ray, ray))
                ray = tuple(c / nrm for c in ray)
            for h in range(num_hyps):
                dv = float(d[h, q])
                sv = float(s[h, q]) if s is not None else 0.
                if not dv >= MIN_DEPTH:
                    if flags & DEFAULT_VALUES and h == 0:
                        dv, sv = DEFAULT_DEPTH, (DEFAULT_SIGMA if s is not None else 0.)
                    else:
                        continue
                ranges = (max(dv - 3 * sv, MIN_DEPTH), dv + 3 * sv) if flags & MINMAX else (dv,)
                idx.append(q)
                hyp.append(h)
                pts.append(pt)
                sig.append(sv)
                imap.append(i)
                item.append(k)
                valid.append(0 if ray is None else 1)
                entry = []
                for r in ranges:
                    if ray is None:
                        entry.append((0., 0., 0.))
                    else:
                        p = tuple(c * r for c in ray)
                        entry.append(transform(poses[k], p) if poses is not None else p)
                cloud.append(entry)
        counts.append(len(idx) - before)
    m = len(idx)
    res = dict(indices=np.array(idx, np.int32), hyp=np.array(hyp, np.int32), points=np.array(pts, np.float64).reshape(m, 2),
               sigma=np.array(sig, np.float64) if flags & SIGMA_VALUE else None,
               index_map=np.array(imap, np.int32) if flags & INDEX_MAPPING else None, item=np.array(item, np.int32),
               valid=np.array(valid, np.uint8), counts=np.array(counts, np.int64))
    c = np.array(cloud, np.float64)
    res["cloud"] = c.reshape(m, 2, 3) if flags & MINMAX else c.reshape(m, 3)
    return res


def generate_plane(cam, prm, xi_cam_plane, polygon):
    """(depth, sigma, cost) [Y][X], and per pixel what the GPU test asks of the scene: (|ray . normal| / (|ray| |normal|) minimum over
    the edges, z . ray), NaN where the pixel never got there"""
    X, Y = prm["x_max"], prm["y_max"]
    xi = [float(v) for v in xi_cam_plane]
    R = sr.rotation_matrix(xi[3:6], 1.)
    t = tuple(xi[:3])
    z = (R[2], R[5], R[8])
    poly = [transform(xi, tuple(float(c) for c in p)) for p in polygon]
    depth, sigma, cost = np.zeros((Y, X)), np.zeros((Y, X)), np.full((Y, X), 5.)
    margin, zdot = np.full((Y, X), np.nan), np.full((Y, X), np.nan)
    for y in range(Y):
        for x in range(X):
            vec = sr.reconstruct(cam, float(x * prm["scale"] + prm["u0"]), float(y * prm["scale"] + prm["v0"]))
            if vec is None:
                continue
            zvec = sr.dot3(z, vec)
            zdot[y, x] = zvec
            if zvec < 1e-3:
                continue
            inside, worst = True, math.inf
            for i in range(len(poly)):
                normal = sr.cross3(poly[i], poly[(i + 1) % len(poly)])
                dn = sr.dot3(vec, normal)
                worst = min(worst, abs(dn) / (math.sqrt(sr.dot3(vec, vec)) * math.sqrt(sr.dot3(normal, normal))))
                if dn < 0:
                    inside = False
                    break
            margin[y, x] = worst
            if not inside:
                continue
            alpha = sr.dot3(t, z) / zvec
            v = tuple(c * alpha for c in vec)
            depth[y, x] = math.sqrt(sr.dot3(v, v))
            sigma[y, x] = 1.
    return depth, sigma, cost, margin, zdot


def compare(prm, depth, sigma, truth, sigma_max=10.):
    """analyzeError of one map: dict with counts (Ngt, Nmax, N), the terms of the three sums in the reference's column-major pixel
    order, the inlier mask and the histogram rows (diff, truth, sigma) it writes"""
    f32 = np.float32
    X, Y = prm["x_max"], prm["y_max"]
    d32, s32 = np.asarray(depth, np.float64).astype(f32), np.asarray(sigma, np.float64).astype(f32)   # toMat, sigmaToMat
    inl = np.zeros((Y, X), np.uint8)
    ngt = nmax = n = 0
    terms = dict(err=[], err2=[], dist=[])
    hist = []
    for x in range(X):
        for y in range(Y):
            t = f32(truth[y * prm["scale"] + prm["v0"], x * prm["scale"] + prm["u0"]])
            d, s = d32[y, x], s32[y, x]
            if t != 0:
                ngt += 1
            if t == 0 or d == 0:
                continue
            if t != t or d != d:
                continue
            nmax += 1
            terms["dist"].append(float(t))
            with np.errstate(over="ignore", invalid="ignore"):
                diff = f32(t - d)
            hist.append((diff, t, s))
            if float(s) > sigma_max or abs(diff) > s:
                continue
            inl[y, x] = 255
            terms["err"].append(float(diff))
            terms["err2"].append(float(diff) * float(diff))
            n += 1
    return dict(counts=(ngt, nmax, n), terms=terms, inliers=inl, hist=hist)


def figures(counts, sums):
    """what the reference prints and writes: err / N 1000, sqrt(err2 / N) 1000, 100 N / Nmax, dist / Nmax, N / Ngt; NaN where a
    denominator is 0"""
    ngt, nmax, n = counts
    err, err2, dist = sums
    div = lambda a, b: a / b if b else math.nan
    return (div(err, n) * 1000, math.sqrt(div(err2, n)) * 1000 if n else math.nan, 100 * div(n, nmax), div(dist, nmax), div(n, ngt))
