"""Plain numpy restatement of the reference's sparse odometry for the sparse odometry tests: harrisCorners / descriptors
(src/localization/sparse_odom.cpp:161-238) on the exact integer response include/visgeom_amd.h section 13 defines, the
brute-force L1 matching with cross-check and threshold (:266-300), computeTransfSparse (:440-469) as the trust-region
Levenberg-Marquardt of tests/lm6_ref.py on the CPU checker's SparseReprojectCost plus photometric_ref's OdometryPrior,
the scoring and selection of ransacNPoints (:511-606), the refinement of feedData (:336-387) and feedData itself.  Written
from reading the reference, with the deviations of DESIGN.md section 9 ("Sparse visual odometry")."""
import math

import numpy as np

from oracle import vgo
from tests import lm6_ref
from tests import photometric_ref as pr

MAX_FEATURES, MATCH_THRESHOLD, NUM_RANSAC_POINTS, RANSAC_ITERATIONS, INLIER_THRESHOLD = 500, 2500., 2, 200, 1.
MAX_LM_ITERATIONS, PRIOR, OUTLIER_GATE = 25, (0.03, 0.5, 0.03, 0.05), 3.6
BORDER, PATCH, TRI_EPS = 7, 4, 1e-3
FTOL, GTOL, PTOL = pr.FTOL, pr.GTOL, pr.PTOL
STATUS_OK, STATUS_TOO_FEW, STATUS_NO_HYPOTHESIS = 0, 1, 2
STATE_FIRST, STATE_SKIPPED, STATE_ESTIMATED = 0, 1, 2


# ---- detection -------------------------------------------------------------------------------------------------------

def _reflect(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def response(img):
    """int64 [h][w]: R = 20 (a c - b^2) - (a + c)^2 of the 7 x 7 box sums of the Sobel products, BORDER_REFLECT_101"""
    I = np.asarray(img).astype(np.int64)
    h, w = I.shape
    um, up = _reflect(np.arange(w) - 1, w), _reflect(np.arange(w) + 1, w)
    vm, vp = _reflect(np.arange(h) - 1, h), _reflect(np.arange(h) + 1, h)
    dx = (I[vm][:, up] + 2 * I[:, up] + I[vp][:, up]) - (I[vm][:, um] + 2 * I[:, um] + I[vp][:, um])
    dy = (I[vp][:, um] + 2 * I[vp] + I[vp][:, up]) - (I[vm][:, um] + 2 * I[vm] + I[vm][:, up])

    def box(p):
        rows = sum(p[:, _reflect(np.arange(w) + d, w)] for d in range(-3, 4))
        return sum(rows[_reflect(np.arange(h) + d, h)] for d in range(-3, 4))

    a, b, c = box(dx * dx), box(dx * dy), box(dy * dy)
    return 20 * (a * c - b * b) - (a + c) * (a + c)


def maxima(resp):
    """raster indices of the strict 3 x 3 maxima inside the 7-pixel border"""
    h, w = resp.shape
    c = resp[BORDER:h - BORDER, BORDER:w - BORDER]
    ok = np.ones(c.shape, bool)
    for dv in (-1, 0, 1):
        for du in (-1, 0, 1):
            if du or dv:
                ok &= c > resp[BORDER + dv:h - BORDER + dv, BORDER + du:w - BORDER + du]
    v, u = np.nonzero(ok)
    return (v + BORDER) * w + (u + BORDER)


def detect(img, max_features=MAX_FEATURES):
    """(keypoints int32 [k][2] as (u, v) ordered by (R, raster index) descending, number of maxima)"""
    resp = response(img)
    idx = maxima(resp)
    order = sorted(idx.tolist(), key=lambda i: (int(resp.flat[i]), i), reverse=True)[:max_features]
    w = resp.shape[1]
    return np.array([[i % w, i // w] for i in order], np.int32).reshape(-1, 2), idx.size


def weights():
    g = 2. * np.arange(-PATCH, PATCH + 1) / PATCH
    return np.array([[math.exp(-0.5 * (x * x + y * y)) for x in g] for y in g])


def descriptors(img, kp):
    """float32 [k][81]: the 9 x 9 patch times the weights, the product in double rounded to float"""
    W = weights()
    out = np.zeros((len(kp), 81), np.float32)
    for k, (u, v) in enumerate(kp):
        out[k] = (W * np.asarray(img)[v - PATCH:v + PATCH + 1, u - PATCH:u + PATCH + 1].astype(np.float64)).ravel().astype(np.float32)
    return out


# ---- matching --------------------------------------------------------------------------------------------------------

def distance_matrix(d1, d2, order=range(81)):
    """L1 in FP64, the 81 terms added in patch order (or in `order`, for the check that the sums are exact)"""
    D = np.zeros((d1.shape[0], d2.shape[0]))
    a, b = d1.astype(np.float64), d2.astype(np.float64)
    for e in order:
        D += np.abs(a[:, e, None] - b[None, :, e])
    return D


def match(d1, d2, threshold=MATCH_THRESHOLD):
    """(pairs int32 [m][2] ordered by the first index, distance [m], D)"""
    if d1.shape[0] == 0 or d2.shape[0] == 0:
        return np.zeros((0, 2), np.int32), np.zeros(0), np.zeros((d1.shape[0], d2.shape[0]))
    D = distance_matrix(d1, d2)
    nn1, nn2 = D.argmin(1), D.argmin(0)   # argmin takes the lowest index on ties
    pairs = [(i, j) for i, j in enumerate(nn1) if nn2[j] == i and not D[i, j] > threshold]
    pairs = np.array(pairs, np.int32).reshape(-1, 2)
    return pairs, D[pairs[:, 0], pairs[:, 1]], D


def rays(cam, kp1, kp2, pairs):
    """(x1 [m][3], x2 [m][3], p2 [m][2], size [m]) of the matched key points"""
    a, b = kp1[pairs[:, 0]].astype(np.float64), kp2[pairs[:, 1]].astype(np.float64)
    X1, ok1 = pr.reconstruct(cam, a[:, 0], a[:, 1])
    X2, ok2 = pr.reconstruct(cam, b[:, 0], b[:, 1])
    return np.where(ok1[:, None], X1, 0.), np.where(ok2[:, None], X2, 0.), b, np.ones(len(pairs))


# ---- computeTransfSparse ---------------------------------------------------------------------------------------------

def normal(cam, xbc, x1, x2, p2, size, prior, xi):
    """(cost, J^T J, J^T r) of OdometryPrior + SparseReprojectCost at xi"""
    r, J = prior.evaluate(xi)
    cost, JtJ, g = 0.5 * float(r @ r), J.T @ J, J.T @ r
    if len(x1):
        rs, Js = vgo.sparse_reproject(vgo.MODEL_EUCM, cam, xbc, x1, x2, p2, size, xi)
        cost, JtJ, g = cost + 0.5 * float(rs @ rs), JtJ + Js.T @ Js, g + Js.T @ rs
    return cost, JtJ, g


def solve(cam, xbc, x1, x2, p2, size, xi_odom, max_iterations=MAX_LM_ITERATIONS, ftol=FTOL, ptol=PTOL, prior=PRIOR):
    """the trust-region loop of lm6_ref on this problem, from xi_odom: (xi, report dict)"""
    pri = pr.OdometryPrior(xi_odom, *prior)
    x1, x2, p2, size = (np.ascontiguousarray(a, dtype=np.float64) for a in (x1, x2, p2, size))
    f = lambda x: normal(cam, xbc, x1, x2, p2, size, pri, x)
    return lm6_ref.solve(f, xi_odom, max_iterations, ftol, GTOL, ptol)


# ---- scoring ---------------------------------------------------------------------------------------------------------

def camera_motion(xbc, xi):
    return pr.compose(pr.inverse_compose(xbc, xi), xbc)


def triangulate(xc, p, q, dtype=np.float64):
    """Triangulator(xc, 1e-3).computeRegular: the scale of every ray p [m][3] (triangulator.cpp:145-259, regDiv :114-128)"""
    R, t = pr.rotation_matrix(xc[3:]).astype(dtype), np.asarray(xc[:3], float).astype(dtype)
    p, q = np.asarray(p).astype(dtype), np.asarray(q).astype(dtype) @ R.T
    r = p + q
    tp, tq, tr, tt, rp, rq = p @ t, q @ t, r @ t, float(t @ t), (r * p).sum(1), (r * q).sum(1)
    delta, delta1 = tp * rq - tq * rp, tt * rq - tr * tq
    with np.errstate(all="ignore"):
        reg = np.where(delta1 == 0., 2. / TRI_EPS, 2. / TRI_EPS - delta / (delta1 * TRI_EPS * TRI_EPS))
        return np.where(delta > TRI_EPS * delta1, delta1 / delta, reg), delta > TRI_EPS * delta1


def score(cam, xbc, xi, x1, x2, p2, dtype=np.float64):
    """pixel distance of every match under the base motion xi, +inf where the triangulated point does not project.  With
    dtype = np.longdouble everything after the camera motion is evaluated in extended precision: the difference to the
    FP64 result is this function's own rounding error."""
    xc = camera_motion(xbc, xi)
    lam, _ = triangulate(xc, x1, x2, dtype)
    x1, p2 = np.asarray(x1).astype(dtype), np.asarray(p2).astype(dtype)
    X = (x1 * lam[:, None] - xc[:3].astype(dtype)) @ pr.rotation_matrix(xc[3:]).astype(dtype)   # R^T (x - t)
    pt, ok = pr.project(tuple(dtype(c) for c in cam), X)
    with np.errstate(all="ignore"):
        return np.where(ok, np.sqrt(((p2 - pt) ** 2).sum(1)), np.inf)


# ---- the library's own draw ------------------------------------------------------------------------------------------

class Draw:
    """include/visgeom_amd.h section 13, vg_sparse_odom_draw_samples: xorshift64* from the seed 0x9E3779B97F4A7C15, one state
    per handle; a table is the head of a Fisher-Yates shuffle of an index vector that persists while m stays the same"""

    def __init__(self):
        self.state, self.perm = 0x9E3779B97F4A7C15, []

    def next(self):
        x = self.state
        x ^= x >> 12
        x ^= (x << 25) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 27
        self.state = x
        return (x * 0x2545F4914F6CDD1D) & 0xFFFFFFFFFFFFFFFF

    def table(self, m, iterations=RANSAC_ITERATIONS, points=NUM_RANSAC_POINTS):
        if len(self.perm) != m:
            self.perm = list(range(m))
        out = np.zeros((iterations, points), np.int32)
        for it in range(iterations):
            for p in range(points):
                j = p + self.next() % (m - p)
                self.perm[p], self.perm[j] = self.perm[j], self.perm[p]
                out[it, p] = self.perm[p]
        return out


# ---- ransac and feed -------------------------------------------------------------------------------------------------

def ransac(cam, xbc, x1, x2, p2, size, xi_odom, samples, num_points=NUM_RANSAC_POINTS):
    """dict(xi_incr, mask, best, inliers, kept, status, hypotheses [n][6], residuals [n][m], gate_err, gate_bound)"""
    xi_odom = np.asarray(xi_odom, float)
    m = len(x1)
    out = {"xi_incr": xi_odom.copy(), "mask": np.zeros(m, bool), "best": -1, "inliers": 0, "kept": 0, "status": STATUS_OK}
    if m < num_points:
        out["status"] = STATUS_TOO_FEW
        return out
    hyp = np.array([solve(cam, xbc, x1[s], x2[s], p2[s], size[s], xi_odom)[0] for s in samples])
    res = np.array([score(cam, xbc, xi, x1, x2, p2) for xi in hyp])
    out["hypotheses"], out["residuals"] = hyp, res
    counts = (res < INLIER_THRESHOLD).sum(1)
    best, count = -1, num_points
    for k, c in enumerate(counts):
        if c > count:
            best, count = k, int(c)
    if best < 0:
        out["status"] = STATUS_NO_HYPOTHESIS
        return out
    mask = res[best] < INLIER_THRESHOLD
    out.update(best=best, inliers=count, mask=mask)
    xi1, rep1 = solve(cam, xbc, x1[mask], x2[mask], p2[mask], size[mask], xi_odom)
    out["refine"] = (xi1, rep1)
    # the reprojection under the camera motion of the ODOMETRY, as the reference has it (sparse_odom.cpp:354-355)
    err = score(cam, xbc, xi_odom, x1[mask], x2[mask], p2[mask]) ** 2
    sigma_sq = 0.
    for e in err:   # in order, like the reference's loop
        sigma_sq += e
    sigma_sq /= (len(err) - 2.)
    keep = err < OUTLIER_GATE * sigma_sq
    sel = np.flatnonzero(mask)[keep]
    out.update(kept=int(keep.sum()), gate_err=err, gate_bound=OUTLIER_GATE * sigma_sq)
    out["xi_incr"], out["final"] = solve(cam, xbc, x1[sel], x2[sel], p2[sel], size[sel], xi_odom)
    return out


class SparseOdometry:
    """feedData on the restatement; samples_for(m) gives the sample table of a pair with m matches"""

    def __init__(self, cam, xbc, max_features=MAX_FEATURES, min_stereo_base=0.):
        self.cam, self.xbc = tuple(map(float, cam)), np.asarray(xbc, float)
        self.max_features, self.min_stereo_base = max_features, min_stereo_base
        self.kp = self.desc = self.odom = None
        self.xi_local, self.xi_incr = np.zeros(6), np.zeros(6)
        self.log = []

    def feed(self, img, xi_odom_new, samples):
        xi_odom_new = np.asarray(xi_odom_new, float)
        have = self.kp is not None and len(self.kp) > 0
        incr = pr.inverse_compose(self.odom, xi_odom_new) if self.odom is not None else xi_odom_new
        if have and np.linalg.norm(camera_motion(self.xbc, incr)[:3]) < self.min_stereo_base:
            return STATE_SKIPPED
        kp, _ = detect(img, self.max_features)
        desc = descriptors(img, kp)
        state = STATE_FIRST
        if have:
            state = STATE_ESTIMATED
            pairs, dist, D = match(self.desc, desc)
            x1, x2, p2, size = rays(self.cam, self.kp, kp, pairs)
            m = len(pairs)
            r = ransac(self.cam, self.xbc, x1, x2, p2, size, incr, np.asarray(samples) % max(m, 1))
            self.xi_incr = r["xi_incr"]
            self.xi_local = pr.compose(self.xi_local, self.xi_incr)
            self.log.append({"pairs": pairs, "distance": dist, "D": D, "ransac": r, "kp1": self.kp, "kp2": kp, "desc1": self.desc, "desc2": desc})
        self.kp, self.desc, self.odom = kp, desc, xi_odom_new
        return state
