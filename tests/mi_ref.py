"""Plain numpy restatement of the reference's mutual-information localization for the MI tests: MutualInformation::Evaluate with
computeShares / computeShareDerivative / computeHist / computeHist2d / reduceHist and MutualInformationOdom
(src/localization/cost_function_mi.cpp), at the settings of ScalePhotometric::computePoseMI (src/localization/photometric.cpp:
260-385: 8 bins, valMax 255), on the pyramids, data packs, EUCM projection, bicubic interpolator and CameraJacobian of
tests/photometric_ref.py.  Every sum runs over the points in point order, like the reference's loops (numpy's add.at and cumsum
are sequential).  Ceres' GradientProblemSolver is replaced by the BFGS that include/visgeom_amd.h describes for
vg_mi_compute_pose; Bfgs below is that algorithm written a second time, not a binding of the library's.  Written
from reading the reference, with the deviations of DESIGN.md section 9 ("Mutual-information localization")."""
import math

import numpy as np

from tests import photometric_ref as pr

NUM_BINS, VAL_MAX = 8, 255.
HIST_STEP = VAL_MAX / (NUM_BINS - 1)
FTOL, GTOL, MAX_ITERATIONS = 1e-2, 1e-3, 50          # computePoseMI's options; the iteration cap is Ceres' default
C1, C2, MAX_SEARCH_EVALS = 1e-4, 0.9, 20
DAMPING = 0.0002
TERM_FUNCTION, TERM_GRADIENT, TERM_NO_CONVERGENCE, TERM_FAILURE = 0, 1, 3, 5


def remap(img8):
    """the grey-level change of the tests' second pass: 0.55 g + 40 + 15 sin(g / 40), rounded to uint8"""
    g = np.asarray(img8).astype(np.float64)
    return np.clip(np.round(0.55 * g + 40. + 15. * np.sin(g / 40.)), 0, 255).astype(np.uint8)


# ---- histograms ----------------------------------------------------------------------------------------------------

def shares(val):
    """computeShares for an array: (idx1, idx2 (-1: none), share)"""
    sv = np.asarray(val, float) / HIST_STEP
    r = pr.c_round(sv)
    tail = np.abs(r - sv)
    inside = (r >= 0) & (r < NUM_BINS)
    idx1 = np.clip(r, 0, NUM_BINS - 1)
    share = np.where(inside, 1. - 2 * tail * tail, 0.)
    up, down = inside & (sv > r) & (r < NUM_BINS - 1), inside & (sv < r) & (r > 0)
    idx2 = np.where(up, idx1 + 1, np.where(down, idx1 - 1, -1))
    return idx1, idx2, share


def share_derivative(val):
    """computeShareDerivative for an array: (idx1, idx2, der)"""
    sv = np.asarray(val, float) / HIST_STEP
    r = pr.c_round(sv)
    tail = np.abs(r - sv)
    idx1, idx2, _ = shares(val)
    der = 4 * tail / HIST_STEP
    der = np.where(idx2 == -1, 0., np.where(idx2 > idx1, -der, der))
    return idx1, idx2, der


def hist(val):
    """computeHist: the points in order; with a neighbour the neighbour's share is added first"""
    val = np.asarray(val, float)
    inc = 1. / len(val)
    i1, i2, s = shares(val)
    two = i2 != -1
    bins = np.stack([np.where(two, i2, i1), i1], 1)
    w = np.stack([np.where(two, inc * (1 - s), inc), np.where(two, inc * s, 0.)], 1)
    out = np.zeros(NUM_BINS)
    np.add.at(out, bins.ravel(), w.ravel())   # sequential, in index order
    return out


def hist2d(val1, val2):
    """computeHist2d, its four cases with the reference's products: flat [idx2 * 8 + idx1], the first axis is val1's"""
    val1, val2 = np.asarray(val1, float), np.asarray(val2, float)
    inc = 1. / len(val1)
    i11, i12, s1 = shares(val1)
    i21, i22, s2 = shares(val2)
    a, b = i12 != -1, i22 != -1
    both, only1, only2, none = a & b, a & ~b, ~a & b, ~a & ~b
    w = np.zeros((len(val1), 4))
    w[both] = np.stack([inc * s1 * s2, inc * (1 - s1) * s2, inc * (1 - s2) * s1, inc * (1 - s1) * (1 - s2)], 1)[both]
    w[only1, :2] = np.stack([s1 * inc, (1 - s1) * inc], 1)[only1]
    w[only2, 0], w[only2, 2] = (inc * s2)[only2], ((1 - s2) * inc)[only2]
    w[none, 0] = inc
    c12, c22 = np.where(a, i12, i11), np.where(b, i22, i21)   # an unused slot adds 0. to a bin the point has anyway
    bins = np.stack([i21 * NUM_BINS + i11, i21 * NUM_BINS + c12, c22 * NUM_BINS + i11, c22 * NUM_BINS + c12], 1)
    out = np.zeros(NUM_BINS * NUM_BINS)
    np.add.at(out, bins.ravel(), w.ravel())
    return out


def reduce_hist(h12):
    """reduceHist: std::accumulate over each row of eight"""
    out = np.zeros(NUM_BINS)
    for i2 in range(NUM_BINS):
        acc = 0.
        for i1 in range(NUM_BINS):
            acc += h12[i2 * NUM_BINS + i1]
        out[i2] = acc
    return out


# ---- the cost ------------------------------------------------------------------------------------------------------

def project_slack(cam, X):
    """how far projectPoint's decision is from its thresholds: min(|eta - 1e-3|, |z / eta - (alpha - 1) / (2 alpha - 1)|)"""
    alpha, beta = cam[0], cam[1]
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    eta = alpha * np.sqrt(z * z + beta * (x * x + y * y)) + (1. - alpha) * z
    slack = np.abs(eta - 1e-3)
    if alpha > 0.5:
        with np.errstate(all="ignore"):
            slack = np.minimum(slack, np.abs(z / eta - (alpha - 1.) / (alpha + alpha - 1.)))
    return slack


def evaluate_mi(loc, scale_idx, xi, target=0, want_grad=True, reverse=False):
    """MutualInformation::Evaluate on the Localizer's pack and target level: dict(values [m] (valVec2), ok [m] (projectPoint),
    slack [m] (project_slack), hist [64], hist1 [8], hist2 [8], logv [64], cost, and with want_grad gradient [6] and terms
    [m, 6], the per-point dMIdf * dfdxi).  reverse: the gradient summed in reversed point order, for the tests' sensitivity
    record."""
    xi = np.asarray(xi, float)
    pack, img = loc.packs[scale_idx], loc.targets[target][scale_idx][0]
    inv = 1. / float(1 << scale_idx)
    m = len(pack["val"])
    inc = 1. / m
    xc = pr.compose(xi, loc.xbc)
    X = (pack["cloud"] - xc[:3]) @ pr.rotation_matrix(-xc[3:]).T
    pt, ok, P = pr.project(loc.cam, X, jac=True)
    with np.errstate(invalid="ignore"):
        ok = ok & (np.abs(pt[:, 0]) <= pr.COORD_LIMIT) & (np.abs(pt[:, 1]) <= pr.COORD_LIMIT)
    u, v = np.where(ok, pt[:, 0], 0.), np.where(ok, pt[:, 1], 0.)
    f, dfdr, dfdc = pr.bicubic(img, v * inv, u * inv)
    val2 = np.where(ok, f, 0.)   # a point that fails to project keeps 0 and is still counted
    h12 = hist2d(pack["val"], val2)
    h2, h1 = reduce_hist(h12), hist(pack["val"])
    logv, cost = np.zeros(NUM_BINS * NUM_BINS), 0.
    for i2 in range(NUM_BINS):
        for i1 in range(NUM_BINS):
            p12 = h12[i2 * NUM_BINS + i1]
            if p12 > 0:
                logv[i2 * NUM_BINS + i1] = math.log(p12 / (h2[i2] * h1[i1]))
                cost -= p12 * logv[i2 * NUM_BINS + i1]
    out = {"values": val2, "ok": ok, "slack": project_slack(loc.cam, X), "hist": h12, "hist1": h1, "hist2": h2, "logv": logv, "cost": cost}
    if not want_grad:
        return out
    grad = np.where(ok[:, None], np.stack([dfdc * inv, dfdr * inv], -1), 0.)
    R21, R32, M = pr.rotation_matrix(-xi[3:]), pr.rotation_matrix(-loc.xbc[3:]), pr.inter_omega_rot(xi[3:])
    L11 = R32 @ R21
    L22 = L11 @ M
    L12 = -R32 @ pr.hat(loc.xbc[:3]) @ R21 @ M
    dfdX = np.einsum("ni,nij->nj", grad, np.where(ok[:, None, None], P, 0.))
    H = np.zeros((m, 3, 3))
    H[:, 0, 1], H[:, 0, 2], H[:, 1, 0], H[:, 1, 2], H[:, 2, 0], H[:, 2, 1] = -X[:, 2], X[:, 1], X[:, 2], -X[:, 0], -X[:, 1], X[:, 0]
    dfdxi = np.concatenate([-dfdX @ L11, np.einsum("ni,nij->nj", dfdX, H @ L22 - L12)], 1)
    i21, i22, dPdf = share_derivative(val2)
    i11, i12, s1 = shares(pack["val"])
    c12, c22 = np.where(i12 != -1, i12, i11), np.where(i22 != -1, i22, i21)
    four = logv[i21 * NUM_BINS + i11] * s1 + logv[i21 * NUM_BINS + c12] * (1 - s1) - logv[c22 * NUM_BINS + i11] * s1 - logv[c22 * NUM_BINS + c12] * (1 - s1)
    two = logv[i21 * NUM_BINS + i11] - logv[c22 * NUM_BINS + i11]
    dMIdP = np.where(i22 != -1, np.where(i12 != -1, four, two), 0.)
    terms = (dMIdP * inc * dPdf)[:, None] * dfdxi
    out["terms"] = terms
    out["gradient"] = -np.cumsum(terms[::-1] if reverse else terms, axis=0)[-1]   # dMIdxi -= dMIdf * dfdxi, point after point
    return out


# ---- the odometry term ---------------------------------------------------------------------------------------------

class MiOdometry:
    """MutualInformationOdom's constructor and the two lines its Evaluate adds (cost_function_mi.cpp:292-368)"""

    def __init__(self, xi_odom, xi_prior, err_v=0.1, err_w=0.01, lambda_t=0.01, lambda_r=0.01):
        xi_odom, self.prior = np.asarray(xi_odom, float), np.asarray(xi_prior, float)
        delta, l = xi_odom[5], float(np.linalg.norm(xi_odom[:3]))
        s, c = math.sin(delta / 2.), math.cos(delta / 2.)
        dfdu = np.array([[s, -l / 2. * c], [c, l / 2. * s], [0., 1.]])
        Cu = np.diag([err_v * err_v * l * l, err_w * err_w * delta * delta])
        Ci = np.linalg.inv(dfdu @ Cu @ dfdu.T + np.diag([lambda_t ** 2, lambda_t ** 2, lambda_r ** 2]))
        C = np.zeros((6, 6))
        C[:2, :2], C[:2, 5], C[5, :2], C[5, 5] = Ci[:2, :2], Ci[:2, 2], Ci[2, :2], Ci[2, 2]
        C[2, 2], C[3, 3], C[4, 4] = 1 / lambda_t ** 2, 1 / lambda_r ** 2, 1 / lambda_r ** 2
        M, R = pr.inter_omega_rot(self.prior[3:]), pr.rotation_matrix(-self.prior[3:])
        J = np.zeros((6, 6))
        J[:3, :3], J[:3, 3:], J[3:, :3], J[3:, 3:] = C[:3, :3] @ R, C[:3, 3:] @ R @ M, C[3:, :3] @ R, C[3:, 3:] @ R @ M
        self.C, self.J = 0.5 * C, J

    def evaluate(self, xi):
        """(added cost, added gradient [6])"""
        err = pr.inverse_compose(self.prior, xi)
        return DAMPING * float(err @ self.C @ err), DAMPING * (err @ self.J)


# ---- the solver ----------------------------------------------------------------------------------------------------

def _interpolate(a, fa, da, b, fb, db):
    """the minimiser of the cubic through both ends (Nocedal & Wright 3.59), a tenth of the interval away from either end, else
    the midpoint"""
    mid, lo, hi = 0.5 * (a + b), min(a, b), max(a, b)
    with np.errstate(all="ignore"):
        d1 = np.float64(da) + db - 3. * (np.float64(fa) - fb) / (a - b)
        rad = d1 * d1 - np.float64(da) * db
        if not rad >= 0. or not np.isfinite(rad):
            return mid
        d2 = math.copysign(1., b - a) * math.sqrt(rad)
        t = b - (b - a) * (db + d2 - d1) / (db - da + 2. * d2)
    if not np.isfinite(t) or t < lo + 0.1 * (hi - lo) or t > hi - 0.1 * (hi - lo):
        return mid
    return float(t)


def line_search(fun, x, f0, g0, d, alpha):
    """strong Wolfe (Nocedal & Wright 3.5 / 3.6): (alpha, f, g) or None after MAX_SEARCH_EVALS evaluations.  fun(x) is (f, g)
    or None for a trial that fails"""
    phi0, dphi0 = f0, float(g0 @ d)
    evals = 0

    def phi(a):
        xt = x + a * d
        r = fun(xt) if np.isfinite(xt).all() else None
        if r is None or not math.isfinite(r[0]) or not np.isfinite(r[1]).all():
            return math.inf, 0., None
        return r[0], float(r[1] @ d), r

    prev = (0., phi0, dphi0)
    lo = hi = None
    while lo is None:
        p, dp, r = phi(alpha)
        evals += 1
        if not p <= phi0 + C1 * alpha * dphi0 or (evals > 1 and p >= prev[1]):
            lo, hi = prev, (alpha, p, dp)
        elif abs(dp) <= -C2 * dphi0:
            return alpha, r[0], r[1]
        elif dp >= 0.:
            lo, hi = (alpha, p, dp), prev
        elif evals >= MAX_SEARCH_EVALS:
            return None
        else:
            prev, alpha = (alpha, p, dp), 2. * alpha
    while evals < MAX_SEARCH_EVALS:
        alpha = _interpolate(*lo, *hi)
        p, dp, r = phi(alpha)
        evals += 1
        if not p <= phi0 + C1 * alpha * dphi0 or p >= lo[1]:
            hi = (alpha, p, dp)
        else:
            if abs(dp) <= -C2 * dphi0:
                return alpha, r[0], r[1]
            if dp * (hi[0] - lo[0]) >= 0.:
                hi = lo
            lo = (alpha, p, dp)
    return None


def bfgs(fun, x0, ftol=FTOL, gtol=GTOL, max_iterations=MAX_ITERATIONS):
    """(x, dict(iterations, initial_cost, final_cost, termination)): the inverse Hessian from the identity, first step length
    min(1, 1 / max|g|) and 1 afterwards, no update when s^T y <= 0"""
    x = np.asarray(x0, float).copy()
    f, g = fun(x)
    rep = {"iterations": 0, "initial_cost": f, "termination": TERM_NO_CONVERGENCE}
    H = np.eye(6)
    if np.abs(g).max() <= gtol:
        rep["termination"] = TERM_GRADIENT
    else:
        while rep["iterations"] < max_iterations:
            d = -H @ g
            if not g @ d < 0.:
                H, d = np.eye(6), -g
            found = line_search(fun, x, f, g, d, min(1., 1. / np.abs(g).max()) if rep["iterations"] == 0 else 1.)
            if found is None:
                rep["termination"] = TERM_FAILURE
                break
            alpha, fn, gn = found
            xn = x + alpha * d
            s, y = xn - x, gn - g
            sy = float(s @ y)
            if sy > 0.:
                rho, Hy = 1. / sy, H @ y
                H = H - rho * (np.outer(s, Hy) + np.outer(Hy, s)) + (rho * rho * float(y @ Hy) + rho) * np.outer(s, s)
            f_old, x, f, g = f, xn, fn, gn
            rep["iterations"] += 1
            if np.abs(g).max() <= gtol:
                rep["termination"] = TERM_GRADIENT
                break
            if abs(f - f_old) <= ftol * abs(f_old):
                rep["termination"] = TERM_FUNCTION
                break
    rep["final_cost"] = f
    return x, rep


def compute_pose_mi(loc, xi, target=0, xi_odom=None, ftol=FTOL, gtol=GTOL, max_iterations=MAX_ITERATIONS):
    """computePoseMI: coarsest scale first, an empty pack skipped; (xi, [report per scale, index = scale]).  xi_odom selects
    MutualInformationOdom with the start pose as its prior."""
    xi = np.asarray(xi, float)
    odom = MiOdometry(xi_odom, xi) if xi_odom is not None else None
    reports = [None] * loc.num_scales
    for s in range(loc.num_scales - 1, -1, -1):
        if len(loc.packs[s]["val"]) == 0:
            reports[s] = {"iterations": 0, "initial_cost": 0., "final_cost": 0., "termination": TERM_NO_CONVERGENCE}
            continue

        def fun(x, s=s):
            e = evaluate_mi(loc, s, x, target)
            if odom is None:
                return e["cost"], e["gradient"]
            c, g = odom.evaluate(x)
            return e["cost"] + c, e["gradient"] + g

        xi, reports[s] = bfgs(fun, xi, ftol, gtol, max_iterations)
    return xi, reports
