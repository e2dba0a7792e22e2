"""Plain numpy restatement of photometric bundle adjustment (include/visgeom_amd.h section 18) for the
dense_ba tests: the reference's ReprojectionCost (test/reconstruction/dense_ba_test.cpp:38-113) generalised by xi_base_cam, a
gradient selection, a depth prior and a grey sigma, on photometric_ref's geometry, bicubic sampler and projection; the exact
elimination of the diagonal depth block; and the trust-region rule of tests/lm6_ref.py applied to all K + m parameters.
Test infrastructure only; FP64 throughout (np.longdouble for the sums where a test asks for it)."""
import math

import numpy as np

from tests import lm6_ref
from tests import photometric_ref as pr

MIN_DEPTH, COORD_LIMIT = pr.MIN_DEPTH, pr.COORD_LIMIT
DEFAULTS = {"sigma_grey": 5., "prior_weight": 1., "grad_thresh": 250., "max_iterations": 150, "function_tolerance": 1e-6}
REFERENCE = {"sigma_grey": 255., "prior_weight": 0., "grad_thresh": 0.}   # dense_ba_test's own problem


def data_pack(cam, prm, img8, depth, sigma, grad_thresh=250., prior_weight=1.):
    """dict(idx int32 [m] (y x_max + x), val [m], dir [m, 3], d0 [m], s0 [m]) in raster order of the depth grid"""
    img = np.asarray(img8).astype(np.float32)
    h, w = img.shape
    gu, gv = pr.sobel(img)
    yy, xx = np.mgrid[0:prm["y_max"], 0:prm["x_max"]]
    u, v = xx * prm["scale"] + prm["u0"], yy * prm["scale"] + prm["v0"]
    inside = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    uc, vc = np.clip(u, 0, w - 1), np.clip(v, 0, h - 1)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(depth) & (depth >= MIN_DEPTH) & inside
    X, rec_ok = pr.reconstruct(cam, uc.astype(float), vc.astype(float))
    g2 = gu[vc, uc].astype(np.float64) ** 2 + gv[vc, uc].astype(np.float64) ** 2
    keep &= rec_ok & ~(g2 < grad_thresh)
    if sigma is None:
        sigma = np.zeros_like(depth)
    if prior_weight > 0:
        with np.errstate(invalid="ignore"):
            keep &= np.isfinite(sigma) & (sigma > 0)
    k = keep.ravel()
    X = X.reshape(-1, 3)[k]
    return {"idx": np.flatnonzero(k).astype(np.int32), "val": img[vc, uc].ravel()[k].astype(np.float64),
            "dir": X / np.linalg.norm(X, axis=1, keepdims=True), "d0": depth.ravel()[k].copy(), "s0": sigma.ravel()[k].copy()}


def evaluate(cam, xi_base_cam, pack, img, xi, depths, sigma_grey):
    """one frame: dict(res [m], jp [m, 6], jd [m], ok [m], u, v [m], eta [m], zn [m]: projectPoint's two test quantities)"""
    cam = tuple(map(float, cam))
    xi, xb = np.asarray(xi, float), np.asarray(xi_base_cam, float)
    Rb = pr.rotation_matrix(xb[3:])
    xc = pr.compose(xi, xb)
    Rinv = pr.rotation_matrix(-xc[3:])
    Xb = (depths[:, None] * pack["dir"]) @ Rb.T + xb[:3]
    X = (Xb - xc[:3]) @ Rinv.T
    pt, ok, P = pr.project(cam, X, jac=True)
    with np.errstate(invalid="ignore"):
        ok = ok & (np.abs(pt[:, 0]) <= COORD_LIMIT) & (np.abs(pt[:, 1]) <= COORD_LIMIT)
    us, vs = np.where(ok, pt[:, 0], 0.), np.where(ok, pt[:, 1], 0.)
    f, dfdr, dfdc = pr.bicubic(img, vs, us)
    grad = np.stack([dfdc, dfdr], -1)
    R21, R32, M = pr.rotation_matrix(-xi[3:]), pr.rotation_matrix(-xb[3:]), pr.inter_omega_rot(xi[3:])
    L11 = R32 @ R21
    L22 = L11 @ M
    L12 = -R32 @ pr.hat(xb[:3]) @ R21 @ M
    dfdX = np.einsum("ni,nij->nj", grad, P)
    H = np.zeros((X.shape[0], 3, 3))
    H[:, 0, 1], H[:, 0, 2], H[:, 1, 0], H[:, 1, 2], H[:, 2, 0], H[:, 2, 1] = -X[:, 2], X[:, 1], X[:, 2], -X[:, 0], -X[:, 1], X[:, 0]
    B = H @ L22 - L12
    jp = np.concatenate([-dfdX @ L11, np.einsum("ni,nij->nj", dfdX, B)], 1) / sigma_grey
    jd = np.einsum("ni,ni->n", dfdX, pack["dir"] @ (Rinv @ Rb).T) / sigma_grey
    alpha, beta = cam[0], cam[1]
    with np.errstate(all="ignore"):
        rho = np.sqrt(X[:, 2] ** 2 + beta * (X[:, 0] ** 2 + X[:, 1] ** 2))
        eta = alpha * rho + (1. - alpha) * X[:, 2]
        zn = X[:, 2] / eta
    return {"res": np.where(ok, (f - pack["val"]) / sigma_grey, 0.), "jp": np.where(ok[:, None], jp, 0.), "jd": np.where(ok, jd, 0.),
            "ok": ok, "u": pt[:, 0], "v": pt[:, 1], "eta": eta, "zn": zn}


class Problem:
    """the bundle adjustment of one key frame and F frames on the restatement"""

    def __init__(self, cam, prm, xi_base_cam, sigma_grey=5., prior_weight=1., grad_thresh=250., max_iterations=150, function_tolerance=1e-6):
        self.cam, self.prm, self.xbc = tuple(map(float, cam)), prm, np.asarray(xi_base_cam, float)
        self.sigma_grey, self.lam, self.grad_thresh = float(sigma_grey), float(prior_weight), float(grad_thresh)
        self.max_iterations, self.ftol = max_iterations, function_tolerance
        self.pack = self.frames = None

    def set_base(self, img8, depth, sigma):
        self.depth_map, self.sigma_map = depth, sigma
        self.pack = data_pack(self.cam, self.prm, img8, depth, sigma, self.grad_thresh, self.lam)

    def set_frames(self, imgs8):
        self.frames = [np.asarray(im).astype(np.float32) for im in imgs8]

    @property
    def prior_scale(self):
        return self.lam / self.pack["s0"] if self.lam > 0 else np.zeros(len(self.pack["s0"]))

    def rows(self, xi, depths=None):
        """dict(res [F, m], jp [F, m, 6], jd [F, m], ok [F, m], p [m] the prior rows, a [m], gd [m], cost, frames: the per-frame
        dicts of evaluate)"""
        xi = np.asarray(xi, float).reshape(-1, 6)
        d = self.pack["d0"] if depths is None else np.asarray(depths, float)
        fr = [evaluate(self.cam, self.xbc, self.pack, img, x, d, self.sigma_grey) for img, x in zip(self.frames, xi)]
        out = {k: np.stack([f[k] for f in fr]) for k in ("res", "jp", "jd", "ok")}
        ps = self.prior_scale
        out["p"] = ps * (d - self.pack["d0"])
        out["a"] = (out["jd"] ** 2).sum(0) + ps * ps
        out["gd"] = (out["jd"] * out["res"]).sum(0) + ps * out["p"]
        out["cost"] = 0.5 * float((out["res"] ** 2).sum()) + 0.5 * float(out["p"] @ out["p"])
        out["frames"], out["depths"] = fr, d
        return out

    @staticmethod
    def normal(r, dtype=np.float64):
        """(H_pp [K, K] block diagonal, g_p [K], W [m, K] the stack of J_pose[f] jd[f]) in dtype"""
        F, m = r["res"].shape
        jp, jd, res = r["jp"].astype(dtype), r["jd"].astype(dtype), r["res"].astype(dtype)
        H, g = np.zeros((6 * F, 6 * F), dtype), np.zeros(6 * F, dtype)
        for f in range(F):
            H[6 * f:6 * f + 6, 6 * f:6 * f + 6] = jp[f].T @ jp[f]
            g[6 * f:6 * f + 6] = jp[f].T @ res[f]
        W = np.concatenate([jp[f] * jd[f][:, None] for f in range(F)], 1)
        return H, g, W

    @staticmethod
    def reduce(r, mu, dtype=np.float64):
        """(S [K, K], rhs [K], D_p [K], e [m]) of the rows r under mu"""
        H, g, W = Problem.normal(r, dtype)
        a, gd = r["a"].astype(dtype), r["gd"].astype(dtype)
        e = a + dtype(mu) * np.clip(a, lm6_ref.DIAG_MIN, lm6_ref.DIAG_MAX)
        Dp = np.clip(np.diag(H), lm6_ref.DIAG_MIN, lm6_ref.DIAG_MAX)
        S = H + dtype(mu) * np.diag(Dp) - (W / e[:, None]).T @ W
        return S, g - (W / e[:, None]).T @ gd, Dp, e

    @staticmethod
    def back_substitute(r, mu, dp, dtype=np.float64):
        """(dd [m], tail [5]: sum D dd^2, g . dd, |dd|^2, |d|^2, max |g|) of the pose step dp"""
        _, _, W = Problem.normal(r, dtype)
        a, gd, d = r["a"].astype(dtype), r["gd"].astype(dtype), r["depths"].astype(dtype)
        D = np.clip(a, lm6_ref.DIAG_MIN, lm6_ref.DIAG_MAX)
        dd = -(gd + W @ np.asarray(dp, dtype)) / (a + dtype(mu) * D)
        return dd, np.array([(D * dd * dd).sum(), (gd * dd).sum(), (dd * dd).sum(), (d * d).sum(), np.abs(gd).max()], dtype)

    def cost(self, xi, depths):
        return self.rows(xi, depths)["cost"]

    def solve(self, xi_start):
        """the trust-region loop of lm6_ref on all K + m parameters: (xi [F, 6], depths [m], a [m] at the solution, report)"""
        x = np.asarray(xi_start, float).reshape(-1)
        d = self.pack["d0"].copy()
        r = self.rows(x, d)
        rep = {"iterations": 0, "initial_cost": r["cost"], "termination": lm6_ref.TERM_NO_CONVERGENCE}
        radius, dec = lm6_ref.RADIUS0, 2.
        while rep["iterations"] < self.max_iterations:
            rep["iterations"] += 1
            mu = 1. / radius
            S, rhs, Dp, _ = self.reduce(r, mu)
            _, g, _ = self.normal(r)
            step_ok = True
            try:
                L = np.linalg.cholesky(S)
                dp = -np.linalg.solve(L.T, np.linalg.solve(L, rhs))
                dd, tail = self.back_substitute(r, mu, dp)
                step_ok = bool(np.isfinite(dp).all() and np.isfinite(tail[:3]).all())
            except np.linalg.LinAlgError:
                step_ok = False
            success = False
            if step_ok:
                rc = self.rows(x + dp, d + dd)
                cost, cost_c = r["cost"], rc["cost"]
                model_change = 0.5 * (mu * (float(Dp @ (dp * dp)) + tail[0]) - (float(g @ dp) + tail[1]))
                rho = (cost - cost_c) / model_change if model_change > 0. else -1.
                if max(np.abs(g).max(), tail[4]) <= lm6_ref.GTOL:
                    rep["termination"] = lm6_ref.TERM_GRADIENT
                    break
                if math.sqrt(float(dp @ dp) + tail[2]) <= lm6_ref.PTOL * (math.sqrt(float(x @ x) + tail[3]) + lm6_ref.PTOL):
                    rep["termination"] = lm6_ref.TERM_PARAMETER
                    break
                if model_change > 0. and math.isfinite(cost_c) and abs(cost - cost_c) <= self.ftol * cost:
                    rep["termination"] = lm6_ref.TERM_FUNCTION
                    break
                success = math.isfinite(cost_c) and rho > lm6_ref.MIN_REL_DECREASE
            if success:
                x, d, r = x + dp, d + dd, rc
                radius = min(radius / max(1. - (2. * rho - 1.) ** 3, 1. / 3.), lm6_ref.MAX_RADIUS)
                dec = 2.
            else:
                radius /= dec
                dec *= 2.
                if radius < lm6_ref.MIN_RADIUS:
                    rep["termination"] = lm6_ref.TERM_RADIUS
                    break
        rep["final_cost"] = r["cost"]
        return x.reshape(-1, 6), d, r["a"], rep
