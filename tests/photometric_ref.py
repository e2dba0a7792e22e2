"""Plain numpy restatement of the reference's photometric localizer for the photometric tests: BinaryScalSpace with gradients
(include/localization/scale_space.h), ScalePhotometric::initPhotometricData and computePose (src/localization/photometric.cpp:46-157),
PhotometricCostFunction::Evaluate with lossFunction / getUMapgin / getVMapgin (src/localization/local_cost_functions.cpp:35-210),
CameraJacobian::dfdxi (include/projection/jacobian.h:54-115), the localization OdometryPrior (local_cost_functions.cpp:393-493),
Ceres' BiCubicInterpolator over the reference's clamping Grid2D (include/ceres.h:48-69), and the trust-region Levenberg-Marquardt
of tests/lm6_ref.py (the rules DESIGN.md section 5.13 names).  Written from reading the reference, with the deviations of DESIGN.md section 9
("Photometric localization"); FP64 throughout except the pyramid, which is float32 like the reference's Mat32f."""
import math

import numpy as np

from tests import lm6_ref
from tests.lm6_ref import (DIAG_MAX, DIAG_MIN, FTOL, GTOL, MAX_RADIUS, MIN_RADIUS, MIN_REL_DECREASE, PTOL, RADIUS0,  # noqa: F401
                           TERM_FUNCTION, TERM_GRADIENT, TERM_NO_CONVERGENCE, TERM_PARAMETER, TERM_RADIUS)

GRAD_THRESH, DIST_MAX, GREY_MAX, LOSS_FACTOR, MIN_DEPTH, MARGIN_PIXELS = 250., 50., 240., 3., 0.25, 50.
COORD_LIMIT = 16777216.
MAX_ITERATIONS = 150   # the reference sets only the iteration cap; Ceres' defaults and the rule are lm6_ref's


# ---- geometry (geometry_core.h, quaternion.h, transformation.h) ----------------------------------------------------

def hat(v):
    return np.array([[0., -v[2], v[1]], [v[2], 0., -v[0]], [-v[1], v[0], 0.]])


def rotation_matrix(v):
    v = np.asarray(v, float)
    th = float(np.linalg.norm(v))
    if th < 1e-5:
        return np.eye(3) + hat(v)
    u = v / th
    return np.eye(3) + math.sin(th) * hat(u) + (1. - math.cos(th)) * (np.outer(u, u) - np.eye(3))


def sinc(x):
    return 1. if x == 0. else math.sin(x) / x


def inter_omega_rot(v):
    v = np.asarray(v, float)
    th = float(np.linalg.norm(v))
    if th < 1e-5:
        return np.eye(3) + hat(v / 2.)
    uh = hat(v / th)
    k1 = sinc(th / 2.)
    k1 = th / 2. * k1 * k1
    return np.eye(3) + k1 * uh + (1. - sinc(th)) * (uh @ uh)


def quat(rot):
    rot = np.asarray(rot, float)
    th = float(np.linalg.norm(rot))
    if th < 1e-6:
        return np.array([rot[0] / 2., rot[1] / 2., rot[2] / 2., 1.])
    return np.append(rot / th * math.sin(th / 2.), math.cos(th / 2.))


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def quat_rotate(q, v):
    x, y, z, w = q
    R = np.array([[-y * y - z * z, x * y - w * z, w * y + x * z], [w * z + x * y, -x * x - z * z, y * z - w * x],
                  [x * z - w * y, w * x + y * z, -x * x - y * y]])
    return 2. * (R @ np.asarray(v, float)) + np.asarray(v, float)


def quat_rotvec(q):
    s = float(np.linalg.norm(q[:3]))
    if s < 1e-5:
        return 2. * q[:3]
    th = 2. * math.atan2(s, q[3])
    th = th - 2. * math.pi if th > math.pi else (th + 2. * math.pi if th < -math.pi else th)
    return q[:3] / s * th


def compose(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    q1, q2 = quat(a[3:]), quat(b[3:])
    return np.concatenate([quat_rotate(q1, b[:3]) + a[:3], quat_rotvec(quat_mul(q1, q2))])


def inverse_compose(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    q1, q2 = quat(a[3:]), quat(b[3:])
    qi = np.array([-q1[0], -q1[1], -q1[2], q1[3]])
    return np.concatenate([quat_rotate(qi, b[:3] - a[:3]), quat_rotvec(quat_mul(qi, q2))])


# ---- EUCM (projection/eucm.h) --------------------------------------------------------------------------------------

def reconstruct(cam, u, v):
    """(X [..., 3], ok)"""
    alpha, beta, fu, fv, u0, v0 = cam
    xn, yn = (u - u0) / fu, (v - v0) / fv
    u2 = xn * xn + yn * yn
    gamma = 1. - alpha
    det = 1 - (alpha - gamma) * beta * u2
    ok = ~(det < 0)
    z = (1. - u2 * alpha * alpha * beta) / (gamma + alpha * np.sqrt(np.where(ok, det, 0.)))
    return np.stack([xn, yn, z], -1), ok


def project(cam, X, jac=False):
    """(pt [..., 2], ok[, dpdX [..., 2, 3]])"""
    alpha, beta, fu, fv, u0, v0 = cam
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    with np.errstate(all="ignore"):
        rho = np.sqrt(z * z + beta * (x * x + y * y))
        eta = alpha * rho + (1. - alpha) * z
        ok = ~(eta < 1e-3)
        if alpha > 0.5:
            ok &= ~(z / eta < (alpha - 1.) / (alpha + alpha - 1.))
        pt = np.stack([fu * (x / eta) + u0, fv * (y / eta) + v0], -1)
        if not jac:
            return pt, ok
        # d(x / eta) with d eta = (alpha beta x / rho, alpha beta y / rho, gamma + alpha z / rho)
        ex, ey, ez = alpha * beta * x / rho, alpha * beta * y / rho, (1. - alpha) + alpha * z / rho
        e2 = eta * eta
        J = np.stack([np.stack([fu * (eta - x * ex) / e2, -fu * x * ey / e2, -fu * x * ez / e2], -1),
                      np.stack([-fv * y * ex / e2, fv * (eta - y * ey) / e2, -fv * y * ez / e2], -1)], -2)
    return pt, ok, J


# ---- scale space ---------------------------------------------------------------------------------------------------

def down(img):
    """one step of BinaryScalSpace::propagate, the reference's loop: row v to min(round(v / 2.), rows - 1) (half away from
    zero), column u to min(u / 2, cols - 1), float32 sums in raster order, then * 0.25"""
    hp, wp = img.shape
    h, w = hp // 2, wp // 2
    out = np.zeros((h, w), np.float32)
    vs = np.minimum((np.arange(hp) + 1) // 2, h - 1)   # round(v / 2.) for v >= 0
    us = np.minimum(np.arange(wp) // 2, w - 1)
    for v in range(hp):       # source rows and columns in ascending order: the order the reference adds in
        for u0 in range(3):   # a target column has at most three sources: 2 us, 2 us + 1 and, in the last one, wp - 1
            cols = np.arange(w) * 2 + u0
            use = cols < wp
            use &= us[np.minimum(cols, wp - 1)] == np.arange(w)
            out[vs[v], use] = out[vs[v], use] + img[v, cols[use]]
    return out * np.float32(0.25)


def _reflect(i, n):
    i = np.abs(i)
    i = np.where(i >= n, 2 * n - 2 - i, i)
    return np.clip(i, 0, n - 1)


def sobel(img):
    """Sobel(CV_32F, 1, 0, 3, 1./8) and (0, 1) with BORDER_REFLECT_101, float32"""
    h, w = img.shape
    um, up = _reflect(np.arange(w) - 1, w), _reflect(np.arange(w) + 1, w)
    vm, vp = _reflect(np.arange(h) - 1, h), _reflect(np.arange(h) + 1, h)
    two, eighth = np.float32(2.), np.float32(0.125)
    du = img[:, up] - img[:, um]
    gu = ((du[vm] + two * du) + du[vp]) * eighth
    dv = img[vp] - img[vm]
    gv = ((dv[:, um] + two * dv) + dv[:, up]) * eighth
    return gu.astype(np.float32), gv.astype(np.float32)


def pyramid(img8, num_scales, gradients=True):
    """[(img, gu, gv)] per level, float32"""
    levels, cur = [], np.asarray(img8).astype(np.float32)
    for i in range(num_scales):
        if i:
            cur = down(cur)
        gu, gv = sobel(cur) if gradients else (None, None)
        levels.append((cur, gu, gv))
    return levels


# ---- the data pack -------------------------------------------------------------------------------------------------

def c_round(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)).astype(np.int64)


def data_pack(level, scale_idx, cam, prm, depth, xi_base_cam):
    """initPhotometricData: dict(idx int32 [m], val [m], cloud [m, 3], dropped_depth: gradient pixels the depth tests refuse)"""
    img, gu, gv = level
    h, w = img.shape
    g2 = gu.astype(np.float64) ** 2 + gv.astype(np.float64) ** 2
    vs, us = np.mgrid[0:h, 0:w]
    ub, vb = us * (1 << scale_idx), vs * (1 << scale_idx)
    xd, yd = c_round((ub - prm["u0"]) / prm["scale"]), c_round((vb - prm["v0"]) / prm["scale"])
    valid = (xd >= 0) & (xd < prm["x_max"]) & (yd >= 0) & (yd < prm["y_max"])
    d = np.where(valid, depth[np.clip(yd, 0, prm["y_max"] - 1), np.clip(xd, 0, prm["x_max"] - 1)], 0.)
    grad_ok = ~(g2 < GRAD_THRESH)
    depth_ok = ~((d > DIST_MAX) | (d == 0.))
    X, rec_ok = reconstruct(cam, ub.astype(float), vb.astype(float))
    keep = grad_ok & depth_ok & ~(img > GREY_MAX) & rec_ok & ~(d < MIN_DEPTH)
    keep = keep.ravel()   # raster order
    X = X.reshape(-1, 3)[keep]
    X = X / np.linalg.norm(X, axis=1, keepdims=True) * d.ravel()[keep, None]
    xb = np.asarray(xi_base_cam, float)
    cloud = X @ rotation_matrix(xb[3:]).T + xb[:3]
    return {"idx": np.flatnonzero(keep).astype(np.int32), "val": img.ravel()[keep].astype(np.float64), "cloud": cloud,
            "dropped_depth": int((grad_ok & ~depth_ok).sum())}


# ---- the cost ------------------------------------------------------------------------------------------------------

def _cubic(p0, p1, p2, p3, x):
    a = 0.5 * (-p0 + 3.0 * p1 - 3.0 * p2 + p3)
    b = 0.5 * (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3)
    c = 0.5 * (-p0 + p2)
    return p1 + x * (c + x * (b + x * a)), c + x * (2.0 * b + 3.0 * a * x)


def bicubic(img, r, c):
    """ceres::BiCubicInterpolator::Evaluate(r, c) over the clamping grid: (f, dfdr, dfdc), in double on the float samples"""
    h, w = img.shape
    row, col = np.floor(r).astype(np.int64), np.floor(c).astype(np.int64)
    fk, dk = [], []
    for k in range(4):
        rr = np.clip(row - 1 + k, 0, h - 1)
        p = [img[rr, np.clip(col - 1 + j, 0, w - 1)].astype(np.float64) for j in range(4)]
        f, d = _cubic(p[0], p[1], p[2], p[3], c - col)
        fk.append(f)
        dk.append(d)
    f, dfdr = _cubic(fk[0], fk[1], fk[2], fk[3], r - row)
    dfdc, _ = _cubic(dk[0], dk[1], dk[2], dk[3], r - row)
    return f, dfdr, dfdc


def margin_of(x, inv_scale, margin, size):
    xs = x * inv_scale
    return np.where(xs < margin, xs - margin, np.where(xs > size - margin - 1, xs - size + margin + 1, 0.))


def loss(x):
    s = 0.1 * np.where(x > 0, 1., -1.)
    arg = -np.abs(x) / LOSS_FACTOR
    e = np.where(arg > -5, np.exp(arg), 0.)
    return s * LOSS_FACTOR * (1. - e), 0.1 * e


def evaluate(cam, xi_base_cam, pack, target_level, scale_idx, xi, want_jac=True):
    """PhotometricCostFunction::Evaluate at pose xi: dict(res [m], jac [m, 6], u, v [m] the projections, err [m] the grey
    difference in front of the loss, state [m]: 0 a residual, 1 failed to project, 2 in the margin)"""
    xi = np.asarray(xi, float)
    scale = float(1 << scale_idx)
    inv, margin = 1. / scale, MARGIN_PIXELS / scale
    h, w = target_level.shape
    xc = compose(xi, xi_base_cam)
    X = (pack["cloud"] - xc[:3]) @ rotation_matrix(-xc[3:]).T
    pt, ok, P = project(cam, X, jac=True)
    with np.errstate(invalid="ignore"):
        ok &= (np.abs(pt[:, 0]) <= COORD_LIMIT) & (np.abs(pt[:, 1]) <= COORD_LIMIT)   # false for NaN
    u, v = np.where(ok, pt[:, 0], 0.), np.where(ok, pt[:, 1], 0.)
    inside = ok & (margin_of(u, inv, margin, w) == 0.) & (margin_of(v, inv, margin, h) == 0.)
    us, vs = np.where(inside, u, margin * scale), np.where(inside, v, margin * scale)
    f, dfdr, dfdc = bicubic(target_level, vs * inv, us * inv)
    rho, drho = loss(f - pack["val"])
    res = np.where(inside, rho, 0.)
    out = {"res": res, "u": pt[:, 0], "v": pt[:, 1], "err": f - pack["val"], "state": np.where(~ok, 1, np.where(inside, 0, 2))}
    if want_jac:
        grad = np.stack([dfdc * inv, dfdr * inv], -1)
        # CameraJacobian(camera, T12 = xi, T23 = xi_base_cam)
        xb = np.asarray(xi_base_cam, float)
        R21, R32, M = rotation_matrix(-xi[3:]), rotation_matrix(-xb[3:]), inter_omega_rot(xi[3:])
        L11 = R32 @ R21
        L22 = L11 @ M
        L12 = -R32 @ hat(xb[:3]) @ R21 @ M
        dfdX = np.einsum("ni,nij->nj", grad, P)
        # hat(X) as a batch
        H = np.zeros((X.shape[0], 3, 3))
        H[:, 0, 1], H[:, 0, 2], H[:, 1, 0], H[:, 1, 2], H[:, 2, 0], H[:, 2, 1] = -X[:, 2], X[:, 1], X[:, 2], -X[:, 0], -X[:, 1], X[:, 0]
        B = H @ L22 - L12
        jac = np.concatenate([-dfdX @ L11, np.einsum("ni,nij->nj", dfdX, B)], 1) * drho[:, None]
        out["jac"] = np.where(inside[:, None], jac, 0.)
    return out


def sums(res, jac):
    """(1/2 sum r^2, J^T J upper triangle row-major [21], J^T r [6])"""
    JtJ = jac.T @ jac
    return 0.5 * float(res @ res), JtJ[np.triu_indices(6)], jac.T @ res


# ---- the motion prior ----------------------------------------------------------------------------------------------

class OdometryPrior:
    """OdometryPrior(errV, errW, lambdaT, lambdaR, xiOdom) of local_cost_functions.cpp:393-493"""

    def __init__(self, xi_odom, err_v=0.03, err_w=0.03, lambda_t=0.01, lambda_r=0.01):
        self.xi = np.asarray(xi_odom, float)
        delta, l = self.xi[5], float(np.linalg.norm(self.xi[:3]))
        s, c = math.sin(delta / 2.), math.cos(delta / 2.)
        dfdu = np.array([[c, l / 2. * s], [-s, l / 2. * c], [0., 1.]])
        Cu = np.diag([err_v * err_v * l * l, err_w * err_w * delta * delta])
        Cx = dfdu @ Cu @ dfdu.T + np.diag([lambda_t ** 2, lambda_t ** 2, lambda_r ** 2])
        U = np.linalg.cholesky(np.linalg.inv(Cx)).T   # LLT::matrixU
        A = np.zeros((6, 6))
        A[1, 1], A[0, 0], A[0, 1], A[0, 5], A[1, 5] = U[0, 0], -U[1, 1], -U[0, 1], -U[1, 2], U[0, 2]
        A[2, 2], A[3, 3], A[4, 4], A[5, 5] = 1. / lambda_t, 1. / lambda_r, 1. / lambda_r, U[2, 2]
        M, R = inter_omega_rot(self.xi[3:]), rotation_matrix(-self.xi[3:])
        J = np.zeros((6, 6))
        J[:3, :3], J[:3, 3:], J[3:, 3:] = A[:3, :3] @ R, A[:3, 3:] @ R @ M, A[3:, 3:] @ R @ M
        self.A, self.J = A, J

    def evaluate(self, xi):
        return self.A @ inverse_compose(self.xi, xi), self.J


# ---- the solver ----------------------------------------------------------------------------------------------------

class Localizer:
    """ScalePhotometric on the restatement: one key frame, any number of targets"""

    def __init__(self, cam, prm, xi_base_cam, num_scales):
        self.cam, self.prm, self.xbc, self.num_scales = tuple(map(float, cam)), prm, np.asarray(xi_base_cam, float), num_scales
        self.base = self.packs = None
        self.targets = []

    def set_base(self, img8, depth):
        self.base = pyramid(img8, self.num_scales)
        self.packs = [data_pack(self.base[i], i, self.cam, self.prm, depth, self.xbc) for i in range(self.num_scales)]

    def set_targets(self, imgs8):
        self.targets = [pyramid(im, self.num_scales, gradients=False) for im in imgs8]

    def evaluate(self, scale_idx, xi, target=0, want_jac=True):
        return evaluate(self.cam, self.xbc, self.packs[scale_idx], self.targets[target][scale_idx][0], scale_idx, xi, want_jac)

    def normal(self, scale_idx, xi, target, prior):
        """(cost, JtJ [6, 6], Jtr [6]) of the photometric block and, if given, the prior block"""
        e = self.evaluate(scale_idx, xi, target)
        cost, JtJ, g = 0.5 * float(e["res"] @ e["res"]), e["jac"].T @ e["jac"], e["jac"].T @ e["res"]
        if prior is not None:
            r, J = prior.evaluate(xi)
            cost, JtJ, g = cost + 0.5 * float(r @ r), JtJ + J.T @ J, g + J.T @ r
        return cost, JtJ, g

    def cost(self, scale_idx, xi, target=0):
        r = self.evaluate(scale_idx, xi, target, want_jac=False)["res"]
        return 0.5 * float(r @ r)

    def solve_scale(self, scale_idx, xi, target=0, prior=None):
        """the trust-region loop of lm6_ref at one scale: (xi, dict(iterations, initial_cost, final_cost, termination))"""
        return lm6_ref.solve(lambda x: self.normal(scale_idx, x, target, prior), xi, MAX_ITERATIONS)

    def compute_pose(self, xi, target=0, xi_prior=None):
        """computePose: coarsest scale first; (xi, [report per scale, index = scale])"""
        prior = OdometryPrior(xi_prior) if xi_prior is not None else None
        reports = [None] * self.num_scales
        for s in range(self.num_scales - 1, -1, -1):
            xi, reports[s] = self.solve_scale(s, xi, target, prior)
        return xi, reports
