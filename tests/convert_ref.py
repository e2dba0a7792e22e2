"""Reference of the conversion between camera models (include/visgeom_amd.h section 20) for the tests.

  * numpy, FP64: the unprojection of the five models in the order of operations of visgeom_amd/csrc/vg_unproject.hpp (restated
    below; Kannala-Brandt and double sphere are camera_models_ref.unproject, which has that order already), the model-to-model map,
    the fit's samples, residuals and Jacobian.  Projections: rectify_ref.project (EUCM / UCM / Mei, the reference's order) and
    camera_models_ref.project; the fit's rows of EUCM / UCM / Mei come from the CPU oracle's per-block Evaluate at the identity
    pose, those of Kannala-Brandt / double sphere from camera_models_ref.
  * mpmath, 50 digits: the unprojection of EUCM / UCM / Mei from the DEFINITION -- the point of the model's quadric (EUCM) or unit
    sphere (UCM, Mei) that projects onto the pixel, Mei's distortion inverted by mpmath.findroot -- not from the closed forms the
    header evaluates.

Order of operations (vg_unproject.hpp).  A NaN or infinite pixel fails; a ray that is not finite fails.  (mx, my) = ((u - u0) / fu,
(v - v0) / fv), r2 = mx mx + my my.
  EUCM  gamma = 1 - alpha; num = 1 - r2 alpha alpha beta; det = 1 - (alpha - gamma) beta r2; fails when det < 0;
        X = (mx, my, num / (gamma + alpha sqrt(det)))
  UCM   disc = 1 + r2 (1 - xi xi); fails when disc < 0; g = sqrt(disc); en = -g - xi r2; ed = xi xi r2 - 1;
        X = (mx, my, ed / (ed + xi en))
  Mei   k1 = ... = k5 = 0: UCM's statements.  Otherwise Newton in two dimensions on distort(m) = (mx, my) from m = (mx, my), at most
        20 steps: q = xx + yy, D = 1 + k1 q + k2 q q + k3 q q q, dD = k1 + 2 k2 q + 3 k3 q q,
        f = (x D + 2 k4 xy + k5 (q + 2 xx) - mx, y D + 2 k5 xy + k4 (q + 2 yy) - my),
        a0 = D + 2 xx dD + 2 k4 y + 6 k5 x, a1 = 2 xy dD + 2 k4 x + 2 k5 y, b1 = D + 2 yy dD + 2 k5 x + 6 k4 y,
        det = a0 b1 - a1 a1 (fails unless > 0), dx = (b1 f0 - a1 f1) / det, dy = (a0 f1 - a1 f0) / det, x -= dx, y -= dy (fails
        when not finite), settled when max(|dx|, |dy|) <= 1e-12 max(|x|, |y|); then UCM's statements on (x, y).
  unit ray  X / sqrt(x x + y y + z z); (0, 0, 0) where the pixel fails."""
import mpmath as mp
import numpy as np

from tests import camera_models_ref as cmr
from tests import rectify_ref

MODEL_ID = {"eucm": 0, "ucm": 1, "mei": 2, "kb": 4, "ds": 5}
K_OF = {"eucm": 6, "ucm": 5, "mei": 10, "kb": 8, "ds": 6}
NEWTON_STEPS, SETTLED = 20, 1e-12


# ------------------------------------------------------------------------------------------ numpy: unprojection
def _unified(xi, x, y):
    with np.errstate(all="ignore"):
        u2 = x * x + y * y
        disc = 1. + u2 * (1 - xi * xi)
        ok = ~(disc < 0)
        g = np.sqrt(np.where(ok, disc, 1.))
        en = -g - xi * u2
        ed = xi * xi * u2 - 1
        return np.stack([x, y, ed / (ed + xi * en)], -1), ok


def _mei_undistort(k, mx, my):
    """(x, y, ok): distort(x, y) = (mx, my) by the header's Newton iteration, element by element"""
    k1, k2, k3, k4, k5 = k
    x, y = mx.copy(), my.copy()
    ok = np.ones(mx.shape, bool)
    settled = np.zeros(mx.shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(NEWTON_STEPS):
            act = ok & ~settled
            if not act.any():
                break
            xx, xy, yy = x * x, x * y, y * y
            r2 = xx + yy
            D = 1. + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
            dD = k1 + 2 * k2 * r2 + 3 * k3 * r2 * r2
            dlx = 2. * k4 * xy + k5 * (r2 + 2. * xx)
            dly = 2. * k5 * xy + k4 * (r2 + 2. * yy)
            f0, f1 = x * D + dlx - mx, y * D + dly - my
            a0 = D + 2 * xx * dD + 2 * k4 * y + 6 * k5 * x
            a1 = 2 * xy * dD + 2 * k4 * x + 2 * k5 * y
            b1 = D + 2 * yy * dD + 2 * k5 * x + 6 * k4 * y
            det = a0 * b1 - a1 * a1
            folded = act & ~(det > 0)
            ok &= ~folded
            act &= ~folded
            dx, dy = (b1 * f0 - a1 * f1) / det, (a0 * f1 - a1 * f0) / det
            x = np.where(act, x - dx, x)
            y = np.where(act, y - dy, y)
            bad = act & ~(np.isfinite(x) & np.isfinite(y))
            ok &= ~bad
            act &= ~bad
            settled |= act & (np.fmax(np.abs(dx), np.abs(dy)) <= SETTLED * np.fmax(np.abs(x), np.abs(y)))
    return x, y, ok & settled


def unproject(model, p, uv):
    """rays [n, 3], NOT normalised (zeros where the pixel fails), ok [n]"""
    p, uv = np.asarray(p, float), np.atleast_2d(np.asarray(uv, float))
    fin = np.isfinite(uv).all(-1)
    safe = np.where(fin[:, None], uv, 0.)
    with np.errstate(all="ignore"):
        if model in ("kb", "ds"):
            X, ok = cmr.unproject(model, p, safe)
        else:
            fu, fv, u0, v0 = p[-4:]
            mx, my = (safe[:, 0] - u0) / fu, (safe[:, 1] - v0) / fv
            if model == "eucm":
                al, be = p[:2]
                r2 = mx * mx + my * my
                ga = 1. - al
                num = 1. - r2 * al * al * be
                det = 1 - (al - ga) * be * r2
                ok = ~(det < 0)
                X = np.stack([mx, my, num / (ga + al * np.sqrt(np.where(ok, det, 1.)))], -1)
            elif model == "ucm" or not np.any(p[1:6] != 0):
                X, ok = _unified(p[0], mx, my)
            else:
                x, y, ok = _mei_undistort(p[1:6], mx, my)
                X, ok2 = _unified(p[0], np.where(ok, x, 0.), np.where(ok, y, 0.))
                ok = ok & ok2
        ok = ok & fin & np.isfinite(X).all(-1)
    return np.where(ok[:, None], X, 0.), ok


def unproject_unit(model, p, uv):
    X, ok = unproject(model, p, uv)
    with np.errstate(all="ignore"):
        n = np.sqrt(X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1] + X[:, 2] * X[:, 2])
        ok = ok & (n > 0) & np.isfinite(n)
        return np.where(ok[:, None], X / np.where(ok, n, 1.)[:, None], 0.), ok


def domain_margin(model, p, uv):
    """the discriminant whose sign decides whether a finite pixel unprojects (> 0: it does): EUCM det, UCM / Mei disc at the
    DISTORTED point for pixels (the undistorted point moves with it at a rate near 1), double sphere 1 - (2 alpha - 1) r2, Kannala-Brandt
    d(theta_max) - rd with theta_max the first zero of d' in (0, pi] or pi.  +inf where the model has no boundary."""
    p, uv = np.asarray(p, float), np.atleast_2d(np.asarray(uv, float))
    fu, fv, u0, v0 = p[-4:]
    mx, my = (uv[:, 0] - u0) / fu, (uv[:, 1] - v0) / fv
    r2 = mx * mx + my * my
    if model == "eucm":
        return 1 - (2 * p[0] - 1) * p[1] * r2
    if model in ("ucm", "mei"):
        return 1. + r2 * (1 - p[0] * p[0])
    if model == "ds":
        return 1. - (2. * p[1] - 1.) * r2 if p[1] > 0.5 else np.full(r2.shape, np.inf)
    k1, k2, k3, k4 = p[:4]
    th = np.linspace(0, np.pi, 20001)
    t2 = th * th
    dp = 1. + t2 * (3. * k1 + t2 * (5. * k2 + t2 * (7. * k3 + t2 * (9. * k4))))
    neg = np.nonzero(~(dp > 0))[0]
    tm = th[neg[0]] if neg.size else np.pi
    dmax = tm * (1. + tm * tm * (k1 + tm * tm * (k2 + tm * tm * (k3 + tm * tm * k4))))
    return dmax - np.sqrt(r2)


# ------------------------------------------------------------------------------------------ numpy: projection, map
def project(model, p, X):
    """uv [n, 2], ok [n] in eval_corner's order"""
    p, X = np.asarray(p, float), np.atleast_2d(np.asarray(X, float))
    if model in ("kb", "ds"):
        return cmr.project(model, p, X)
    u, v, ok = rectify_ref.project(MODEL_ID[model], p, X[:, 0], X[:, 1], X[:, 2])
    return np.stack([u, v], -1), ok


def convert_maps(dst_model, dst_p, src_model, src_p, size, R=None):
    """what vg_convert_map computes: (map_x, map_y float32 [h, w], ok [h, w], uv float64 [h, w, 2])"""
    w, h = size
    R = np.eye(3) if R is None else np.asarray(R, float).reshape(3, 3)
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X, seen = unproject(dst_model, dst_p, np.stack([j.ravel(), i.ravel()], -1))
    Y = np.stack([R[k, 0] * X[:, 0] + R[k, 1] * X[:, 1] + R[k, 2] * X[:, 2] for k in range(3)], -1)
    uv, ok = project(src_model, src_p, Y)
    ok = (ok & seen).reshape(h, w)
    uv = uv.reshape(h, w, 2)
    with np.errstate(all="ignore"):
        mx = np.where(ok, uv[..., 0], -1.).astype(np.float32)
        my = np.where(ok, uv[..., 1], -1.).astype(np.float32)
    return mx, my, ok, uv


# ------------------------------------------------------------------------------------------ numpy: the fit
def fit_samples(src_model, src_p, size, grid, max_angle=np.pi):
    """(rays [kept, 3] unit, uv [kept, 2], dropped): the grid's pixels the source camera unprojects no further than max_angle from
    the axis, in raster order"""
    w, h = size
    gw, gh = grid
    a, b = np.meshgrid(np.arange(gw, dtype=np.float64), np.arange(gh, dtype=np.float64))
    uv = np.stack([((a + 0.5) * w / gw - 0.5).ravel(), ((b + 0.5) * h / gh - 0.5).ravel()], -1)
    X, ok = unproject_unit(src_model, src_p, uv)
    keep = ok & (np.arccos(np.clip(X[:, 2], -1., 1.)) <= max_angle)
    return X[keep], uv[keep], int((~keep).sum())


def default_start(src_model, src_p, dst_model):
    src_p = np.asarray(src_p, float)
    f0 = src_p[-4:-2] / ((1. + src_p[0]) if src_model in ("ucm", "mei", "ds") else 1.)
    c = src_p[-2:]
    head = {"eucm": [0.5, 1.], "ucm": [1.], "mei": [1., 0, 0, 0, 0, 0], "kb": [0., 0, 0, 0], "ds": [0., 0.5]}[dst_model]
    return np.concatenate([head, (2. if dst_model in ("ucm", "mei") else 1.) * f0, c])


def fit_residual_jacobian(model, p, rays, uv, want_jac=True):
    """(r [2n], J [2n, K] or None, ok [n]) of the samples at intrinsics p; a sample that does not project has zero rows"""
    p, rays, uv = np.asarray(p, float), np.asarray(rays, float), np.asarray(uv, float)
    n = rays.shape[0]
    if model in ("kb", "ds"):
        q, ok = cmr.project(model, p, rays)
        r = np.where(ok[:, None], q - uv, 0.).ravel()
        J = cmr.intrinsic_jacobian(model, p, rays).reshape(2 * n, K_OF[model]) if want_jac else None
        return r, J, ok
    from oracle import vgo

    res, jacs = vgo.eval_block(vgo.MODELS[model], [0], rays, uv, [p, np.zeros(6)], want_jac=want_jac,
                               jac_mask=[True, False] if want_jac else None)
    ok = ~np.any(res.reshape(n, 2) == cmr.BIG, axis=1)
    r = np.where(np.repeat(ok, 2), res, 0.)
    return r, (jacs[0] if want_jac else None), ok


def fit_cost_gradient(model, p, rays, uv):
    r, J, ok = fit_residual_jacobian(model, p, rays, uv)
    return 0.5 * float(r @ r), J.T @ r, ok


# ------------------------------------------------------------------------------------------ mpmath, 50 digits
mp.mp.dps = 50
mpf = mp.mpf


def mp_unproject(model, p, uv):
    """the unit ray through pixel uv of an EUCM / UCM / Mei camera as an mpf triple, or None outside the domain; from the
    definitions: the normalised point m (Mei: distort(m) = m_d solved by findroot), then the point of the projection surface above it"""
    p = [mpf(float(v)) for v in p]
    fu, fv, u0, v0 = p[-4:]
    x, y = (mpf(float(uv[0])) - u0) / fu, (mpf(float(uv[1])) - v0) / fv
    if model == "mei" and any(v != 0 for v in p[1:6]):
        k1, k2, k3, k4, k5 = p[1:6]
        mx, my = x, y

        def f(a, b):
            q = a * a + b * b
            D = 1 + k1 * q + k2 * q ** 2 + k3 * q ** 3
            return (a * D + 2 * k4 * a * b + k5 * (q + 2 * a * a) - mx, b * D + 2 * k5 * a * b + k4 * (q + 2 * b * b) - my)

        sol = mp.findroot(f, (mx, my), tol=mpf(10) ** -45)
        x, y = sol[0], sol[1]
    r2 = x * x + y * y
    if model == "eucm":
        # the surface z = (1 - alpha) z' + alpha sqrt(z'^2 + beta r^2) = 1 scaled: X = (x, y, z) with
        # alpha sqrt(z^2 + beta r2) + (1 - alpha) z = 1
        al, be = p[0], p[1]
        if 1 - (2 * al - 1) * be * r2 < 0:
            return None
        if al == 0:
            z = mpf(1)
        else:
            # alpha^2 (z^2 + beta r2) = (1 - (1 - alpha) z)^2, the root with 1 - (1 - alpha) z >= 0
            A, B, C = al * al - (1 - al) ** 2, 2 * (1 - al), al * al * be * r2 - 1
            if A == 0:
                z = -C / B
            else:
                disc = mp.sqrt(B * B - 4 * A * C)
                roots = [(-B + disc) / (2 * A), (-B - disc) / (2 * A)]
                good = [zz for zz in roots if 1 - (1 - al) * zz >= 0 and (al <= mpf(1) / 2 or zz >= (al - 1) / (2 * al - 1) - mpf(10) ** -40)]
                z = max(good)
        ray = (x, y, z)
    else:
        xi = p[0]
        disc = 1 + (1 - xi * xi) * r2
        if disc < 0:
            return None
        eta = (xi + mp.sqrt(disc)) / (r2 + 1)   # the point of the unit sphere: (eta x, eta y, eta - xi)
        ray = (eta * x, eta * y, eta - xi)
    n = mp.sqrt(sum(c * c for c in ray))
    return tuple(c / n for c in ray)
