"""numpy restatement of the rectification semantics (include/visgeom_amd.h section 7) that the GPU tests compare against:
the pinhole -> camera maps in FP64 in the reference's order, and the float32 bilinear remap with a constant border."""
import numpy as np


def pinhole_rays(pinhole):
    """pinhole.h:40-49 for every pixel (j, i) of a [height, width] grid -> X0, X1 (X2 = 1)"""
    w, h, u0, v0, f = pinhole
    j, i = np.meshgrid(np.arange(int(w), dtype=np.float64), np.arange(int(h), dtype=np.float64))
    return (j - u0) / f, (i - v0) / f


def transform(R, t, X0, X1):
    """R X + t with X = (X0, X1, 1), every row summed left to right"""
    x = R[0, 0] * X0 + R[0, 1] * X1 + R[0, 2] * 1. + t[0]
    y = R[1, 0] * X0 + R[1, 1] * X1 + R[1, 2] * 1. + t[1]
    z = R[2, 0] * X0 + R[2, 1] * X1 + R[2, 2] * 1. + t[2]
    return x, y, z


def project(model, p, x, y, z):
    """projectPoint of EUCM (0) / UCM (1) / Mei (2), vectorised, in the order of eucm.h / ucm.h / mei.h -> (u, v, ok)"""
    with np.errstate(all="ignore"):
        if model == 0:
            alpha, beta, fu, fv, u0, v0 = p
            rho = np.sqrt(z * z + beta * (x * x + y * y))
            eta = alpha * rho + (1. - alpha) * z
            ok = ~(eta < 1e-3)
            if alpha > 0.5:
                C = (alpha - 1.) / (alpha + alpha - 1.)
                ok &= ~(z / eta < C)
            return fu * (x / eta) + u0, fv * (y / eta) + v0, ok
        rho = np.sqrt(z * z + x * x + y * y)
        d = 1. / (z + p[0] * rho)
        xn, yn = x * d, y * d
        if model == 1:
            _, fu, fv, u0, v0 = p
            return fu * xn + u0, fv * yn + v0, np.ones(x.shape, bool)
        _, k1, k2, k3, k4, k5, fu, fv, u0, v0 = p
        xx, xy, yy = xn * xn, xn * yn, yn * yn
        r2 = xx + yy
        D = 1. + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
        dx = 2. * k4 * xy + k5 * (r2 + 2. * xx)
        dy = 2. * k5 * xy + k4 * (r2 + 2. * yy)
        return fu * (xn * D + dx) + u0, fv * (yn * D + dy) + v0, np.ones(x.shape, bool)


def rectify_maps(model, intr, pinhole, R, t):
    """the maps vg_rectify_map computes: float32 [height, width] each, (-1, -1) where the projection fails"""
    X0, X1 = pinhole_rays(pinhole)
    u, v, ok = project(model, np.asarray(intr, np.float64), *transform(R, t, X0, X1))
    return np.where(ok, u, -1.).astype(np.float32), np.where(ok, v, -1.).astype(np.float32)


def remap(images, map_x, map_y, fill):
    """vg_remap on the host: images [N, H, W, C] uint8 / float32, maps float32 of any shape S -> [N, *S, C] of the images' dtype.
    Every operation in float32, in the order the kernel evaluates it."""
    images = np.asarray(images)
    N, H, W, C = images.shape
    f32 = np.float32
    mx, my = np.asarray(map_x, f32), np.asarray(map_y, f32)
    fillv = f32(fill)
    inside = (mx > f32(-1)) & (mx < f32(W)) & (my > f32(-1)) & (my < f32(H))   # False for NaN
    fx = np.floor(np.where(inside, mx, f32(0)))
    fy = np.floor(np.where(inside, my, f32(0)))
    ax, ay = (np.where(inside, mx, f32(0)) - fx).astype(f32), (np.where(inside, my, f32(0)) - fy).astype(f32)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    src = images.astype(f32)

    def tap(xs, ys):
        valid = inside & (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
        vals = src[:, np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1), :]   # [N, *S, C]
        return np.where(valid[None, ..., None], vals, fillv)

    p00, p01, p10, p11 = tap(x0, y0), tap(x1, y0), tap(x0, y1), tap(x1, y1)
    a_x, a_y = ax[None, ..., None], ay[None, ..., None]
    bx, by = (f32(1) - a_x).astype(f32), (f32(1) - a_y).astype(f32)
    v = by * (bx * p00 + a_x * p01) + a_y * (bx * p10 + a_x * p11)
    v = np.where(inside[None, ..., None], v, fillv).astype(f32)
    if images.dtype == np.uint8:
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return v
