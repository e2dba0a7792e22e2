"""numpy restatement of the corner detector's pixel and per-candidate stages (include/visgeom_amd.h section 8; the reference's
src/calibration/corner_detector.cpp) that the GPU tests compare against: both blurs, the gradients and the response
(computeResponse), _avgVal, the local maxima, VAL_THRESH and the accepted candidates (selectCandidates with checkCorner and
scaleInvarient), the circle rasteriser, and SubpixelCorner's cost and gradient over Ceres' bicubic interpolation."""
import math

import numpy as np

SIGMAS = (1.4, 2.0, 1.0)


def gaussian(n, sigma):
    """cv::getGaussianKernel(n, sigma, CV_64F) for sigma > 0, rounded to float32"""
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    cf = np.exp((-0.5 / (sigma * sigma)) * x * x)
    s = 0.
    for c in cf:
        s += c
    return (cf * (1. / s)).astype(np.float32)


def reflect101(idx, n):
    idx = np.abs(idx)
    return np.where(idx >= n, 2 * n - 2 - idx, idx)


def blur(img, n, sigma):
    """the separable blur of the library: float32 taps summed in order (rows, then columns), BORDER_REFLECT_101, rounded half
    to even to u8"""
    w = gaussian(n, sigma)
    r = n // 2
    H, W = img.shape
    x = img.astype(np.float32)
    cols = reflect101(np.arange(-r, W + r), W)
    xp = x[:, cols]
    h = w[0] * xp[:, 0:W]
    for i in range(1, n):
        h = h + w[i] * xp[:, i:i + W]
    rows = reflect101(np.arange(-r, H + r), H)
    hp = h[rows, :]
    v = w[0] * hp[0:H]
    for j in range(1, n):
        v = v + w[j] * hp[j:j + H]
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def response(img, sigma):
    """computeResponse(0.7, sigma) (.cpp:262-330): dict src1, src2, gradx, grady, imgrad, resp, avg"""
    src1 = blur(img, 3, 0.7)
    src2 = blur(img, 1 + 2 * int(math.ceil(sigma)), sigma)
    H, W = img.shape
    s1, s2 = src1.astype(np.int64), src2.astype(np.int64)
    c = (slice(1, H - 1), slice(1, W - 1))
    sh = lambda a, dv, du: a[1 + dv:H - 1 + dv, 1 + du:W - 1 + du]
    d1x, d2x = sh(s1, 0, 1) - sh(s1, 0, -1), sh(s2, 0, 1) - sh(s2, 0, -1)
    d1y, d2y = sh(s1, 1, 0) - sh(s1, -1, 0), sh(s2, 1, 0) - sh(s2, -1, 0)
    gxS = (d1x.astype(np.float64) - 0.3 * d2x) / 2.
    gyS = (d1y.astype(np.float64) - 0.3 * d2y) / 2.
    out = {k: np.zeros((H, W), np.float32) for k in ("gradx", "grady", "imgrad", "resp")}
    out["gradx"][c] = (gxS * 0.01).astype(np.float32)
    out["grady"][c] = (gyS * 0.01).astype(np.float32)
    out["imgrad"][c] = (np.sqrt(gxS * gxS + gyS * gyS) * 0.01).astype(np.float32)
    iuu = (sh(s2, 0, -1) + sh(s2, 0, 1) - 2 * sh(s2, 0, 0)).astype(np.float64)
    ivv = (sh(s2, -1, 0) + sh(s2, 1, 0) - 2 * sh(s2, 0, 0)).astype(np.float64)
    iuv = (sh(s2, -1, -1) + sh(s2, 1, 1) - sh(s2, 1, -1) - sh(s2, -1, 1)).astype(np.float64) / 4
    gx = np.trunc(d2x / 2.)   # integer division in the reference
    gy = np.trunc(d2y / 2.)
    gsq = gx * gx + gy * gy
    rv = -iuu * ivv + iuv * iuv - 0.001 * (gsq * gsq)
    keep = rv > 0.01
    out["resp"][c] = np.where(keep, rv, 0.).astype(np.float32)
    cnt = int(keep.sum())
    out["avg"] = float(rv[keep].sum()) / cnt if cnt else float("nan")
    out["src1"], out["src2"] = src1, src2
    return out


def local_maxima(resp, avg, R):
    """selectCandidates' scan (.cpp:497-521) -> list of (value, u, v), value descending, ties by smaller v W + u"""
    H, W = resp.shape
    res = []
    cand = np.argwhere(~(resp.astype(np.float64) < avg))
    for v, u in cand:
        if u < R or u >= W - R or v < R or v >= H - R:
            continue
        val = resp[v, u]
        ok = True
        for j in range(-R, R + 1):
            for i in range(-R, R + 1):
                if (i == 0 and j == 0) or i * i + j * j > R * R + 1:
                    continue
                nb = resp[v + j, u + i]
                if val <= nb:
                    if val == nb and (i > 0 or (i == 0 and j > 0)):
                        continue
                    ok = False
                    break
            if not ok:
                break
        if ok:
            res.append((float(val), int(u), int(v)))
    res.sort(key=lambda t: (-t[0], t[2] * W + t[1]))
    return res


def _sign(x):
    return 1 if x > 0 else -1


def circle(r):
    """getCircle around (0, 0) (.cpp:1079-1108, CurveRasterizer curve_rasterizer.h:170-259) -> list of (du, dv)"""
    if r == 1:
        return list(zip([1, 1, 0, -1, -1, -1, 0, 1], [0, 1, 1, 1, 0, -1, -1, -1]))
    k1 = -float(r * r)
    f = lambda u, v: (1. * u) * u + (1. * v) * v + k1
    st = {"u": r, "v": 0}
    st["fu"], st["fv"], st["d"] = 2. * r, 0., f(r, 0)
    eps = 1 if st["fu"] * (r - 0) - st["fv"] * (0 - r) > 0 else -1

    def move_u(du):
        if du:
            st["u"] += du
            fu2 = 2. * st["u"]
            st["d"] += 0.5 * du * (st["fu"] + fu2)
            st["fu"], st["fv"] = fu2, 2. * st["v"]

    def move_v(dv):
        if dv:
            st["v"] += dv
            fv2 = 2. * st["v"]
            st["d"] += 0.5 * dv * (st["fv"] + fv2)
            st["fv"], st["fu"] = fv2, 2. * st["u"]

    rnd = lambda x: int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)   # std::round
    res, i = [], 0
    while True:
        res.append((st["u"], st["v"]))
        if i > 5 and abs(st["u"] - r) <= 1 and abs(st["v"]) <= 1:
            break
        i += 1
        if abs(st["fu"]) > abs(st["fv"]):
            move_v(eps * _sign(st["fu"]))
            move_u(-rnd(st["d"] / st["fu"]))
        else:
            move_u(-eps * _sign(st["fv"]))
            move_v(-rnd(st["d"] / st["fv"]))
    return res


def _transitions(img, u, v, r):
    H, W = img.shape
    s = [int(img[min(max(v + dv, 0), H - 1), min(max(u + du, 0), W - 1)]) for du, dv in circle(r)]
    n = len(s)
    return [s[1] - s[n - 1]] + [s[k + 1] - s[k - 1] for k in range(1, n - 1)] + [s[0] - s[n - 2]]


def _set_zero(tv, it):
    n, ref = len(tv), tv[it]
    d = it
    while True:
        tv[d] = 0
        d = (d + 1) % n
        if not tv[d] * ref > 0:
            break
    b = it
    while True:
        tv[b] = 0
        b = n - 1 if b == 0 else b - 1
        if not tv[b] * ref > 0:
            break


def _argmax(tv):
    return max(range(len(tv)), key=lambda k: (tv[k], -k))


def _argmin(tv):
    return min(range(len(tv)), key=lambda k: (tv[k], k))


def check_corner(img, u, v, check_radius):
    """checkCorner (.cpp:331-442)"""
    for radius in range(check_radius, check_radius + max(3, check_radius)):
        tv = _transitions(img, u, v, radius)
        n = len(tv)
        d1, d2 = n // 2 - 2, n - (n // 2 - 2)
        i1 = _argmax(tv)
        m1 = tv[i1]
        _set_zero(tv, i1)
        i2 = _argmax(tv)
        if tv[i2] < m1 * 0.3:
            return False
        m2 = tv[i2]
        _set_zero(tv, i2)
        if not d1 <= abs(i1 - i2) <= d2:
            return False
        i3 = _argmax(tv)
        if tv[i3] > m2 * 0.5:
            return False
        _set_zero(tv, i3)
        j1 = _argmin(tv)
        n1 = tv[j1]
        if n1 > m1 * -0.3:
            return False
        _set_zero(tv, j1)
        j2 = _argmin(tv)
        if tv[j2] > n1 * -0.3:
            return False
        n2 = tv[j2]
        _set_zero(tv, j2)
        if not d1 <= abs(j1 - j2) <= d2:
            return False
        j3 = _argmin(tv)
        if tv[j3] < n2 * 0.5:
            return False
        _set_zero(tv, j3)
    return True


def scale_invariant(gradx, grady, u0, v0, R):
    """scaleInvarient (.cpp:444-492)"""
    H, W = gradx.shape
    for radius in range(R, 2 * R):
        acc, norm = 0., 1e-10
        for dv in range(-radius, radius + 1):
            for du in range(-radius, radius + 1):
                sq = float(du * du + dv * dv)
                if sq > radius * radius + 1 or sq < 1:
                    continue
                u, v = u0 + du, v0 + dv
                if u < 0 or u >= W or v < 0 or v >= H:
                    continue
                gx, gy = float(gradx[v, u]), float(grady[v, u])
                g2 = gx * gx + gy * gy
                if g2 < 1e-3:
                    continue
                p = gx * du + gy * dv
                acc += p * p / sq
                norm += g2
        if acc / norm < 0.3:
            return True
    return False


def candidates(img, sigma, cols, rows):
    """selectCandidates (.cpp:494-610): (accepted [(u, v)] in order, VAL_THRESH, number of maxima)"""
    m = response(img, sigma)
    R = int(math.floor(1.5 * sigma + 0.5))
    mx = local_maxima(m["resp"], m["avg"], R)
    K = cols * rows
    acc = 0.
    for val, _, _ in mx[:K]:
        acc += val
    thresh = 0.05 * acc / K
    out = []
    for val, u, v in mx:
        if not val > thresh or len(out) >= 10 * K:
            break
        if not any(check_corner(img, u, v, r) for r in range(1, R + 1)):
            continue
        if not scale_invariant(m["gradx"], m["grady"], u, v, R):
            continue
        out.append((u, v))
    return out, thresh, len(mx)


# ---- SubpixelCorner (.cpp:31-103) ----

def _hermite(p0, p1, p2, p3, x):
    a = 0.5 * (-p0 + 3.0 * p1 - 3.0 * p2 + p3)
    b = 0.5 * (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3)
    c = 0.5 * (-p0 + p2)
    return p1 + x * (c + x * (b + x * a)), c + x * (2.0 * b + 3.0 * a * x)


def bicubic(grid, r, c):
    """ceres::BiCubicInterpolator::Evaluate(r, c) over Grid2D's clamped border -> (f, dfdr, dfdc)"""
    H, W = grid.shape
    row, col = int(math.floor(r)), int(math.floor(c))
    fr, dc = [], []
    for k in range(4):
        rr = min(max(row - 1 + k, 0), H - 1)
        p = [float(grid[rr, min(max(col - 1 + q, 0), W - 1)]) for q in range(4)]
        f, d = _hermite(*p, c - col)
        fr.append(f)
        dc.append(d)
    f, dfdr = _hermite(*fr, r - row)
    dfdc, _ = _hermite(*dc, r - row)
    return f, dfdr, dfdc


def subpixel_cost(gradu, gradv, prior, length, x, steps=7):
    """SubpixelCorner::Evaluate: (cost, gradient[5]) at parameters x = (u, v, theta1, theta2, h)"""
    u, v = x[0], x[1]
    step = length / steps
    stepVec = []
    for i in range(1, steps + 1):
        stepVec += [-i * step, i * step]
    cost = 0.1 * ((prior[0] - u) ** 2 + (prior[1] - v) ** 2)
    g = np.array([0.2 * (u - prior[0]), 0.2 * (v - prior[1]), 0., 0., 0.])
    h = x[4]
    for direction in range(2):
        th = 2 + direction
        s, c = math.sin(x[th]), math.cos(x[th])
        flow = 1 if direction else -1
        for L in stepVec:
            eta = (1 if L > 0 else -1) * flow
            ui = u + c * L - s * h * eta
            vi = v + s * L + c * h * eta
            fu, fuv, fuu = bicubic(gradu, vi, ui)
            fv, fvv, fvu = bicubic(gradv, vi, ui)
            cost += eta * (fv * c - fu * s)
            dudth = -s * L - c * h * eta
            dvdth = c * L - s * h * eta
            g[0] += eta * (fvu * c - fuu * s)
            g[1] += eta * (fvv * c - fuv * s)
            g[th] += eta * ((fvv * dvdth + fvu * dudth) * c - (fuv * dvdth + fuu * dudth) * s - fu * c - fv * s)
            g[4] += fvv * c * c + fuu * s * s - s * c * (fvu + fuv)
    return cost, g
