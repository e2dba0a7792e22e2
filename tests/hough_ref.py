"""numpy restatement of the reference's hough_test (test/reconstruction/hough_test.cpp) with the deviations of DESIGN.md
section 9 "Line detection", for the line detection tests.  FP64 in the reference's expression order (numpy ufuncs and Python
floats are IEEE doubles and nothing is fused), C round (half away from zero) written out, the blur in float32 under the
project's float rule: the accumulator, the blur, the maxima and the lines agree with the library bit for bit.  The vote is
vectorised over the image, everything per line is scalar.  The rasteriser and the scalar camera are those of stereo_ref."""
import math

import numpy as np

from tests.stereo_ref import Poly2, Raster, cround, fdiv, reconstruct

COUNTS = ("selected", "not_reconstructed", "first_votes", "antipode_votes", "failed_projections", "outside")
NOT_VALID, BOTH_VALID = -1., -2.
MAX_TRACE = 1500


def params(**kw):
    """hough_test.cpp:93-97, 416, 445"""
    p = dict(margin=5, grad_thresh=0.001, search_size=2, acc_thresh=7., acc_delta_thresh=0.05, horizon_ratio=3e-3, blur_size=5,
             blur_sigma=0.9)
    assert set(kw) <= set(p)
    p.update(kw)
    return p


def acc_size(acc_cam):
    """(acc_w, acc_h): Mat32f acc(2 v0, 2 u0) (.cpp:369)"""
    return int(2 * acc_cam[4]), int(2 * acc_cam[5])


def round_away(x):
    """C round() of an array: half away from zero"""
    r = np.trunc(x)
    return r + np.where(np.abs(x - r) >= 0.5, np.sign(x), 0.)


def sobel(img):
    """integer 3 x 3 Sobel sums (kx, ky) of a u8 image; the border stays zero (it is never visited: margin >= 1)"""
    a = img.astype(np.int64)
    kx, ky = np.zeros_like(a), np.zeros_like(a)
    kx[1:-1, 1:-1] = (a[:-2, 2:] - a[:-2, :-2]) + 2 * (a[1:-1, 2:] - a[1:-1, :-2]) + (a[2:, 2:] - a[2:, :-2])
    ky[1:-1, 1:-1] = (a[2:, :-2] - a[:-2, :-2]) + 2 * (a[2:, 1:-1] - a[:-2, 1:-1]) + (a[2:, 2:] - a[:-2, 2:])
    return kx, ky


def reconstruct_v(p, u, v):
    """EnhancedCamera::reconstructPoint on arrays: (ok, x, y, z)"""
    alpha, beta, fu, fv, u0, v0 = p
    xn = (u - u0) / fu
    yn = (v - v0) / fv
    u2 = xn * xn + yn * yn
    gamma = 1. - alpha
    num = 1. - u2 * alpha * alpha * beta
    det = 1 - (alpha - gamma) * beta * u2
    ok = ~(det < 0)
    denom = gamma + alpha * np.sqrt(np.where(ok, det, 0.))
    return ok, xn, yn, num / denom


def project_v(p, x, y, z):
    """EnhancedProjector on arrays: (ok, u, v)"""
    alpha, beta, fu, fv, u0, v0 = p
    denom = alpha * np.sqrt(z * z + beta * (x * x + y * y)) + (1. - alpha) * z
    ok = ~(denom < 1e-3)
    if alpha > 0.5:
        zn = z / denom
        C = (alpha - 1.) / (alpha + alpha - 1.)
        ok &= ~(zn < C)
    return ok, fu * (x / denom) + u0, fv * (y / denom) + v0


def _cast(acc, acc_cam, A, B, C):
    """the votes of the normals (A, B, C): (cast, failed, outside) counts"""
    h, w = acc.shape
    ok, qu, qv = project_v(acc_cam, A, B, C)
    cu, cv = round_away(qu), round_away(qv)
    inside = ok & (cu >= 0.) & (cu < w) & (cv >= 0.) & (cv < h)   # NaN is outside
    np.add.at(acc, (cv[inside].astype(np.int64), cu[inside].astype(np.int64)), 1)
    return int(inside.sum()), int((~ok).sum()), int((ok & ~inside).sum())


def vote(img, cam, acc_cam, prm, stats=None):
    """(accumulator int32 [acc_h, acc_w], counts int64 [6]) of one image (.cpp:363-420).  A dict given as `stats` is filled with
    the (cast, failed, outside) counts of the first and of the antipode votes and the number of antipode votes tried."""
    w, h = acc_size(acc_cam)
    acc = np.zeros((h, w), dtype=np.int32)
    kx, ky = sobel(img)
    m = prm["margin"]
    gnorm = (kx * kx + ky * ky).astype(np.float64) / 4194304.   # exact: gx^2 + gy^2 of the float gradient k / 2048
    sel = np.zeros(img.shape, dtype=bool)
    sel[m:img.shape[0] - m, m:img.shape[1] - m] = True
    sel &= ~(gnorm < prm["grad_thresh"])
    v, u = np.nonzero(sel)   # raster order
    counts = np.zeros(6, dtype=np.int64)
    counts[0] = u.size
    with np.errstate(all="ignore"):
        ok, x, y, z = reconstruct_v(cam, u.astype(np.float64), v.astype(np.float64))
        counts[1] = int((~ok).sum())
        x, y, z = x[ok], y[ok], z[ok]
        fx, fy = kx[v, u][ok] / 2048., ky[v, u][ok] / 2048.
        alpha, beta = cam[0], cam[1]
        gamma = 1. - alpha
        Kx = 2 * alpha * alpha * beta * x
        Ky = 2 * alpha * alpha * beta * y
        P = 2 * (alpha - gamma)
        Q = 2 * gamma
        Y0, Y1, Y2 = -fy * (P * z + Q), fx * (P * z + Q), fy * Kx - fx * Ky
        A, B, C = y * Y2 - z * Y1, z * Y0 - x * Y2, x * Y1 - y * Y0
        neg = C < 0
        A, B, C = np.where(neg, A * -1, A), np.where(neg, B * -1, B), np.where(neg, C * -1, C)
        c1, f1, o1 = _cast(acc, acc_cam, A, B, C)
        anti = C * C / (A * A + B * B) < prm["horizon_ratio"]   # 0 / 0 is NaN: no antipode vote
        c2, f2, o2 = _cast(acc, acc_cam, -A[anti], -B[anti], -C[anti])
    counts[2:] = (c1, c2, f1 + f2, o1 + o2)
    if stats is not None:
        stats.update(first=(c1, f1, o1), antipode=(c2, f2, o2), antipode_tried=int(anti.sum()))
    return acc, counts


def gaussian(n, sigma):
    """cv::getGaussianKernel(n, sigma, CV_64F), normalised, rounded to float"""
    cf, s = [], 0.
    scale2x = -0.5 / (sigma * sigma)
    for i in range(n):
        x = i - (n - 1) * 0.5
        cf.append(math.exp(scale2x * x * x))
        s += cf[-1]
    s = 1. / s
    return np.array([c * s for c in cf]).astype(np.float32)


def _reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def blur(acc, prm):
    """the float blur of the int32 accumulator: row pass, then column pass; taps summed in order; BORDER_REFLECT_101"""
    w = gaussian(prm["blur_size"], prm["blur_sigma"])
    r = prm["blur_size"] // 2
    a = acc.astype(np.float32)
    for axis in (1, 0):
        idx = np.arange(a.shape[axis])
        out = None
        for i in range(prm["blur_size"]):
            tap = w[i] * np.take(a, _reflect101(idx - r + i, a.shape[axis]), axis=axis)
            out = tap if out is None else out + tap
        a = out
        assert a.dtype == np.float32
    return a


def maxima(b, acc_cam, prm, stats=None):
    """the kept bins of the blurred accumulator in raster order (.cpp:458-482): [(centroid u, v, value, ABC)].  A dict given
    as `stats` is filled with why candidates were dropped: "window" bins passed the (2 s + 1)^2 test, of which
    "not_reconstructed" failed the accumulator camera's reconstruction and "behind" gave n[2] < 0; "bins" lists the raster
    positions v * acc_w + u of the kept ones."""
    s = prm["search_size"]
    if stats is not None:
        stats.update(window=0, not_reconstructed=0, behind=0, bins=[])
    h, w = b.shape
    out = []
    vs, us = np.nonzero(~(b.astype(np.float64) < prm["acc_thresh"]))
    for v, u in zip(vs.tolist(), us.tolist()):
        if u < s or u >= w - s or v < s or v >= h - s:
            continue
        val = float(b[v, u])
        win = b[v - s:v + s + 1, u - s:u + s + 1].astype(np.float64) + prm["acc_delta_thresh"]
        win[s, s] = -math.inf
        if (val <= win).any():
            continue
        uacc = vacc = nacc = 0.
        for du in (-1, 0, 1):
            for dv in (-1, 0, 1):
                x = float(b[v + dv, u + du])
                nacc += x
                uacc += du * x
                vacc += dv * x
        cu, cv = u + fdiv(uacc, nacc), v + fdiv(vacc, nacc)
        ABC = reconstruct(acc_cam, cu, cv)
        if stats is not None:
            stats["window"] += 1
            stats["not_reconstructed"] += ABC is None
            stats["behind"] += ABC is not None and ABC[2] < 0
        if ABC is None or ABC[2] < 0:   # deviation: the reference goes on with an unset vector when the reconstruction fails
            continue
        if stats is not None:
            stats["bins"].append(v * w + u)
        out.append((cu, cv, val, ABC))
    return out


def polynomial(p, plane):
    """computePolynomial (.cpp:31-91)"""
    alpha, beta, fu, fv, u0, v0 = [float(x) for x in p]
    A, B, C = [float(x) for x in plane]
    gamma = 1 - alpha
    ag = alpha - gamma
    a2b = alpha * alpha * beta
    fufv, fufu, fvfv = fu * fv, fu * fu, fv * fv
    AA, BB, CC = A * A, B * B, C * C
    CCfufv = CC * fufv
    dd = fdiv(CCfufv, AA + BB)
    if (AA + BB) > 0 and dd < 1.:
        normABinv = 1. / math.sqrt(AA + BB)
        Cnorm = C / math.sqrt(AA + BB + CC)
        du = -A * Cnorm * normABinv * fu
        dv = -B * Cnorm * normABinv * fv
        return [0., 0., 0., A / fu, B / fv, -(u0 + du) * A / fu - (v0 + dv) * B / fv]
    kuu = fdiv(AA * ag + CC * a2b, CC * fufu)
    kuv = fdiv(2 * A * B * ag, CCfufv)
    kvv = fdiv(BB * ag + CC * a2b, CC * fvfv)
    ku = fdiv(2 * (-(AA * fv * u0 + A * B * fu * v0) * ag - A * C * fufv * gamma - CC * a2b * fv * u0), CCfufv * fu)
    kv = fdiv(2 * (-(BB * fu * v0 + A * B * fv * u0) * ag - B * C * fufv * gamma - CC * a2b * fu * v0), CCfufv * fv)
    k1 = fdiv(A * A * fv * fv * u0 * u0 * (alpha - gamma) + 2 * A * B * fu * fv * u0 * v0 * (alpha - gamma)
              + 2 * A * C * fu * fv * fv * gamma * u0 + B * B * fu * fu * v0 * v0 * (alpha - gamma) + 2 * B * C * fu * fu * fv * gamma * v0
              + C * C * alpha * alpha * beta * fu * fu * v0 * v0 + C * C * alpha * alpha * beta * fv * fv * u0 * u0 - C * C * fu * fu * fv * fv,
              C * C * fu * fu * fv * fv)
    return [kuu, kuv, kvv, ku, kv, k1]


def _round_d(x):
    """C round() of a double, as a double (NaN and infinities pass through)"""
    return float(cround(x)) if math.isfinite(x) else x


def _solve_quadratic(A, B, C):
    if abs(A) < 1e-8:
        return fdiv(-C, B), -1.7976931348623157e308
    delta = B * B - 4 * A * C
    if delta < 0:
        return None
    ainv = 0.5 / A
    sq = math.sqrt(delta)
    return (-B + sq) * ainv, (-B - sq) * ainv


def _choose_valid(val_max, x1, x2):
    x1, x2 = _round_d(x1), _round_d(x2)
    ok1, ok2 = 0 <= x1 < val_max, 0 <= x2 < val_max
    if ok1 and ok2:
        return BOTH_VALID
    return x1 if ok1 else (x2 if ok2 else NOT_VALID)


def _distance_check(cam, pu, pv):
    r2 = cam[2] * cam[3] / (cam[0] * cam[0] * cam[1])
    pu -= cam[4]
    pv -= cam[5]
    return pu * pu + pv * pv < r2


def _border_point(cam, poly, fixed_v, c, other_max):
    """one border of findPoint (.cpp:212-242); a candidate exists only for a valid root or BOTH_VALID (deviation 6)"""
    kuu, kuv, kvv, ku, kv, k1 = poly
    k2, k2c, kl, klc = (kuu, kvv, ku, kv) if fixed_v else (kvv, kuu, kv, ku)
    roots = _solve_quadratic(k2, kuv * c + kl, k2c * c * c + klc * c + k1)
    if roots is None:
        return None
    res = _choose_valid(other_max, *roots)
    if res >= 0:
        x = res
    elif res == BOTH_VALID:
        x0 = cam[4] if fixed_v else cam[5]
        x = roots[0] if abs(roots[0] - x0) < abs(roots[1] - x0) else roots[1]
    else:
        return None
    cand = (x, c) if fixed_v else (c, x)
    return cand if _distance_check(cam, *cand) else None


def _bring_to_border(cam, width, height, poly, pt):
    pu, pv = _round_d(pt[0]), _round_d(pt[1])
    if 0 <= pu < width and 0 <= pv < height:
        return (pu, pv)
    cu = 0. if pu < width // 2 else float(width - 1)
    cv = 0. if pv < height // 2 else float(height - 1)
    return _border_point(cam, poly, False, cu, height) or _border_point(cam, poly, True, cv, width)


def end_points(width, height, cam, n, poly):
    """findTerminalPoints (.cpp:100-122, 275-283): [pt1u, pt1v, pt2u, pt2v] or None (status 1)"""
    cam = [float(x) for x in cam]
    r = 1. / (cam[0] * math.sqrt(cam[1]))
    if abs(n[0]) + abs(n[1]) < 1e-4:
        p1, p2 = (r, 0.), (0., r)
    else:
        nrm = math.sqrt(n[0] * n[0] + n[1] * n[1])
        pn = (n[0] / nrm * r, n[1] / nrm * r)
        p1 = (pn[1] * cam[2] + cam[4], -pn[0] * cam[3] + cam[5])
        p2 = (-pn[1] * cam[2] + cam[4], pn[0] * cam[3] + cam[5])
    p1 = _bring_to_border(cam, width, height, poly, p1)
    if p1 is None:
        return None
    p2 = _bring_to_border(cam, width, height, poly, p2)
    if p2 is None:
        return None
    return [p1[0], p1[1], p2[0], p2[1]]


def trace(poly, pt4, max_steps=MAX_TRACE):
    """the pixels of .cpp:499-536: int32 [n, 2]"""
    r = Raster(cround(pt4[0]), cround(pt4[1]), cround(pt4[2]), cround(pt4[3]), Poly2(*poly))
    out = []
    while len(out) < max_steps and abs(r.u - pt4[2]) + abs(r.v - pt4[3]) > 2:
        out.append((r.u, r.v))
        r.step()
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def detect(img, cam, acc_cam, prm, stats=None):
    """one image through every stage: dict(acc, counts, blur, lines float64 [k, 16], status int32 [k]); stats: see maxima"""
    height, width = img.shape
    acc, counts = vote(img, cam, acc_cam, prm, stats)
    b = blur(acc, prm)
    lines, status = [], []
    for cu, cv, val, ABC in maxima(b, acc_cam, prm, stats):
        nrm = math.sqrt(ABC[0] * ABC[0] + ABC[1] * ABC[1] + ABC[2] * ABC[2])
        poly = polynomial(cam, ABC)
        pts = end_points(width, height, cam, ABC, poly)
        status.append(0 if pts is not None else 1)
        lines.append([cu, cv, val] + [x / nrm for x in ABC] + poly + (pts if pts is not None else [math.nan] * 4))
    return dict(acc=acc, counts=counts, blur=b, lines=np.array(lines, dtype=np.float64).reshape(-1, 16),
                status=np.array(status, dtype=np.int32))
