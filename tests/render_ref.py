"""Restatement of the reference's RenderDevice in numpy / Python, written from its sources: RenderDevice::fillBuffers and fillImage
(src/render/render.cpp:86-193), Plane::intersection (plane.cpp:39-60), Background::intersection (background.cpp:34-56),
Texture::sample (texture.cpp:28-70), bilinear (include/ocv.h:64-84), ceres' BiCubicInterpolator over the clamping Grid2D
(include/ceres.h) and LookupFilter (aa_filter_lt.cpp).

The operation order it fixes (every + and * below is one IEEE double operation, nothing fused):
  * a 3-vector dot product is (a0 b0 + a1 b1) + a2 b2, R x is three such rows, |x| is sqrt of the dot product;
  * the plane's point is (dir lambda + pos) - t per component, uv = u0 + fu (ex . pt);
  * the four buffers are narrow: index int16 (-1), u / v / depth float32 (depth starts at 1e6); an object wins when
    double(stored float depth) > its depth, and later stages read the float32-rounded u and v;
  * a footprint column is (max - min) / count with count the 1 or 2 neighbours holding the same index, zero for none;
  * nu = min(max(round(|eu| 2.75), 1), 24) with round half away from zero; the first tap is (pt + eu origin(nu)) + ev origin(nv),
    a row starts at pt0 + double(vidx) vstep and walks by ptCur += ustep; a row is summed left to right from 0, the rows top to
    bottom from 0; the grey value is the truncation of min(255, max(res, 0));
  * bilinear truncates towards zero, clamps u before v and lets a failed u send v to row 0, and evaluates
    (i11 dx + i10 dx2) dy + (i01 dx + i00 dx2) (1 - dy).
numpy's cumulative sums are used where a sum's order matters: np.add.accumulate adds strictly in index order (np.sum does not)."""
import math

import numpy as np

from tests import stereo_ref as sr

SIGMA = 0.55
MAX_KERNEL = 24
SAMPLE_COUNT = 600
BACKGROUND_DEPTH = 150.
PLANE_GATE = 0.01
DEPTH_INIT = np.float32(1e6)
MAX_PLANES = 64
COUNTS = ("not_reconstructed", "uncovered", "background", "plane", "single_tap")


def filter_origin(length):
    return 3 * SIGMA * (-1 + 1. / length)


def filter_step(length):
    return 6 * SIGMA / length


RADIUS = 5 * SIGMA


def _filter_table():
    """LookupFilter::LookupFilter, its loops as written: kernels[length] for length 0 .. 24"""
    kernel_data, integral = [0.] * (SAMPLE_COUNT + 1), [0.] * (SAMPLE_COUNT + 1)
    step = filter_step(SAMPLE_COUNT)
    x = filter_origin(SAMPLE_COUNT)
    for i in range(SAMPLE_COUNT):
        kernel_data[i] = math.exp(-x * x / (2 * SIGMA * SIGMA)) - 0.35 * math.exp(-x * x / (1.3 * SIGMA * SIGMA))
        integral[i + 1] = integral[i] + kernel_data[i]
        x += step
    kernel_data[SAMPLE_COUNT] = 0.
    normalizer = 1. / integral[SAMPLE_COUNT]
    integral[SAMPLE_COUNT] = 1.
    for i in range(SAMPLE_COUNT):
        integral[i] *= normalizer
        kernel_data[i] *= normalizer
    kernels = [[], [1.], [0.5, 0.5]]
    for length in range(3, MAX_KERNEL + 1):
        frac_samples = float(SAMPLE_COUNT) / length
        prev, k = 0., []
        for i in range(length):
            frac_idx = frac_samples * (i + 1)
            idx = int(frac_idx)
            cur = integral[idx] + (frac_idx - idx) * kernel_data[idx]
            k.append(cur - prev)
            prev = cur
        kernels.append(k)
    return [np.array(k, dtype=np.float64) for k in kernels]


KERNELS = _filter_table()


def background(texture):
    """Background(ptree): the object record of a panorama"""
    tex = np.ascontiguousarray(texture, dtype=np.uint8)
    rows, cols = tex.shape
    return dict(kind="background", texture=tex, u0=cols / 2., v0=rows / 2., fu=cols / (2 * math.pi), fv=rows / (2 * math.pi),
                t=(0., 0., 0.), ex=(1., 0., 0.), ey=(0., 1., 0.), ez=(0., 0., 1.))


def plane(texture, pose, width, height):
    """Plane(ptree)"""
    tex = np.ascontiguousarray(texture, dtype=np.uint8)
    rows, cols = tex.shape
    R = sr.rotation_matrix([float(v) for v in pose[3:]], 1.)
    return dict(kind="plane", texture=tex, u0=cols / 2., v0=rows / 2., fu=cols / float(width), fv=rows / float(height),
                t=tuple(float(v) for v in pose[:3]), ex=(R[0], R[3], R[6]), ey=(R[1], R[4], R[7]), ez=(R[2], R[5], R[8]))


def world(background_texture, planes):
    """planes: [(texture, pose, width, height), ...]"""
    return [background(background_texture)] + [plane(*p) for p in planes]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def reconstruct(cam, u, v):
    """EnhancedCamera::reconstructPoint (eucm.h:85-104) on arrays: (X0, X1, X2, ok)"""
    alpha, beta, fu, fv, u0, v0 = [float(c) for c in cam]
    xn = (u - u0) / fu
    yn = (v - v0) / fv
    u2 = xn * xn + yn * yn
    gamma = 1. - alpha
    num = 1. - u2 * alpha * alpha * beta
    det = 1 - (alpha - gamma) * beta * u2
    ok = ~(det < 0)
    denom = gamma + alpha * np.sqrt(np.where(ok, det, 0.))
    return xn, yn, num / denom, ok


def _inside(o, uu, vv):
    rows, cols = o["texture"].shape
    return (uu >= 0) & (uu <= cols - 1) & (vv >= 0) & (vv <= rows - 1)


def _hit(o, pos, d):
    """intersection() of one object on arrays of rays: (hit, u, v, depth)"""
    if o["kind"] == "background":
        sphi, cphi = _dot(o["ex"], d), _dot(o["ez"], d)
        cth = np.sqrt(sphi * sphi + cphi * cphi)
        sth = _dot(o["ey"], d)
        phi = np.array([math.atan2(a, b) for a, b in zip(sphi.ravel(), cphi.ravel())]).reshape(sphi.shape)
        th = np.array([math.atan2(a, b) for a, b in zip(sth.ravel(), cth.ravel())]).reshape(sphi.shape)
        uu = o["u0"] + o["fu"] * phi
        vv = o["v0"] + o["fv"] * th
        return _inside(o, uu, vv), uu, vv, np.full(sphi.shape, BACKGROUND_DEPTH)
    t = o["t"]
    num = _dot(o["ez"], (t[0] - pos[0], t[1] - pos[1], t[2] - pos[2]))
    den = _dot(o["ez"], d)
    with np.errstate(all="ignore"):
        gate = ~(den * num < PLANE_GATE)
        lam = num / den
        depth = lam * np.sqrt(_dot(d, d))
        pt = [d[i] * lam + pos[i] - t[i] for i in range(3)]
        uu = o["u0"] + o["fu"] * _dot(o["ex"], pt)
        vv = o["v0"] + o["fv"] * _dot(o["ey"], pt)
        return gate & _inside(o, uu, vv), uu, vv, depth


def fill_buffers(cam, width, height, objects, xi_cam):
    """fillBuffers: dict(index int16, u, v, depth float32 [height, width], ok: the pixel reconstructs, close: the two nearest hits
    are less than one float32 step apart, so which of them the float32 depth test keeps hangs on the last bit of a depth)"""
    xi = [float(v) for v in xi_cam]
    R = sr.rotation_matrix(xi[3:], 1.)
    pos = xi[:3]
    vv, uu = np.mgrid[0:height, 0:width]
    x0, x1, x2, ok = reconstruct(cam, uu.astype(np.float64), vv.astype(np.float64))
    d = [R[3 * i] * x0 + R[3 * i + 1] * x1 + R[3 * i + 2] * x2 for i in range(3)]
    index = np.full((height, width), -1, np.int16)
    ub, vb = np.zeros((height, width), np.float32), np.zeros((height, width), np.float32)
    depth = np.full((height, width), DEPTH_INIT, np.float32)
    hits = []
    for k, o in enumerate(objects):
        hit, ou, ov, od = _hit(o, pos, d)
        with np.errstate(all="ignore"):
            take = ok & hit & (depth.astype(np.float64) > od)
        depth[take] = od[take].astype(np.float32)
        index[take] = k
        ub[take] = ou[take].astype(np.float32)
        vb[take] = ov[take].astype(np.float32)
        hits.append(np.where(ok & hit & np.isfinite(od), od, np.inf))
    two = np.sort(np.stack(hits + [np.full((height, width), np.inf)]), axis=0)[:2]
    with np.errstate(all="ignore"):
        close = np.isfinite(two[1]) & (two[1] - two[0] < np.spacing(two[0].astype(np.float32)).astype(np.float64))
    return dict(index=index, u=ub, v=vb, depth=depth, ok=ok, close=close)


def bilinear(tex, x, y):
    """bilinear<double>(Mat8u, x, y) on arrays of coordinates"""
    rows, cols = tex.shape
    u, v = np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64)
    dx, dy = x - u, y - v
    dx2 = 1 - dx
    fail_u = (u < 0) | (u > cols - 2)
    uc = np.where(u < 0, 0, np.where(u > cols - 2, cols - 1, u))
    to_zero = fail_u | (v < 0)            # `fail` is already set when v is tested: v = 0
    vc = np.where(to_zero, 0, np.where(v > rows - 2, rows - 1, v))
    fail = to_zero | (v > rows - 2)
    ui, vi = np.clip(u, 0, max(cols - 2, 0)), np.clip(v, 0, max(rows - 2, 0))
    t = tex.astype(np.float64)
    i00, i01, i10, i11 = t[vi, ui], t[vi, np.minimum(ui + 1, cols - 1)], t[np.minimum(vi + 1, rows - 1), ui], \
        t[np.minimum(vi + 1, rows - 1), np.minimum(ui + 1, cols - 1)]
    val = (i11 * dx + i10 * dx2) * dy + (i01 * dx + i00 * dx2) * (1 - dy)
    return np.where(fail, t[vc, uc], val)


def _cubic(p0, p1, p2, p3, x):
    """ceres::CubicHermiteSpline<1>, the value"""
    a = 0.5 * (-p0 + 3.0 * p1 - 3.0 * p2 + p3)
    b = 0.5 * (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3)
    c = 0.5 * (-p0 + p2)
    return p1 + x * (c + x * (b + x * a))


def bicubic(tex, r, c):
    """BiCubicInterpolator<Grid2D<uchar>>::Evaluate(r, c, &f, NULL, NULL)"""
    rows, cols = tex.shape
    row, col = int(math.floor(r)), int(math.floor(c))
    cc = [min(max(col - 1 + j, 0), cols - 1) for j in range(4)]
    f = []
    for k in range(4):
        p = tex[min(max(row - 1 + k, 0), rows - 1)]
        f.append(_cubic(float(p[cc[0]]), float(p[cc[1]]), float(p[cc[2]]), float(p[cc[3]]), c - col))
    return _cubic(f[0], f[1], f[2], f[3], r - row)


def _round(x):
    """std::round of a non-negative double: halves away from zero"""
    r = math.floor(x)
    return r + 1. if x - r >= 0.5 else r


def kernel_length(e0, e1):
    return int(min(max(_round(math.sqrt(e0 * e0 + e1 * e1) * RADIUS), 1.), 24.))


def sample(tex, pt, eu, ev):
    """Texture::sample: (grey value, nu, nv, taps that left the texture on the [left, right, top, bottom])"""
    rows, cols = tex.shape
    nu, nv = kernel_length(eu[0], eu[1]), kernel_length(ev[0], ev[1])
    if nu == 1 and nv == 1:
        res = bicubic(tex, pt[1], pt[0])
        left = [0, 0, 0, 0]
    else:
        su, sv, ou, ov = filter_step(nu), filter_step(nv), filter_origin(nu), filter_origin(nv)
        ustep, vstep = (eu[0] * su, eu[1] * su), (ev[0] * sv, ev[1] * sv)
        pt0 = (pt[0] + eu[0] * ou + ev[0] * ov, pt[1] + eu[1] * ou + ev[1] * ov)
        vidx = np.arange(nv, dtype=np.float64)
        xs, ys = np.empty((nv, nu)), np.empty((nv, nu))
        xs[:, 0], ys[:, 0] = pt0[0] + vidx * vstep[0], pt0[1] + vidx * vstep[1]
        xs[:, 1:], ys[:, 1:] = ustep[0], ustep[1]
        xs, ys = np.add.accumulate(xs, axis=1), np.add.accumulate(ys, axis=1)   # ptCur += ustep, in order
        terms = bilinear(tex, xs, ys) * KERNELS[nu][None, :]
        ures = np.add.accumulate(terms, axis=1)[:, -1]                          # 0 + t0 is t0: the sum from the left
        res = float(np.add.accumulate(ures * KERNELS[nv])[-1])
        left = [int((xs < 0).sum()), int((xs > cols - 1).sum()), int((ys < 0).sum()), int((ys > rows - 1).sum())]
    grey = min(255., max(res, 0.))
    return int(grey), nu, nv, left


def fill_image(width, height, objects, buf):
    """fillImage on the buffers of fill_buffers (only index, u and v are read): dict(image uint8 with 0 where nothing is hit,
    nu, nv int [height, width] (0 where nothing is hit), ucount, vcount: neighbours holding the same index along the row / the
    column (-1 where nothing is hit), left: taps that left the textures on the four sides)"""
    index, ub, vb = buf["index"], buf["u"].astype(np.float64), buf["v"].astype(np.float64)
    image = np.zeros((height, width), np.uint8)
    nus, nvs = np.zeros((height, width), np.int32), np.zeros((height, width), np.int32)
    ucs, vcs = np.full((height, width), -1, np.int32), np.full((height, width), -1, np.int32)
    left = np.zeros(4, np.int64)
    for v in range(height):
        for u in range(width):
            idx = index[v, u]
            if idx == -1:
                continue
            pt = (float(ub[v, u]), float(vb[v, u]))
            eu, ev = [0., 0.], [0., 0.]
            count, u_min, u_max, v_min, v_max = 0, pt[0], pt[0], pt[1], pt[1]
            if u > 0 and index[v, u - 1] == idx:
                count, u_min, v_min = count + 1, float(ub[v, u - 1]), float(vb[v, u - 1])
            if u < width - 1 and index[v, u + 1] == idx:
                count, u_max, v_max = count + 1, float(ub[v, u + 1]), float(vb[v, u + 1])
            if count:
                eu = [(u_max - u_min) / count, (v_max - v_min) / count]
            ucs[v, u] = count
            count, u_min, u_max, v_min, v_max = 0, pt[0], pt[0], pt[1], pt[1]
            if v > 0 and index[v - 1, u] == idx:
                count, u_min, v_min = count + 1, float(ub[v - 1, u]), float(vb[v - 1, u])
            if v < height - 1 and index[v + 1, u] == idx:
                count, u_max, v_max = count + 1, float(ub[v + 1, u]), float(vb[v + 1, u])
            if count:
                ev = [(u_max - u_min) / count, (v_max - v_min) / count]
            vcs[v, u] = count
            image[v, u], nus[v, u], nvs[v, u], out = sample(objects[idx]["texture"], pt, eu, ev)
            left += out
    return dict(image=image, nu=nus, nv=nvs, ucount=ucs, vcount=vcs, left=left)


def counts_of(objects, buf, img):
    """the five counters of a view, in the order of COUNTS"""
    kinds = np.array([o["kind"] == "background" for o in objects])
    covered = buf["index"] >= 0
    bg = covered & kinds[np.maximum(buf["index"], 0)]
    return np.array([(~buf["ok"]).sum(), (buf["ok"] & ~covered).sum(), bg.sum(), (covered & ~bg).sum(),
                     (covered & (img["nu"] == 1) & (img["nv"] == 1)).sum()], dtype=np.int64)


def render(cam, width, height, objects, xi_cam):
    """RenderDevice::render of one view: the buffers, the image record and counts, in one dict"""
    buf = fill_buffers(cam, width, height, objects, xi_cam)
    img = fill_image(width, height, objects, buf)
    out = dict(buf)
    out.update(img)
    out["counts"] = counts_of(objects, buf, img)
    return out
