"""Plain-Python / numpy restatement of the reference's EnhancedSgm (src/reconstruction/eucm_sgm.cpp) with the deviations of
DESIGN.md section 9, for the stereo tests.  Scalar FP64 in the library's evaluation order (Python floats are IEEE doubles
and nothing is fused), so the geometry, curve walks, costs and disparities agree with the GPU bit for bit; the aggregation is
vectorised over scanlines.  Not pinned to reference outputs (the image has no OpenCV / Eigen to build the reference with)."""
import math

import numpy as np

INVERTED, TOO_CLOSE = 1, 2
DISPARITY_MARGIN = 20
MOVE_LIMIT = 1 << 20
INF = 1 << 28


def cround(x):
    """C round(): half away from zero"""
    r = math.trunc(x)
    if abs(x - r) >= 0.5:
        r += 1 if x > 0 else -1
    return int(r)


def fdiv(a, b):
    """IEEE a / b"""
    if b != 0:
        return a / b
    if a != a or a == 0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1., b)


def rnd_move(x):
    """-round(x) as a move: NaN -> 0, clamped to +-2^20"""
    if x != x:
        return 0
    if math.isinf(x):
        r = MOVE_LIMIT if x > 0 else -MOVE_LIMIT
    else:
        r = max(-MOVE_LIMIT, min(MOVE_LIMIT, cround(x)))
    return -r


def sign(x):
    return 2 * int(x > 0) - 1


class Poly2:
    """Polynomial2: kuu u^2 + kuv u v + kvv v^2 + ku u + kv v + k1"""

    def __init__(self, kuu, kuv, kvv, ku, kv, k1):
        self.k = (float(kuu), float(kuv), float(kvv), float(ku), float(kv), float(k1))

    @staticmethod
    def circle(u0, v0, r):
        return Poly2(1, 0, 1, -2 * u0, -2 * v0, u0 * u0 + v0 * v0 - r * r)

    def val(self, u, v):
        kuu, kuv, kvv, ku, kv, k1 = self.k
        return (kuu * u + kuv * v + ku) * u + (kvv * v + kv) * v + k1

    def gu(self, u, v):
        kuu, kuv, kvv, ku, kv, k1 = self.k
        return 2 * kuu * u + kuv * v + ku

    def gv(self, u, v):
        kuu, kuv, kvv, ku, kv, k1 = self.k
        return kuv * u + 2 * kvv * v + kv


class Raster:
    """CurveRasterizer<int, Polynomial2> (curve_rasterizer.h, second definition)"""

    def __init__(self, u, v, eu, ev, surf):
        self.u, self.v, self.surf = int(u), int(v), surf
        self.fu = surf.gu(self.u, self.v)
        self.fv = surf.gv(self.u, self.v)
        self.delta = surf.val(self.u, self.v)
        self.eps = 1 if self.fu * float(ev - self.v) - self.fv * float(eu - self.u) > 0 else -1

    def copy(self):
        r = Raster.__new__(Raster)
        r.__dict__.update(self.__dict__)
        return r

    def move_u(self, du):
        if du == 0:
            return
        self.u += du
        fu2 = self.surf.gu(self.u, self.v)
        self.delta += 0.5 * du * (self.fu + fu2)
        self.fu = fu2
        self.fv = self.surf.gv(self.u, self.v)

    def move_v(self, dv):
        if dv == 0:
            return
        self.v += dv
        fv2 = self.surf.gv(self.u, self.v)
        self.delta += 0.5 * dv * (self.fv + fv2)
        self.fv = fv2
        self.fu = self.surf.gu(self.u, self.v)

    def step(self):
        if abs(self.fu) > abs(self.fv):
            self.move_v(self.eps * sign(self.fu))
            self.move_u(rnd_move(fdiv(self.delta, self.fu)))
        else:
            self.move_u(-self.eps * sign(self.fv))
            self.move_v(rnd_move(fdiv(self.delta, self.fv)))

    def unstep(self):
        if abs(self.fu) > abs(self.fv):
            self.move_v(-self.eps * sign(self.fu))
            self.move_u(rnd_move(fdiv(self.delta, self.fu)))
        else:
            self.move_u(self.eps * sign(self.fv))
            self.move_v(rnd_move(fdiv(self.delta, self.fv)))

    def steps(self, n):
        if n > 0:
            for _ in range(n):
                self.step()
        else:
            for _ in range(-n):
                self.unstep()


def walk(poly, u, v, eu, ev, step_mult, n):
    """positions of a rasteriser after setStep(step_mult) and each of n steps (n < 0: unsteps): [|n| + 1][2]"""
    r = Raster(u, v, eu, ev, poly)
    r.eps *= step_mult
    out = [(r.u, r.v)]
    for _ in range(abs(n)):
        r.step() if n > 0 else r.unstep()
        out.append((r.u, r.v))
    return np.array(out, dtype=np.int32)


# ---- cameras, transform --------------------------------------------------------------------------------------------

def reconstruct(p, u, v):
    alpha, beta, fu, fv, u0, v0 = p
    xn = (u - u0) / fu
    yn = (v - v0) / fv
    u2 = xn * xn + yn * yn
    gamma = 1. - alpha
    num = 1. - u2 * alpha * alpha * beta
    det = 1 - (alpha - gamma) * beta * u2
    if det < 0:
        return None
    denom = gamma + alpha * math.sqrt(det)
    return (xn, yn, num / denom)


def project(p, X):
    alpha, beta, fu, fv, u0, v0 = p
    x, y, z = X
    denom = alpha * math.sqrt(z * z + beta * (x * x + y * y)) + (1. - alpha) * z
    if denom < 1e-3:
        return None
    if alpha > 0.5:
        zn = z / denom
        C = (alpha - 1.) / (alpha + alpha - 1.)
        if zn < C:
            return None
    return (fu * (x / denom) + u0, fv * (y / denom) + v0)


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def mat_vec(M, x):
    return tuple(M[3 * i] * x[0] + M[3 * i + 1] * x[1] + M[3 * i + 2] * x[2] for i in range(3))


def cross3(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def rotation_matrix(v, sgn):
    """rotationMatrix of the rotation vector sgn * v in the library's order (vg_geometry.hpp rotation_matrix)"""
    th = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    v0, v1, v2 = sgn * v[0], sgn * v[1], sgn * v[2]
    if th < 1e-5:
        return (1., -v2, v1, v2, 1., -v0, -v1, v0, 1.)
    s, c = math.sin(th), math.cos(th)
    thInv = 1. / th
    u1, u2, u3 = v0 * thInv, v1 * thInv, v2 * thInv
    cv = 1. - c
    return (1. + cv * (u1 * u1 - 1.), -s * u3 + cv * u1 * u2, s * u2 + cv * u1 * u3,
            s * u3 + cv * u2 * u1, 1. + cv * (u2 * u2 - 1.), -s * u1 + cv * u2 * u3,
            -s * u2 + cv * u3 * u1, s * u1 + cv * u3 * u2, 1. + cv * (u3 * u3 - 1.))


# ---- parameters ----------------------------------------------------------------------------------------------------

DEFAULTS = dict(scale=1, u0=0, v0=0, u_max=1, v_max=1, x_max=1, y_max=1, equal_margins=0, num_epipolar_planes=2000,
                epipole_margin=2500, disp_max=48, error_max=25, flaw_cost=7, desc_length=5, desc_resp_thresh=5,
                scales=[1, 2, 3, 5], step_cost=5, jump_cost=32, image_based_cost=1, salient_points_only=1, use_uv_cache=1)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    if p["equal_margins"]:
        p["x_max"] = (p["u_max"] - 2 * p["u0"]) // p["scale"] + 1
        p["y_max"] = (p["v_max"] - 2 * p["v0"]) // p["scale"] + 1
    return p


# ---- epipolar geometry ---------------------------------------------------------------------------------------------

def compute_polynomial(cam, ep, plane):
    alpha, beta, fu, fv, u0, v0 = cam
    gamma = 1 - alpha
    ag = alpha - gamma
    a2b = alpha * alpha * beta
    fufv, fufu, fvfv = fu * fv, fu * fu, fv * fv
    A, B, C = plane
    AA, BB, CC = A * A, B * B, C * C
    CCfufv = CC * fufv
    dd = fdiv(CCfufv, AA + BB)
    if (AA + BB) > 0 and dd < 1.:
        normABinv = 1. / math.sqrt(AA + BB)
        Cnorm = C / math.sqrt(AA + BB + CC)
        du = -A * Cnorm * normABinv * fu
        dv = -B * Cnorm * normABinv * fv
        return Poly2(0., 0., 0., A / fu, B / fv, -(u0 + du) * A / fu - (v0 + dv) * B / fv)
    kuu = (AA * ag + CC * a2b) / (CC * fufu)
    kuv = 2 * A * B * ag / (CCfufv)
    kvv = (BB * ag + CC * a2b) / (CC * fvfv)
    ku = 2 * (-(AA * fv * u0 + A * B * fu * v0) * ag - A * C * fufv * gamma - CC * a2b * fv * u0) / (CCfufv * fu)
    kv = 2 * (-(BB * fu * v0 + A * B * fv * u0) * ag - B * C * fufv * gamma - CC * a2b * fu * v0) / (CCfufv * fv)
    k1 = -(kuu * ep[0] * ep[0] + kuv * ep[0] * ep[1] + kvv * ep[1] * ep[1] + ku * ep[0] + kv * ep[1])
    return Poly2(kuu, kuv, kvv, ku, kv, k1)


class Geometry:
    """everything EnhancedSgm's constructor computes: transform, epipoles, curve tables, per-pixel geometry"""

    def __init__(self, c1, c2, xi, prm):
        self.c1, self.c2, self.p = tuple(map(float, c1)), tuple(map(float, c2)), prm
        xi = [float(v) for v in xi]
        self.R = rotation_matrix(xi[3:], 1.)
        self.Rinv = rotation_matrix(xi[3:], -1.)
        self.t = tuple(xi[:3])
        t = self.t
        ti = tuple(-v for v in mat_vec(self.Rinv, t))
        self.ep, self.ep_ok, self.ep_px = {}, {}, {}
        for cam, c, pts in ((0, self.c1, (t, tuple(-v for v in t))), (1, self.c2, (ti, tuple(-v for v in ti)))):
            for k in range(2):
                e = project(c, pts[k])
                self.ep_ok[cam, k] = e is not None
                if e is None:
                    self.ep[cam, k], self.ep_px[cam, k] = (0., 0.), (0, 0)
                    continue
                e = tuple(max(-1e6, min(1e6, v)) for v in e)
                self.ep[cam, k] = e
                self.ep_px[cam, k] = (cround(e[0]), cround(e[1]))
            if not self.ep_ok[cam, 0] and not self.ep_ok[cam, 1]:
                raise ValueError("neither epipole projects into camera %d" % (cam + 1))
        n = prm["num_epipolar_planes"]
        self.n = n
        self.pstep = 4. / n
        tn = math.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2])
        z = tuple(-(v / tn) for v in t)
        self.z = z
        axis = 0 if z[2] * z[2] > z[0] * z[0] + z[1] * z[1] else 2
        xb = tuple((1. if i == axis else 0.) - z[i] * z[axis] for i in range(3))
        xn = math.sqrt(xb[0] * xb[0] + xb[1] * xb[1] + xb[2] * xb[2])
        self.xb = tuple(v / xn for v in xb)
        self.yb = cross3(z, self.xb)
        z2 = mat_vec(self.Rinv, z)
        self.table = [[], []]
        for cam, c in ((0, self.c1), (1, self.c2)):
            ep = self.ep[cam, 0 if self.ep_ok[cam, 0] else 1]
            for idx in range(n):
                if idx < n // 2:
                    s = self.pstep * idx - 1
                    d = tuple(self.xb[i] + s * self.yb[i] for i in range(3))
                else:
                    cc = self.pstep * (-idx + n // 2) + 1
                    d = tuple(cc * self.xb[i] + self.yb[i] for i in range(3))
                plane = cross3(d, z) if cam == 0 else cross3(mat_vec(self.Rinv, d), z2)
                self.table[cam].append(compute_polynomial(c, ep, plane))
            self.table[cam].append(self.table[cam][0])
        self.pixels()

    def index(self, X):
        c = dot3(X, self.xb)
        s = dot3(X, self.yb)
        ac, as_ = abs(c), abs(s)
        if ac + as_ < 1e-4:
            return 0
        i = cround((s / c + 1) / self.pstep) if ac > as_ else cround((1 - c / s) / self.pstep) + self.n // 2
        return max(0, min(self.n, i))

    def choose(self, cam, u, v):
        e, a = self.ep_px[cam, 0], self.ep_px[cam, 1]
        du, dv = float(u) - e[0], float(v) - e[1]
        au, av = float(u) - a[0], float(v) - a[1]
        dist, anti = du * du + dv * dv, au * au + av * av
        th = self.p["epipole_margin"]
        res = 0
        if self.ep_ok[cam, 0] and self.ep_ok[cam, 1]:
            if anti < dist:
                res |= INVERTED
                if anti < th:
                    res |= TOO_CLOSE
            elif dist < th:
                res |= TOO_CLOSE
        elif self.ep_ok[cam, 0]:
            if dist < th:
                res |= TOO_CLOSE
        else:
            res |= INVERTED
            if anti < th:
                res |= TOO_CLOSE
        return res

    def uv1(self, x, y):
        p = self.p
        return x * p["scale"] + p["u0"], y * p["scale"] + p["v0"]

    def pixels(self):
        """geometry int32 [y][x][8]: status, pinf u, v, index, flags1, flags2, 0, 0"""
        p = self.p
        g = np.zeros((p["y_max"], p["x_max"], 8), np.int32)
        for y in range(p["y_max"]):
            for x in range(p["x_max"]):
                u, v = self.uv1(x, y)
                X = reconstruct(self.c1, float(u), float(v))
                if X is None:
                    continue
                g[y, x, 0] = 1
                g[y, x, 3] = self.index(X)
                g[y, x, 4] = self.choose(0, u, v)
                pinf = project(self.c2, mat_vec(self.Rinv, X))
                if pinf is None:
                    continue
                g[y, x, 0] |= 2
                g[y, x, 1], g[y, x, 2] = cround(pinf[0]), cround(pinf[1])
                g[y, x, 5] = self.choose(1, g[y, x, 1], g[y, x, 2])
        self.geom = g

    def raster(self, cam, u, v, index, flags):
        inv = 1 if flags & INVERTED else 0
        e = self.ep_px[cam, inv]
        r = Raster(u, v, e[0], e[1], self.table[cam][index])
        if inv:
            r.eps *= -1
        return r


# ---- matching cost -------------------------------------------------------------------------------------------------

def compare_descriptor(desc, samples, flaw):
    """compareDescriptor (eucm_stereo.cpp:78-218): cost per sample position"""
    desc = [int(d) for d in desc]
    L = len(desc)
    lo, hi = [0] * L, [0] * L
    for i in range(1, L - 1):
        d, d1, d2 = desc[i], (desc[i] + desc[i - 1]) // 2, (desc[i] + desc[i + 1]) // 2
        lo[i], hi[i] = min(d, d1, d2), max(d, d1, d2)
    for i, j in ((0, 1), (L - 1, L - 2)):
        m = (desc[i] + desc[j]) // 2
        if desc[i] > desc[j]:
            lo[i], hi[i] = m, desc[i]
        else:
            lo[i], hi[i] = desc[i], m
    s = np.asarray(samples, dtype=np.int64)
    N = len(s)
    H = L // 2

    def err(i):
        return np.maximum(0, np.maximum(lo[i] - s, s - hi[i]))

    big = np.full(2, INF, np.int64)
    A = err(0)
    for i in range(1, H + 1):
        Ap = np.concatenate([big, A])
        A = np.minimum(np.minimum(A + flaw, Ap[1:N + 1]), Ap[:N] + flaw) + err(i)
    C = A
    A = err(L - 1)
    for i in range(L - 2, H, -1):
        An = np.concatenate([A, big])
        A = np.minimum(np.minimum(A + flaw, An[1:N + 1]), An[2:N + 2] + flaw) + err(i)
    An = np.concatenate([A, big])
    return C + np.minimum(np.minimum(A + flaw, An[1:N + 1]), An[2:N + 2] + flaw)


def fill_gaps(data, step, D):
    """fillGaps (eucm_sgm.cpp:407-448), case 3 as (2 a + b) / 3, (a + 2 b) / 3"""
    base = step
    while base < D:
        a, b = int(data[base - step]), int(data[base])
        for i in range(step - 1, 0, -1):
            data[base - i] = (a * i + b * (step - i)) // step
        base += step
    base -= step
    data[base + 1:D] = data[base]


def descriptor(img1, r0, prm):
    """EpipolarDescriptor::compute: (step, response, descriptor)"""
    L = prm["desc_length"]
    H = L // 2
    h, w = img1.shape
    resp, desc, step = 0, None, -1
    for sc in prm["scales"]:
        r = r0.copy()
        r.eps *= -sc
        r.steps(-H)
        desc = []
        for i in range(L):
            if i > 0:
                r.step()
            if r.v < 0 or r.v >= h or r.u < 0 or r.u >= w:
                return -1, resp, desc
            desc.append(int(img1[r.v, r.u]))
        tv = sum(abs(desc[i - 1] - desc[i]) for i in range(1, L))
        resp = (tv * 100) // (desc[H] + 30)
        step = sc
        if abs(resp) > prm["desc_resp_thresh"] * L:
            break
    return step, resp, desc


def cache_walk(G, g):
    """the uv-cache walk: a rasteriser kDisparityMargin unsteps back from pinf; .go(k) moves it to cache position k"""
    r = G.raster(1, int(g[1]), int(g[2]), int(g[3]), int(g[5]))
    r.steps(-DISPARITY_MARGIN)
    state = {"k": 0}

    def go(k):
        r.steps(k - state["k"])
        state["k"] = k
        return r.u, r.v

    return go


def curve_cost(G, img1, img2):
    """computeCurveCost: err uint8 [y][x][D], step, salient, skip uint8 [y][x]"""
    p = G.p
    Y, X, D, L = p["y_max"], p["x_max"], p["disp_max"], p["desc_length"]
    H = L // 2
    h, w = img2.shape
    err = np.zeros((Y, X, D), np.uint8)
    stepb, sal, skip = (np.zeros((Y, X), np.uint8) for _ in range(3))

    def skip_pixel(y, x):
        err[y, x, 0] = 0
        err[y, x, 1:] = 255
        skip[y, x] = 1

    for y in range(Y):
        for x in range(X):
            g = G.geom[y, x]
            if not (g[0] & 1) or not (g[0] & 2) or (g[4] & TOO_CLOSE):
                skip_pixel(y, x)
                continue
            u, v = G.uv1(x, y)
            step, resp, desc = descriptor(img1, G.raster(0, u, v, int(g[3]), int(g[4])), p)
            if step < 1:
                skip_pixel(y, x)
                continue
            stepb[y, x] = step
            if p["salient_points_only"] and step < 2 and abs(resp) > p["desc_resp_thresh"] * L:
                sal[y, x] = 1
            n_steps = (D + step - 1) // step
            N = n_steps + L - 1
            samples, crossed = [], False
            if p["use_uv_cache"]:
                go = cache_walk(G, g)
                pos = [go(DISPARITY_MARGIN - H * step + i * step) for i in range(N)]
            else:
                r = G.raster(1, int(g[1]), int(g[2]), int(g[3]), int(g[5]))
                r.eps *= step
                r.steps(-H)
                pos = []
                for i in range(N):
                    if i > 0:
                        r.step()
                    pos.append((r.u, r.v))
            for su, sv in pos:
                if sv < 0 or sv >= h or su < 0 or su >= w:
                    crossed = True
                    break
                samples.append(int(img2[sv, su]))
            if crossed:
                skip_pixel(y, x)
                continue
            cost = compare_descriptor(desc, samples, p["flaw_cost"])
            row = err[y, x]
            for d in range(n_steps):
                row[d * step] = min(int(cost[H + d]), 255)
            if step > 1:
                fill_gaps(row, step, D)
    return err, stepb, sal, skip


# ---- aggregation ---------------------------------------------------------------------------------------------------

def jump_costs(prm, step):
    """_costBuffer: 8-bit jump_cost x {1, 3, 6} by step; jump_cost where the step was never set"""
    J = prm["jump_cost"]
    if not prm["image_based_cost"]:
        return np.full(step.shape, J, np.int64)
    k = np.where(step == 1, 1, np.where(step == 2, 3, 6))
    return np.where(step == 0, J, (J * k) & 255).astype(np.int64)


def _dp(err, jump, lam):
    """one direction over axis 0 of err [n][lines][D] (int64), jump [n][lines]: the tableau [n][lines][D]"""
    out = np.empty_like(err)
    c = err[0].copy()
    out[0] = c
    big = np.full(c.shape[:-1] + (1,), INF, np.int64)
    for i in range(1, err.shape[0]):
        best = c.min(axis=-1, keepdims=True)
        right = np.concatenate([c[..., 1:], big], axis=-1) + lam
        left = np.concatenate([big, c[..., :-1]], axis=-1) + lam
        c = np.minimum(np.minimum(np.minimum(c, right), left), best + jump[i][..., None]) + err[i]
        out[i] = c
    return out


def aggregate(prm, err, step):
    """L + R + T + B (computeDynamicProgramming) of err [Y][X][D]: int64 [Y][X][D]"""
    e = err.astype(np.int64)
    jmp = jump_costs(prm, step)
    lam = prm["step_cost"]
    ex, jx = e.transpose(1, 0, 2), jmp.T          # [X][Y][D]: rows scan along x
    Lt = _dp(ex, jx, lam).transpose(1, 0, 2)
    Rt = _dp(ex[::-1], jx[::-1], lam)[::-1].transpose(1, 0, 2)
    Tt = _dp(e, jmp, lam)
    Bt = _dp(e[::-1], jmp[::-1], lam)[::-1]
    return Lt + Rt + Tt + Bt


def winner(prm, err, total, sal, skip):
    """reconstructDisparity: int32 [Y][X], -1 where none"""
    e = err.astype(np.int64)
    cost = total - 2 * e
    cost[..., 0] = np.iinfo(np.int64).max
    cost = np.where(e > prm["error_max"], np.iinfo(np.int64).max, cost)
    d = cost.argmin(axis=-1)
    none = cost.min(axis=-1) == np.iinfo(np.int64).max
    off = skip.astype(bool) | (bool(prm["salient_points_only"]) & (sal == 0))
    return np.where(none | off, -1, d).astype(np.int32)


# ---- depth ---------------------------------------------------------------------------------------------------------

def reg_div(num, den):
    eps = 1e-3
    if den > eps * num:
        return num / den
    if num == 0:
        return 2. / eps
    return 2. / eps - den / (num * eps * eps)


def tri_lambda(R, t, p, q0):
    q = mat_vec(R, q0)
    r = tuple(p[i] + q[i] for i in range(3))
    tp, tq, tr, tt = dot3(t, p), dot3(t, q), dot3(t, r), dot3(t, t)
    rp, rq = dot3(r, p), dot3(r, q)
    return reg_div(tt * rq - tr * tq, tp * rq - tq * rp)


def depth(G, err, step, sal, skip, disp):
    """reconstructDepth with the six-argument triangulate: depth, sigma, cost float64 [Y][X]"""
    p = G.p
    Y, X = p["y_max"], p["x_max"]
    dep, sig, cst = (np.zeros((Y, X)) for _ in range(3))
    h, w = p["v_max"], p["u_max"]
    for y in range(Y):
        for x in range(X):
            g = G.geom[y, x]
            if (p["salient_points_only"] and not sal[y, x]) or skip[y, x] or not (g[0] & 1):
                continue
            cst[y, x] = float(err[y, x, 0])
            d, s = int(disp[y, x]), int(step[y, x])
            if p["use_uv_cache"]:
                go = cache_walk(G, g)
                pts = []
                for k in (DISPARITY_MARGIN + d, DISPARITY_MARGIN + d + s):
                    u2, v2 = go(k)
                    pts.append((u2, v2) if 0 <= u2 < w and 0 <= v2 < h else (-1, -1))
            else:
                r = G.raster(1, int(g[1]), int(g[2]), int(g[3]), int(g[5]))
                r.steps(d)
                pts = [(r.u, r.v)]
                r.steps(s)
                pts.append((r.u, r.v))
            u1, v1 = G.uv1(x, y)
            P = reconstruct(G.c1, float(u1), float(v1))
            q1 = reconstruct(G.c2, float(pts[0][0]), float(pts[0][1]))
            q2 = reconstruct(G.c2, float(pts[1][0]), float(pts[1][1]))
            if P is None or q1 is None or q2 is None:
                continue
            pn = math.sqrt(dot3(P, P))
            l1 = tri_lambda(G.R, G.t, P, q1) * pn
            l2 = tri_lambda(G.R, G.t, P, q2) * pn
            if l1 < 100.:
                sig[y, x] = abs(l2 - l1)
                dep[y, x] = l1
    return dep, sig, cst


def stereo(c1, c2, xi, prm, img1, img2, G=None):
    """the whole pipeline for one pair: dict of every stage's output"""
    G = G or Geometry(c1, c2, xi, prm)
    err, step, sal, skip = curve_cost(G, img1, img2)
    total = aggregate(prm, err, step)
    disp = winner(prm, err, total, sal, skip)
    dep, sig, cst = depth(G, err, step, sal, skip, disp)
    return dict(geom=G.geom, err=err, step=step, salient=sal, skip=skip, total=total, disparity=disp, depth=dep, sigma=sig,
                cost=cst)
