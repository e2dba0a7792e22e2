"""Plain-Python restatement of the reference's MotionStereo (src/reconstruction/eucm_motion_stereo.cpp) with the deviations
of DESIGN.md section 9 ("Motion stereo"), for the motion stereo tests.  Built on tests/stereo_ref.py (rasteriser, curve tables,
epipoles, descriptor, compareDescriptor, EUCM reconstruct / project, regular triangulation); scalar FP64 in the library's
evaluation order, so every stage agrees with the GPU bit for bit.  Written from reading the reference, not pinned to its
outputs (there is no OpenCV / Eigen here to build it with)."""
import math

import numpy as np

from tests import stereo_ref as sr

REJ_SELECT, REJ_UNCERTAINTY, TOO_CERTAIN, REJ_SAMPLE, NOT_UPDATED, UPDATED = 1, 2, 3, 4, 5, 6
MIN_DEPTH = 0.25
COORD_LIMIT = 16777216.
# record fields, as vg_motion_stereo_select writes them
STATUS, GSTEP, GU2, GV2, SU, SV, FU, FV, DISP_MAX, INVERTED, BEST, BEST_COST, INDEX2 = range(13)
# OpenCV's getGaussianKernel for ksize 7, sigma <= 0: a fixed table, exact in float
GAUSS7 = np.array([0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125], dtype=np.float32)


def params(gradient_thresh=2, **kw):
    p = sr.params(**kw)
    p["gradient_thresh"] = gradient_thresh
    return p


def reflect101(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def compute_mask(img, thresh):
    """computeMask: Sobel(ksize 1) x and y, |gx| + |gy|, 7 x 7 Gaussian (sigma 0), u8, threshold to 0 / 128; reflect-101"""
    h, w = img.shape
    im = img.astype(np.int32)
    cx = np.array([reflect101(i, w) for i in range(-1, w + 1)])
    cy = np.array([reflect101(i, h) for i in range(-1, h + 1)])
    gx = im[:, cx[2:]] - im[:, cx[:-2]]
    gy = im[cy[2:], :] - im[cy[:-2], :]
    g = (np.abs(gx) + np.abs(gy)).astype(np.float32)
    bx = np.array([reflect101(i, w) for i in range(-3, w + 3)])
    by = np.array([reflect101(i, h) for i in range(-3, h + 3)])
    rows = np.zeros((h, w), np.float32)
    for k in range(7):
        rows = rows + GAUSS7[k] * g[:, bx[k:k + w]]
    out = np.zeros((h, w), np.float32)
    for k in range(7):
        out = out + GAUSS7[k] * rows[by[k:k + h], :]
    v = np.clip(np.rint(out), 0, 255).astype(np.int32)   # rint: half to even
    return np.where(v > thresh, 128, 0).astype(np.uint8)


def fuse(v1, s1, v2, s2):
    """filter (depth_map.cpp:32-37): the merged (value, sigma)"""
    K = sr.fdiv(1., s1 + s2)
    v = (v1 * s2 + v2 * s1) * K
    a, b = s1 * s2 * K, 0.05 * v
    return v, (b if a < b else a)


def dmax(a, b):
    return b if a < b else a


def coord_ok(pt):
    return abs(pt[0]) <= COORD_LIMIT and abs(pt[1]) <= COORD_LIMIT


class MotionStereo:
    """MotionStereo for one pair of cameras and one key frame"""

    def __init__(self, c1, c2, prm):
        self.c1, self.c2, self.p = tuple(map(float, c1)), tuple(map(float, c2)), prm
        self.img1 = self.mask = self.G = None

    def set_base(self, img1):
        self.img1 = np.ascontiguousarray(img1, dtype=np.uint8)
        self.mask = compute_mask(self.img1, self.p["gradient_thresh"])

    def set_transformation(self, xi):
        # Geometry also fills the per-pixel table of the SGM restatement, which nothing here reads
        self.G = sr.Geometry(self.c1, self.c2, xi, self.p)

    def select_point(self, x, y, rec):
        """selectPoint: (ok, gX, descriptor); writes gstep, gu2, gv2 into rec once they exist"""
        p, G = self.p, self.G
        u, v = G.uv1(x, y)
        h, w = self.img1.shape
        if u < 0 or u >= w or v < 0 or v >= h:
            return False, None, None
        if int(self.mask[v, u]) < p["gradient_thresh"]:
            return False, None, None
        X = sr.reconstruct(self.c1, float(u), float(v))
        if X is None:
            return False, None, None
        flags = G.choose(0, u, v)
        if flags & sr.TOO_CLOSE:
            return False, None, None
        ref = G.raster(0, u, v, G.index(X), flags)
        step, resp, desc = sr.descriptor(self.img1, ref, p)
        rec[GSTEP] = step
        ru = ref.copy()
        ru.eps *= step
        ru.step()
        rec[GU2], rec[GV2] = ru.u, ru.v
        if step != 1 or not abs(resp) > p["desc_resp_thresh"] * p["desc_length"]:
            return False, None, None
        return True, X, desc

    def compute_uncertainty(self, X, d, s, rec):
        """computeUncertainty: ok; writes the start / end points, gdispMax, the inverted flag and the camera 2 curve index"""
        p, G = self.p, self.G
        if d == 0.:
            ps = sr.project(self.c2, sr.mat_vec(G.Rinv, X))
            if ps is None or not coord_ok(ps):
                return False
            su, sv = sr.cround(ps[0]), sr.cround(ps[1])
            rec[SU], rec[SV] = su, sv
            fl = G.choose(1, su, sv)
            if fl & sr.TOO_CLOSE:
                return False
            inv = 1 if fl & sr.INVERTED else 0
            fu, fv = G.ep_px[1, inv]
            rec[FU], rec[FV] = fu, fv
            if inv:
                rec[DISP_MAX], rec[INVERTED] = p["disp_max"], 1
            else:
                rec[DISP_MAX] = min(p["disp_max"], max(abs(su - fu), abs(sv - fv)))
        else:
            nrm = math.sqrt(sr.dot3(X, X))
            X = tuple(sr.fdiv(c, nrm) for c in X)
            far, near = d + 3 * s, dmax(d - 3 * s, MIN_DEPTH)
            Xa = tuple(X[i] * far - G.t[i] for i in range(3))
            Xb = tuple(X[i] * near - G.t[i] for i in range(3))
            ps = sr.project(self.c2, sr.mat_vec(G.Rinv, Xa))
            if ps is None or not coord_ok(ps):
                return False
            pf = sr.project(self.c2, sr.mat_vec(G.Rinv, Xb))
            if pf is None or not coord_ok(pf):
                return False
            rec[DISP_MAX] = min(p["disp_max"], sr.cround(dmax(abs(pf[0] - ps[0]), abs(pf[1] - ps[1]))))
            rec[SU], rec[SV] = sr.cround(ps[0]), sr.cround(ps[1])
            rec[FU], rec[FV] = sr.cround(pf[0]), sr.cround(pf[1])
        rec[INDEX2] = G.index(X)
        return True

    def _raster2(self, rec):
        r = sr.Raster(int(rec[SU]), int(rec[SV]), int(rec[FU]), int(rec[FV]), self.G.table[1][int(rec[INDEX2])])
        if rec[INVERTED]:
            r.eps *= -1
        r.steps(-(self.p["desc_length"] // 2))
        return r

    def sample_image(self, img2, rec):
        """sampleImage: (samples, positions) or None when the walk leaves the image"""
        h, w = img2.shape
        r = self._raster2(rec)
        samples, pos = [], []
        for i in range(int(rec[DISP_MAX]) + self.p["desc_length"] - 1):
            if i > 0:
                r.step()
            if r.v < 0 or r.v >= h or r.u < 0 or r.u >= w:
                return None
            samples.append(int(img2[r.v, r.u]))
            pos.append((r.u, r.v))
        return samples, pos

    def reconstruct(self, x, y, desc, samples, pos, rec, dist, sigma, cost):
        """reconstruct: (updated, dist, sigma, cost)"""
        p, G = self.p, self.G
        H = p["desc_length"] // 2
        cv = sr.compare_descriptor(desc, samples, p["flaw_cost"])
        seg = cv[H:len(cv) - H]
        best = H + int(np.argmin(seg))   # the first minimum, as min_element
        bc = int(cv[best])
        rec[BEST], rec[BEST_COST] = best, bc
        if not (bc < p["error_max"] and float(bc) < 2 * cost):
            return False, dist, sigma, cost
        u, v = G.uv1(x, y)
        p1 = sr.reconstruct(self.c1, float(u), float(v))
        p2 = sr.reconstruct(self.c1, float(rec[GU2]), float(rec[GV2]))
        q1 = sr.reconstruct(self.c2, float(pos[best][0]), float(pos[best][1]))
        q2 = sr.reconstruct(self.c2, float(pos[best + 1][0]), float(pos[best + 1][1]))
        if p1 is None or p2 is None or q1 is None or q2 is None:
            return False, dist, sigma, cost
        pn = math.sqrt(sr.dot3(p1, p1))
        l1 = sr.tri_lambda(G.R, G.t, p1, q1) * pn
        l2 = sr.tri_lambda(G.R, G.t, p2, q2) * pn
        sn = abs(l2 - l1)
        if dist != 0.:
            dist, sigma = fuse(dist, sigma, l1, sn)
            cost = cost * 0.7 + bc * 0.3
        else:
            dist, sigma, cost = l1, sn, float(bc)
        return True, dist, sigma, cost

    def compute(self, xi, img2, prior=None):
        """both overloads of compute: dict(depth, sigma, cost float64 [Y][X], record int32 [Y][X][16], counts int64 [6])"""
        p = self.p
        self.set_transformation(xi)
        Y, X = p["y_max"], p["x_max"]
        if prior is None:
            dep, sig, cst = np.zeros((Y, X)), np.zeros((Y, X)), np.full((Y, X), float(p["error_max"]))
        else:
            dep, sig, cst = (np.array(a, dtype=np.float64, copy=True) for a in prior)
        record = np.zeros((Y, X, 16), np.int32)
        for y in range(Y):
            for x in range(X):
                rec = record[y, x]
                rec[STATUS] = self._pixel(x, y, img2, prior is not None, rec, dep, sig, cst)
        st = record[..., STATUS]
        counts = np.array([(st == 1).sum(), (st == 2).sum(), (st == 3).sum(), (st == 4).sum(), (st >= 5).sum(), (st == 6).sum()],
                          dtype=np.int64)
        return dict(depth=dep, sigma=sig, cost=cst, record=record, counts=counts)

    def _pixel(self, x, y, img2, with_prior, rec, dep, sig, cst):
        ok, X, desc = self.select_point(x, y, rec)
        if not ok:
            return REJ_SELECT
        if not self.compute_uncertainty(X, float(dep[y, x]), float(sig[y, x]), rec):
            return REJ_UNCERTAINTY
        if rec[DISP_MAX] < (2 if with_prior else 1):
            return TOO_CERTAIN
        sp = self.sample_image(img2, rec)
        if sp is None:
            return REJ_SAMPLE
        upd, d, s, c = self.reconstruct(x, y, desc, sp[0], sp[1], rec, float(dep[y, x]), float(sig[y, x]), float(cst[y, x]))
        if not upd:
            return NOT_UPDATED
        dep[y, x], sig[y, x], cst[y, x] = d, s, c
        return UPDATED
