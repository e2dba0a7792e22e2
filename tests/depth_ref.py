"""Plain-Python restatement of the reference's DepthMap::wrapDepth, merge and filterNoise (src/reconstruction/depth_map.cpp:723-760,
917-958, 868-914) with the deviations of DESIGN.md section 9 ("Depth map propagation"), for the depth fusion tests.  Built on
tests/stereo_ref.py (EUCM reconstruct / project, C round, IEEE division, the rotation matrix) and tests/motion_ref.py (fuse);
scalar FP64 in the library's evaluation order, so it agrees with the GPU bit for bit.  Written from reading the reference, not
pinned to its outputs."""
import math

import numpy as np

from tests import motion_ref as mr
from tests import stereo_ref as sr

MIN_DEPTH, DEFAULT_SIGMA, DEFAULT_COST = mr.MIN_DEPTH, 30., 5.
# the sequential loops of the reference, pixel by pixel
DX = (-1, 0, 1, 1, 1, 0, -1, -1)
DY = (1, 1, 1, 0, -1, -1, -1, 0)


def grid(prm):
    """(scale, u0, v0, x_max, y_max) of a stereo_ref / motion_ref parameter dict"""
    return prm["scale"], prm["u0"], prm["v0"], prm["x_max"], prm["y_max"]


def warp(cam, prm, xi, depth, sigma, cost):
    """wrapDepth(T12): dict(depth, sigma, cost float64 [Y][X], counts int64 [6]: sources, dropped by reconstruct, dropped by
    project, outside the map, lost the depth test, targets written)"""
    scale, u0, v0, X, Y = grid(prm)
    cam = tuple(map(float, cam))
    xi = [float(v) for v in xi]
    Rinv, t = sr.rotation_matrix(xi[3:], -1.), xi[:3]
    dep, sig, cst = np.zeros((Y, X)), np.full((Y, X), DEFAULT_SIGMA), np.full((Y, X), DEFAULT_COST)
    counts = np.zeros(6, np.int64)
    for y in range(Y):       # ascending source index, strict "<": the nearest source wins, on a tie the first
        for x in range(X):
            d = float(depth[y, x])
            if not d >= MIN_DEPTH:
                continue
            counts[0] += 1
            P = sr.reconstruct(cam, float(x * scale + u0), float(y * scale + v0))
            if P is None:
                counts[1] += 1
                continue
            nrm = math.sqrt(sr.dot3(P, P))
            X1 = tuple(sr.fdiv(P[i], nrm) * d - t[i] for i in range(3))
            X2 = sr.mat_vec(Rinv, X1)
            q = sr.project(cam, X2)
            dist = math.sqrt(sr.dot3(X2, X2))
            if q is None or not dist > 0.:
                counts[2] += 1
                continue
            if not mr.coord_ok(q):
                counts[3] += 1
                continue
            xd, yd = sr.cround((q[0] - u0) / scale), sr.cround((q[1] - v0) / scale)
            if xd < 0 or xd >= X or yd < 0 or yd >= Y:
                counts[3] += 1
                continue
            if dep[yd, xd] == 0. or dist < dep[yd, xd]:
                if dep[yd, xd] != 0.:
                    counts[4] += 1   # the earlier holder loses
                dep[yd, xd] = dist
                sig[yd, xd] = float(sigma[y, x]) + 0.005 * dist
                cst[yd, xd] = float(cost[y, x])
            else:
                counts[4] += 1
    counts[5] = int((dep != 0).sum())
    return dict(depth=dep, sigma=sig, cost=cst, counts=counts)


def merge(depth, sigma, depth2, sigma2):
    """merge(depth2): dict(depth, sigma, counts int64 [5]: skipped, copied, fused, replaced, kept); the inputs are not modified"""
    dep, sig = np.array(depth, dtype=np.float64, copy=True), np.array(sigma, dtype=np.float64, copy=True)
    counts = np.zeros(5, np.int64)
    Y, X = dep.shape
    for y in range(Y):
        for x in range(X):
            d2 = float(depth2[y, x])
            if d2 < MIN_DEPTH or d2 == 0.:
                counts[0] += 1
                continue
            s2 = float(sigma2[y, x])
            d, s = float(dep[y, x]), float(sig[y, x])
            if d == 0.:
                dep[y, x], sig[y, x] = d2, s2
                counts[1] += 1
            elif abs(d - d2) < 2 * (s + s2):
                dep[y, x], sig[y, x] = mr.fuse(d, s, d2, s2)
                counts[2] += 1
            elif d2 < d:
                dep[y, x], sig[y, x] = d2, s2
                counts[3] += 1
            else:
                counts[4] += 1
    return dict(depth=dep, sigma=sig, counts=counts)


def filter_noise(depth, sigma):
    """filterNoise: dict(depth, sigma, counts int64 [3]: interior pixels with a depth, cleared, smoothed)"""
    src, ssrc = np.asarray(depth, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    dep, sig = src.copy(), ssrc.copy()
    counts = np.zeros(3, np.int64)
    Y, X = src.shape
    for y in range(1, Y - 1):
        for x in range(1, X - 1):
            d = float(src[y, x])
            if d == 0.:
                continue
            counts[0] += 1
            s = float(ssrc[y, x])
            filled = matches = 0
            acc = d * 5
            for i in range(8):
                x2, y2 = x + DX[i], y + DY[i]
                nd = float(src[y2, x2])
                if nd == 0.:
                    continue
                filled += 1
                err = abs(d - nd)
                if err > s or err > 3 * float(ssrc[y2, x2]):
                    continue
                matches += 1
                acc += nd
            if (matches < 2 and matches < filled) or filled < 2:
                dep[y, x] = sig[y, x] = 0.
                counts[1] += 1
            else:
                dep[y, x] = acc / (matches + 5)
                counts[2] += 1
    return dict(depth=dep, sigma=sig, counts=counts)
