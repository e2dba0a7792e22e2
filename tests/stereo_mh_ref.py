"""Restatement of multi-hypothesis stereo, on top of tests/stereo_ref.py: EnhancedSgm::reconstructDisparityMH
(eucm_sgm.cpp:628-738), reconstructDepth over the hypothesis planes (eucm_sgm.cpp:154-218), DepthMap::regularize
(depth_map.cpp:960-983) and DepthMap::reconstruct(pack, ALL_HYPOTHESES | SIGMA_VALUE) (depth_map.cpp:532-635).  Plain Python,
written from the rule and not from the kernels: a pixel is a loop over its valid disparities.

The winner of one pixel.  V: the disparities d in [0, D), ascending, whose matching error is at most error_max; c(d) = total[d]
- 2 err[d].  v_i is a candidate when it has a successor in V, c(v_i) < c(v_i+1) and (i = 0 or c(v_i) <= c(v_i-1)); it reports
r_i = v_i+1 - 1 (the reference's d - 1 at the time it sees the successor).  With (m, r) = (0, -1), hypothesis h takes the
cheapest candidate (the first on a tie) with (c > m or (c = m and r_i != r)) and (h = 0 or c <= m + hypo_difference), and
(m, r) becomes what it took; when there is none, h and every later hypothesis are -1.  final_cost is c, INT32_MAX where the
disparity is -1 (the reference leaves stale values there)."""
import math

import numpy as np

from tests import stereo_ref as sr

MIN_DEPTH = 0.25
NO_COST = np.iinfo(np.int32).max


def candidates(err_row, total_row, error_max):
    """[(c, r)] of one pixel, in ascending order of the disparity"""
    V = [d for d in range(len(err_row)) if int(err_row[d]) <= error_max]
    c = [int(total_row[d]) - 2 * int(err_row[d]) for d in V]
    out = []
    for i in range(len(V) - 1):
        if c[i] < c[i + 1] and (i == 0 or c[i] <= c[i - 1]):
            out.append((c[i], V[i + 1] - 1))
    return out


def select(cands, hyp_max, hypo_difference):
    """(disparity [hyp_max], final_cost [hyp_max]) from one pixel's candidates"""
    disp, cost = [-1] * hyp_max, [NO_COST] * hyp_max
    m, r = 0, -1
    for h in range(hyp_max):
        best = None
        for c, ri in cands:
            if not (c > m or (c == m and ri != r)):
                continue
            if h > 0 and c > m + hypo_difference:
                continue
            if best is None or c < best[0]:
                best = (c, ri)
        if best is None:
            break
        disp[h], cost[h] = best[1], best[0]
        m, r = best
    return disp, cost


def select_row(err_row, total_row, error_max, hyp_max, hypo_difference):
    return select(candidates(err_row, total_row, error_max), hyp_max, hypo_difference)


def winner_mh(prm, err, total, sal, hyp_max, hypo_difference):
    """reconstructDisparityMH: (disparity, final_cost) int32 [hyp_max][Y][X]; the skip buffer is not consulted"""
    Y, X, _ = err.shape
    disp = np.full((hyp_max, Y, X), -1, np.int32)
    cost = np.full((hyp_max, Y, X), NO_COST, np.int32)
    for y in range(Y):
        for x in range(X):
            if prm["salient_points_only"] and not sal[y, x]:
                continue
            d, c = select_row(err[y, x], total[y, x], prm["error_max"], hyp_max, hypo_difference)
            disp[:, y, x] = d
            cost[:, y, x] = c
    return disp, cost


def depth_mh(G, err, step, sal, skip, disp):
    """reconstructDepth per plane: (depth, sigma, cost) float64 [hyp_max][Y][X]; the cost of plane h is err[y][x][h]"""
    planes = [sr.depth(G, err[:, :, h:], step, sal, skip, disp[h]) for h in range(disp.shape[0])]
    return tuple(np.stack([p[i] for p in planes]) for i in range(3))


def stereo_mh(c1, c2, xi, prm, img1, img2, hyp_max, hypo_difference, base=None, G=None):
    """the whole pipeline for one pair with hyp_max hypotheses; base: sr.stereo's output for the same arguments, if at hand
    (it is not changed)"""
    G = G or sr.Geometry(c1, c2, xi, prm)
    base = base or sr.stereo(c1, c2, xi, prm, img1, img2, G)
    disp, final = winner_mh(prm, base["err"], base["total"], base["salient"], hyp_max, hypo_difference)
    dep, sig, cst = depth_mh(G, base["err"], base["step"], base["salient"], base["skip"], disp)
    return dict(disparity=disp, final_cost=final, depth=dep, sigma=sig, cost=cst)


def regularize(depth, sigma, cost):
    """DepthMap::regularize of [hyp_max][Y][X] maps: new arrays"""
    depth, sigma, cost = (np.array(a, dtype=np.float64) for a in (depth, sigma, cost))
    H, Y, X = depth.shape
    for h in range(H - 1):
        for y in range(Y):
            for x in range(X):
                if depth[h, y, x] < MIN_DEPTH:
                    h2 = h + 1
                    while h2 < H and depth[h2, y, x] < MIN_DEPTH:
                        h2 += 1
                    if h2 == H:
                        continue
                    depth[h, y, x] = depth[h2, y, x]
                    sigma[h, y, x] = sigma[h2, y, x]
                    cost[h, y, x] = cost[h2, y, x]
                    depth[h2, y, x] = 0.
    return depth, sigma, cost


def holes(depth):
    """pixels and planes below MIN_DEPTH with a filled plane above them: what regularize moves"""
    filled = depth >= MIN_DEPTH
    above = np.flip(np.cumsum(np.flip(filled, 0), 0), 0) - filled   # filled planes strictly above
    return int(((~filled) & (above > 0)).sum())


def pack_mh(cam, prm, depth, sigma):
    """DepthMap::reconstruct(ALL_HYPOTHESES | SIGMA_VALUE): (indices int32 [m], hyp int32 [m], cloud [m][3], sigma [m]); prm
    holds scale, u0, v0"""
    H, Y, X = depth.shape
    idx, hyp, cloud, sig = [], [], [], []
    for y in range(Y):
        for x in range(X):
            if not depth[0, y, x] >= MIN_DEPTH:
                continue
            P = sr.reconstruct(cam, float(x * prm["scale"] + prm["u0"]), float(y * prm["scale"] + prm["v0"]))
            for h in range(H):
                d = depth[h, y, x]
                if not d >= MIN_DEPTH:
                    continue
                idx.append(y * X + x)
                hyp.append(h)
                sig.append(sigma[h, y, x])
                if P is None:
                    cloud.append((0., 0., 0.))
                else:
                    nrm = math.sqrt(sr.dot3(P, P))
                    cloud.append(tuple(P[i] / nrm * d for i in range(3)))
    return (np.array(idx, np.int32), np.array(hyp, np.int32), np.array(cloud, np.float64).reshape(-1, 3),
            np.array(sig, np.float64))
