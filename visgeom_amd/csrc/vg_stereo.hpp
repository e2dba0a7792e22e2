// vg_stereo.hpp -- dense fisheye stereo: the reference's EnhancedSgm (src/reconstruction/eucm_sgm.cpp), semi-global
// matching along the epipolar curves of two unrectified EUCM images.  The four kernels: per-pixel geometry, curve cost,
// directional aggregation (left+right, top+bottom with the winner) and depth, on the shared pieces of vg_stereo_device.hpp
// (among them the descriptor and its matching, which motion stereo runs too).  The multi-hypothesis call runs the column
// kernel's MH instantiation, which selects the K best local minima where it would take the winner, and the depth kernel over
// the hypothesis planes.
// The entries are in vg_stereo_tu.hip.
#pragma once

#include "vg_stereo_device.hpp"

namespace vgs {

// ---------------------------------------------------------------------------------------------------------------------
// kernels

// computeReconstructed / computeRotated / computePinf and the curve index + epipole choice: one lane per depth pixel
__global__ __launch_bounds__(256) void stereo_geometry_kernel(StereoGeom g, GeomEntry *out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t P = (int64_t)g.x_max * g.y_max;
    if (i >= P) return;
    const int x = (int)(i % g.x_max), y = (int)(i / g.x_max);
    const int u = x * g.scale + g.u0, v = y * g.scale + g.v0;
    GeomEntry e = {0, 0, 0, 0, 0, 0, 0, 0};
    double X[3], Xr[3], pinf[2];
    if (eucm_reconstruct(g.c1, (double)u, (double)v, X)) {
        e.status = kGeomMask;
        e.index = curve_index(g, X);
        e.flags1 = choose_epipole(g, 0, u, v);
        mat_vec(g.Rinv, X, Xr);
        if (eucm_project(g.c2, Xr, pinf)) {
            e.status |= kGeomPinf;
            e.pinf_u = round_int(pinf[0]);
            e.pinf_v = round_int(pinf[1]);
            e.flags2 = choose_epipole(g, 1, e.pinf_u, e.pinf_v);
        }
    }
    out[i] = e;
}

// the unit-step walk of camera 2 for the uv cache: state k is kDisparityMargin unsteps back from pinf, then k steps
// (k < 0: further unsteps -- DESIGN.md section 9, deviation 3).  Positions outside the image read as (-1, -1).
struct CacheWalk {
    Raster r;
    int k;
    VGS_HD void start(const StereoGeom &g, const GeomEntry &e)
    {
        make_raster(g, 1, e.pinf_u, e.pinf_v, e.index, e.flags2, r);
        r.steps(-kDisparityMargin);
        k = 0;
    }
    VGS_HD void go(int k_to)
    {
        r.steps(k_to - k);   // only ever forward after the first call with k_to < 0
        k = k_to;
    }
};

struct CurveCostArgs {
    const uint8_t *img1, *img2;    // [n][v_max][u_max]
    const GeomEntry *geom;         // [P]
    uint8_t *err;                  // [n][P][disp_max]
    uint8_t *step, *salient, *skip;   // [n][P]
    int64_t n_pairs;
};

// writes the skipPixel pattern (eucm_sgm.cpp:220-226)
__device__ __forceinline__ void skip_pixel(uint8_t *e, int D, uint8_t *skip)
{
    e[0] = 0;
    for (int d = 1; d < D; d++) e[d] = 255;
    *skip = 1;
}

// computeCurveCost (eucm_sgm.cpp:228-393) with EpipolarDescriptor::compute, compareDescriptor and fillGaps: one lane per
// (pair, depth pixel).  The descriptor, its thresholds and the DP are vg_stereo_device.hpp's; here are the sample walk of
// camera 2 (uv-cache walk or stepped rasteriser), skipPixel where it leaves the image, and the error volume with fillGaps.
__global__ __launch_bounds__(kMatchLanes) void stereo_curve_cost_kernel(StereoGeom g, CurveCostArgs a)
{
    __shared__ MatchLds lds;
    const int lane = threadIdx.x;
    const int64_t P = (int64_t)g.x_max * g.y_max;
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= P * a.n_pairs) return;
    const int64_t pair = gi / P, pix = gi % P;
    const int D = g.disp_max, L = g.desc_length, H = L / 2, f = g.flaw_cost;
    uint8_t *e = a.err + gi * D;
    uint8_t *skipp = a.skip + gi;
    a.step[gi] = 0;
    a.salient[gi] = 0;
    *skipp = 0;
    const GeomEntry ge = a.geom[pix];
    if (!(ge.status & kGeomMask) || !(ge.status & kGeomPinf) || (ge.flags1 & kEpipoleTooClose)) {
        skip_pixel(e, D, skipp);
        return;
    }
    const int x = (int)(pix % g.x_max), y = (int)(pix / g.x_max);
    const uint8_t *im1 = a.img1 + pair * (int64_t)g.u_max * g.v_max;
    const uint8_t *im2 = a.img2 + pair * (int64_t)g.u_max * g.v_max;

    Raster ref;
    make_raster(g, 0, x * g.scale + g.u0, y * g.scale + g.v0, ge.index, ge.flags1, ref);
    int resp;
    const int step = compute_descriptor(g, ref, im1, lds, lane, resp);
    if (step < 1) {
        skip_pixel(e, D, skipp);
        return;
    }
    a.step[gi] = (uint8_t)step;
    if (g.salient_points_only && step < 2 && abs(resp) > g.desc_resp_thresh * L) a.salient[gi] = 1;
    descriptor_thresholds(lds, L, lane);

    // the sample walk of camera 2
    const int nSteps = (D + step - 1) / step;
    const int N = nSteps + L - 1;
    CacheWalk cw;
    Raster r2;
    if (g.use_uv_cache) {
        cw.start(g, ge);
        cw.go(kDisparityMargin - H * step);
    } else {
        make_raster(g, 1, ge.pinf_u, ge.pinf_v, ge.index, ge.flags2, r2);
        r2.eps *= step;
        r2.steps(-H);
    }

    MatchDp dp;
    dp.init();
    int prev = 0;
    const int t_end = nSteps + 3 * H;   // column j = t - 2H is final at time t; j runs to H + nSteps - 1
    for (int t = 0; t < t_end; t++) {
        if (t < N) {
            int su, sv;
            if (g.use_uv_cache) {
                if (t > 0) cw.go(cw.k + step);
                su = cw.r.u;
                sv = cw.r.v;
            } else {
                if (t > 0) r2.step();
                su = r2.u;
                sv = r2.v;
            }
            if (!inside(g, su, sv)) {
                skip_pixel(e, D, skipp);
                return;
            }
            dp.push(lds, lane, H, f, t, im2[(int64_t)sv * g.u_max + su]);
        }
        int total;
        if (dp.advance(lds, lane, L, f, t, N, total)) {
            const int d = t - 3 * H;   // column H + d
            const int val = imin(total, 255);
            if (step == 1) {
                e[d] = (uint8_t)val;
            } else {
                const int base = d * step;
                e[base] = (uint8_t)val;
                if (d > 0)   // fillGaps (eucm_sgm.cpp:407-448), case 3 as (2 a + b) / 3, (a + 2 b) / 3
                    for (int i = step - 1; i > 0; i--) e[base - i] = (uint8_t)((prev * i + val * (step - i)) / step);
                if (d == nSteps - 1)
                    for (int q = base + 1; q < D; q++) e[q] = (uint8_t)val;
            }
            prev = val;
        }
    }
}

// the per-pixel jump cost of the dynamic programming (_costBuffer; a pixel whose descriptor step was never set: jump_cost)
__device__ __forceinline__ int jump_of(const StereoGeom &g, int step)
{
    if (!g.image_based_cost || step == 0) return g.jump_cost;
    const int k = step == 1 ? 1 : (step == 2 ? 3 : 6);
    return (uint8_t)(g.jump_cost * k);   // _costBuffer is 8-bit
}

constexpr int kAggLanes = 64;        // one wave per scanline
constexpr int kAggPer = 4;           // disparities per lane (disp_max <= 256)

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = imin(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

struct AggArgs {
    const uint8_t *err;          // [n][P][D]
    const uint8_t *step, *salient, *skip;   // [n][P]
    int *sum;                    // [n][P][D]  L + R (+ T + B when write_total)
    int32_t *disparity;          // [n][P]
    int64_t n_pairs;
    int write_total;             // the aggregation stage entry: store L + R + T + B
};

// computeDynamicStep (eucm_sgm.cpp:450-476) for one wave: c[] holds inCost of this lane's disparities and becomes outCost
__device__ __forceinline__ void dyn_step(int *c, const uint8_t *err, int D, int lambda, int jump, int *lds)
{
    const int lane = threadIdx.x;
    int m = kInf;
#pragma unroll
    for (int q = 0; q < kAggPer; q++) {
        const int d = lane + q * kAggLanes;
        if (d < D) {
            m = imin(m, c[q]);
            lds[d] = c[q];
        }
    }
    const int best = wave_min(m);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kAggPer; q++) {
        const int d = lane + q * kAggLanes;
        if (d < D) {
            int val = c[q];
            if (d + 1 < D) val = imin(val, lds[d + 1] + lambda);
            if (d > 0) val = imin(val, lds[d - 1] + lambda);
            val = imin(val, best + jump);
            c[q] = val + err[d];
        }
    }
    __syncthreads();
}

// left then right tableaux of one row (computeDynamicProgramming, eucm_sgm.cpp:513-543): sum = L + R
__global__ __launch_bounds__(kAggLanes) void stereo_agg_rows_kernel(StereoGeom g, AggArgs a)
{
    __shared__ int lds[256];
    const int64_t row = blockIdx.x;   // pair * y_max + y
    const int X = g.x_max, D = g.disp_max, lane = threadIdx.x;
    const int64_t p0 = row * X;
    for (int pass = 0; pass < 2; pass++) {
        int c[kAggPer];
        const int x0 = pass == 0 ? 0 : X - 1, dx = pass == 0 ? 1 : -1;
        const uint8_t *er = a.err + (p0 + x0) * D;
        int *sr = a.sum + (p0 + x0) * D;
#pragma unroll
        for (int q = 0; q < kAggPer; q++) {
            const int d = lane + q * kAggLanes;
            if (d < D) {
                c[q] = er[d];
                sr[d] = pass == 0 ? c[q] : sr[d] + c[q];
            }
        }
        for (int i = 1; i < X; i++) {
            const int64_t p = p0 + x0 + (int64_t)dx * i;
            const int jump = jump_of(g, a.step[p]);
            dyn_step(c, a.err + p * D, D, g.step_cost, jump, lds);
            int *s = a.sum + p * D;
#pragma unroll
            for (int q = 0; q < kAggPer; q++) {
                const int d = lane + q * kAggLanes;
                if (d < D) s[d] = pass == 0 ? c[q] : s[d] + c[q];
            }
        }
    }
}

constexpr int kMaxHyp = 8;           // hypotheses per pixel of the multi-hypothesis winner

// what the multi-hypothesis winner adds to AggArgs: hyp_max in [2, kMaxHyp], maxHypDiff, and the two outputs
struct MhArgs {
    int hyp_max, hypo_difference;
    int32_t *disparity, *final_cost;   // [n][hyp_max][P]; final_cost may be NULL
};

// the lowest set bit above position 64 q + b of the 256-bit mask m, -1 if none (q is a constant after unrolling)
__device__ __forceinline__ int next_bit(const unsigned long long *m, int q, int b)
{
    const unsigned long long hi = b == 63 ? 0ull : m[q] & (~0ull << (b + 1));
    if (hi) return q * 64 + __ffsll((long long)hi) - 1;
    for (int w = q + 1; w < kAggPer; w++)
        if (m[w]) return w * 64 + __ffsll((long long)m[w]) - 1;
    return -1;
}

// the highest set bit below position 64 q + b, -1 if none
__device__ __forceinline__ int prev_bit(const unsigned long long *m, int q, int b)
{
    const unsigned long long lo = m[q] & ((1ull << b) - 1ull);
    if (lo) return q * 64 + 63 - __clzll((long long)lo);
    for (int w = q - 1; w >= 0; w--)
        if (m[w]) return w * 64 + 63 - __clzll((long long)m[w]);
    return -1;
}

// reconstructDisparityMH (eucm_sgm.cpp:628-738) for one pixel, by the wave that holds its whole aggregated cost: cost[q] =
// total - 2 err of this lane's disparities, valid[q] = err <= error_max.  A valid disparity is a candidate when its cost is
// below its next valid neighbour's and not above its previous one's; it reports the disparity in front of that next neighbour.
// hyp_max rounds each take the cheapest candidate (then the lowest disparity) that is dearer than the round before, or as dear
// at another disparity, and from the second round on within hypo_difference of it.  lds is free between two dyn_steps; the
// two barriers here keep it so.  Every lane of the wave calls this; lane 0 writes.
__device__ __forceinline__ void select_hypotheses(const int *cost, const bool *valid, bool off, const MhArgs &m, int64_t out, int64_t P, int *lds)
{
    const int lane = threadIdx.x;
    unsigned long long mask[kAggPer], cand[kAggPer];
#pragma unroll
    for (int q = 0; q < kAggPer; q++) {
        mask[q] = __ballot(valid[q]);
        if (valid[q]) lds[lane + q * kAggLanes] = cost[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kAggPer; q++) {
        cand[q] = ~0ull;
        if (valid[q]) {
            const int nx = next_bit(mask, q, lane), pv = prev_bit(mask, q, lane);
            if (nx >= 0 && cost[q] < lds[nx] && (pv < 0 || cost[q] <= lds[pv]))
                cand[q] = (unsigned long long)(unsigned)cost[q] << 32 | (unsigned)(nx - 1);
        }
    }
    __syncthreads();
    long long min_cost = 0;
    int min_disp = -1, h = 0;
    for (; h < m.hyp_max && !off; h++) {
        unsigned long long key = ~0ull;
#pragma unroll
        for (int q = 0; q < kAggPer; q++) {
            const long long c = (long long)(cand[q] >> 32);
            const int r = (int)(cand[q] & 0xffffffffu);
            const bool ok = cand[q] != ~0ull && (c > min_cost || (c == min_cost && r != min_disp)) && (h == 0 || c <= min_cost + m.hypo_difference);
            if (ok && cand[q] < key) key = cand[q];
        }
        key = wave_min_u64(key);
        if (key == ~0ull) break;
        min_cost = (long long)(key >> 32);
        min_disp = (int)(key & 0xffffffffu);
        if (lane == 0) {
            m.disparity[out + h * P] = min_disp;
            if (m.final_cost) m.final_cost[out + h * P] = (int32_t)min_cost;
        }
    }
    if (lane == 0)
        for (; h < m.hyp_max; h++) {
            m.disparity[out + h * P] = -1;
            if (m.final_cost) m.final_cost[out + h * P] = INT32_MAX;
        }
}

// top then bottom tableaux of one column (eucm_sgm.cpp:544-576) added to sum; the bottom pass has the whole sum of every
// pixel it reaches and picks the winner there (reconstructDisparity, eucm_sgm.cpp:580-626; MH: the hyp_max winners of
// reconstructDisparityMH, to m's planes instead of a.disparity)
template <bool MH>
__global__ __launch_bounds__(kAggLanes) void stereo_agg_cols_kernel(StereoGeom g, AggArgs a, MhArgs m)
{
    __shared__ int lds[256];
    const int64_t colid = blockIdx.x;   // pair * x_max + x
    const int X = g.x_max, Y = g.y_max, D = g.disp_max, lane = threadIdx.x;
    const int64_t pair = colid / X;
    const int x = (int)(colid % X);
    const int64_t P = (int64_t)X * Y;
    for (int pass = 0; pass < 2; pass++) {
        int c[kAggPer];
        for (int i = 0; i < Y; i++) {
            const int y = pass == 0 ? i : Y - 1 - i;
            const int64_t p = pair * P + (int64_t)y * X + x;
            const uint8_t *er = a.err + p * D;
            if (i == 0) {
#pragma unroll
                for (int q = 0; q < kAggPer; q++) {
                    const int d = lane + q * kAggLanes;
                    if (d < D) c[q] = er[d];
                }
            } else {
                dyn_step(c, er, D, g.step_cost, jump_of(g, a.step[p]), lds);
            }
            int *s = a.sum + p * D;
            if (pass == 0) {
#pragma unroll
                for (int q = 0; q < kAggPer; q++) {
                    const int d = lane + q * kAggLanes;
                    if (d < D) s[d] += c[q];
                }
                continue;
            }
            if (MH) {
                int cost[kAggPer];
                bool valid[kAggPer];
#pragma unroll
                for (int q = 0; q < kAggPer; q++) {
                    const int d = lane + q * kAggLanes;
                    cost[q] = 0;
                    valid[q] = false;
                    if (d < D) {
                        const int ev = er[d];
                        cost[q] = s[d] + c[q] - 2 * ev;
                        valid[q] = ev <= g.error_max;
                    }
                }
                // the skip buffer is not consulted (eucm_sgm.cpp:643)
                select_hypotheses(cost, valid, g.salient_points_only && a.salient[p] == 0, m, pair * m.hyp_max * P + (int64_t)y * X + x, P, lds);
                continue;
            }
            unsigned long long key = ~0ull;
#pragma unroll
            for (int q = 0; q < kAggPer; q++) {
                const int d = lane + q * kAggLanes;
                if (d < D) {
                    const int tot = s[d] + c[q];
                    if (a.write_total) s[d] = tot;
                    const int ev = er[d];
                    if (d >= 1 && ev <= g.error_max) {
                        const unsigned long long k = (unsigned long long)(unsigned)(tot - 2 * ev) << 32 | (unsigned)d;
                        key = k < key ? k : key;
                    }
                }
            }
            key = wave_min_u64(key);
            if (lane == 0) {
                const bool off = (g.salient_points_only && a.salient[p] == 0) || a.skip[p];
                a.disparity[p] = (off || key == ~0ull) ? -1 : (int)(key & 0xffffffffu);
            }
        }
    }
}

struct DepthArgs {
    const GeomEntry *geom;
    const uint8_t *err, *step, *salient, *skip;
    const int32_t *disparity;
    double *depth, *sigma, *cost;    // [n][P]
    int64_t n_pairs;
};

// one pixel of reconstructDepth (eucm_sgm.cpp:186-213) with the six-argument triangulate (eucm_stereo.cpp:250-296): the
// range and its sigma at disparity `disp` (-1 is walked like any other), left as they are where the triangulation fails
__device__ __forceinline__ void depth_at(const StereoGeom &g, const GeomEntry &ge, int64_t pix, int disp, int step, double &dep, double &sig)
{
    const int x = (int)(pix % g.x_max), y = (int)(pix / g.x_max);
    int u21, v21, u22, v22;
    if (g.use_uv_cache) {
        CacheWalk cw;
        cw.start(g, ge);
        cw.go(kDisparityMargin + disp);
        const bool in1 = inside(g, cw.r.u, cw.r.v);
        u21 = in1 ? cw.r.u : -1;
        v21 = in1 ? cw.r.v : -1;
        cw.go(cw.k + step);
        const bool in2 = inside(g, cw.r.u, cw.r.v);
        u22 = in2 ? cw.r.u : -1;
        v22 = in2 ? cw.r.v : -1;
    } else {
        Raster r;
        make_raster(g, 1, ge.pinf_u, ge.pinf_v, ge.index, ge.flags2, r);
        r.steps(disp);
        u21 = r.u;
        v21 = r.v;
        r.steps(step);
        u22 = r.u;
        v22 = r.v;
    }
    const int gu = x * g.scale + g.u0, gv = y * g.scale + g.v0;
    double l1, s1;
    if (triangulate_pairs(g, gu, gv, gu, gv, u21, v21, u22, v22, l1, s1) && l1 < kTriangulateDistMax) {
        sig = s1;
        dep = l1;
    }
}

// reconstructDepth (eucm_sgm.cpp:154-218): one lane per pixel
__global__ __launch_bounds__(256) void stereo_depth_kernel(StereoGeom g, DepthArgs a)
{
    const int64_t P = (int64_t)g.x_max * g.y_max;
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= P * a.n_pairs) return;
    const int64_t pix = gi % P;
    double dep = 0., sig = 0., cst = 0.;
    const GeomEntry ge = a.geom[pix];
    if (!((g.salient_points_only && !a.salient[gi]) || a.skip[gi]) && (ge.status & kGeomMask)) {
        cst = (double)a.err[gi * g.disp_max];
        depth_at(g, ge, pix, a.disparity[gi], a.step[gi], dep, sig);
    }
    if (a.depth) a.depth[gi] = dep;
    if (a.sigma) a.sigma[gi] = sig;
    if (a.cost) a.cost[gi] = cst;
}

// reconstructDepth over the hypothesis planes: one lane per (pair, plane, pixel); a.disparity and the outputs are
// [n][hyp_max][P], and the cost of plane h is the matching error at index h (eucm_sgm.cpp:174), not at the plane's disparity
__global__ __launch_bounds__(256) void stereo_depth_mh_kernel(StereoGeom g, DepthArgs a, int hyp_max)
{
    const int64_t P = (int64_t)g.x_max * g.y_max;
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= P * hyp_max * a.n_pairs) return;
    const int64_t pix = gi % P, pair = gi / (P * hyp_max);
    const int h = (int)(gi / P % hyp_max);
    const int64_t pi = pair * P + pix;
    double dep = 0., sig = 0., cst = 0.;
    const GeomEntry ge = a.geom[pix];
    if (!((g.salient_points_only && !a.salient[pi]) || a.skip[pi]) && (ge.status & kGeomMask)) {
        cst = (double)a.err[pi * g.disp_max + h];
        depth_at(g, ge, pix, a.disparity[gi], a.step[pi], dep, sig);
    }
    if (a.depth) a.depth[gi] = dep;
    if (a.sigma) a.sigma[gi] = sig;
    if (a.cost) a.cost[gi] = cst;
}

}  // namespace vgs
