// vg_dense_ba.hpp -- photometric bundle adjustment: the poses of F further frames and the depth of every selected key-frame
// cell, refined together on the grey difference (the reference's dense_ba_test, test/reconstruction/dense_ba_test.cpp:38-113,
// with a gradient selection, a depth prior and a grey sigma added: DESIGN.md section 5.21).  Per residual a 6-parameter pose
// block and a 1-parameter depth block, so the depth block of the normal equations is diagonal and is eliminated exactly:
//   ba_select_kernel    the pack, in raster order of the depth grid (count / scan / place, no atomics)
//   ba_eval_kernel      one lane per (frame, point): residual, pose row, depth entry to row buffers, and the 28 sums per frame
//   ba_point_kernel     one lane per point: a = sum jd^2 + (lambda / sigma0)^2, g_d, the prior's cost
//   ba_schur_kernel     sum (w / e) [w | g_d]^T over the points, e = a + mu clamp(a): v_mfma_f64_16x16x4_f64 contracts 4
//                       points per instruction; a wave owns a contiguous run of points and keeps its tiles in registers
//   ba_schur_final_kernel  the waves' tiles in wave order, then S = H_pp + mu D_p - sum, rhs = g_p - sum
//   ba_backsub_kernel   the candidate depths from the pose step, and the depth block's share of the trust-region rule's sums
// Every sum has one order: wave butterflies, then the workgroups' (waves') partials in index order, as contiguous runs whose
// sums are added in run order (run_sum64).  No floating-point atomics.
#pragma once

#include "vg_bicubic.hpp"
#include "vg_compact.hpp"
#include "vg_photometric_row.hpp"

namespace vgba {

using namespace vgs;

constexpr int kLanes = 256, kWaves = kLanes / 64;
constexpr int kMaxFrames = 8;      // kSums (vg_photometric_row.hpp) sums per frame
constexpr int kTail = 5;           // sum D dx^2 | g . dx | |dx|^2 | |x|^2 | max |g| of the depth block
constexpr int kSchurBlocks = 128;  // at most this many workgroups reduce; beyond 128 x 256 points a wave's run grows

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- the pack --------------------------------------------------------------------------------------------------------

struct SelectArgs {
    const float *img;             // the key frame, full size
    int w, h;
    double cam[6];
    Grid g;
    const double *depth, *sigma;  // [y_max][x_max]; sigma may be NULL
    double grad_thresh;
    int need_sigma;               // the prior is on: a cell needs a finite sigma > 0
    unsigned *block_counts;
    const unsigned *block_offsets;
    int32_t *idx;
    double *val, *dir, *d0, *s0;
};

VGS_HD bool select_cell(const SelectArgs &a, int64_t cell, double &value, double *dir, double &d, double &s)
{
    const int x = (int)(cell % a.g.x_max), y = (int)(cell / a.g.x_max);
    d = a.depth[cell];
    s = a.sigma ? a.sigma[cell] : 0.;
    if (!(isfinite(d) && d >= kMinDepth)) return false;
    const int u = x * a.g.scale + a.g.u0, v = y * a.g.scale + a.g.v0;   // uConv, vConv
    if (u < 0 || u >= a.w || v < 0 || v >= a.h) return false;
    double Xr[3];
    if (!eucm_reconstruct(a.cam, (double)u, (double)v, Xr)) return false;
    float fgu, fgv;
    sobel8_at(a.img, a.w, a.h, u, v, fgu, fgv);   // the gradient of photo_sobel_kernel, at the cell's pixel only
    const double gu = fgu, gv = fgv;
    if (gu * gu + gv * gv < a.grad_thresh) return false;
    if (a.need_sigma && !(isfinite(s) && s > 0.)) return false;
    value = a.img[(int64_t)v * a.w + u];
    const double nrm = sqrt(dot3(Xr, Xr));
    for (int i = 0; i < 3; i++) dir[i] = Xr[i] / nrm;
    return true;
}

// pass 1 (WRITE = false): the survivors of every block of 256 cells; pass 2: their raster-ordered places from the scanned
// block counts (vgc::block_place)
template <bool WRITE>
__global__ __launch_bounds__(kLanes) void ba_select_kernel(SelectArgs a)
{
    const int64_t cell = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    double value = 0., dir[3] = {0., 0., 0.}, d = 0., s = 0.;
    const bool keep = cell < (int64_t)a.g.x_max * a.g.y_max && select_cell(a, cell, value, dir, d, s);
    const unsigned pos = vgc::block_place<WRITE, kLanes>(keep, blockIdx.x, a.block_counts, a.block_offsets);
    if (!WRITE || !keep) return;
    a.idx[pos] = (int32_t)cell;
    a.val[pos] = value;
    for (int i = 0; i < 3; i++) a.dir[3 * (int64_t)pos + i] = dir[i];
    a.d0[pos] = d;
    a.s0[pos] = s;
}

// ---- evaluate --------------------------------------------------------------------------------------------------------

// what one frame brings: xiCam = xi o xi_base_cam (rotMatInv, trans), M = R(xiCam)^T R(xi_base_cam) for the depth entry and
// CameraJacobian(camera, xi, xi_base_cam)'s L11 | L12 | L22
struct Frame {
    double Rinv[9], t[3], M[9], L11[9], L12[9], L22[9];
};

struct EvalArgs {
    const Frame *frames;        // DEVICE [F]
    const float *imgs;          // [F][h][w]
    int w, h;
    double cam[6], Rb[9], tb[3], sigma_grey;
    const double *val, *dir, *depth;   // the pack and the depths the rows are taken at
    int m, blocks;
    double *res, *jp, *jd;      // [F][m], [F][m][6], [F][m]
    double *partials;           // [F][blocks][kSums]
};

// r, the pose row and the depth entry of point i in one frame.  A point that does not project, or whose coordinates exceed
// +-2^24 px, has a zero residual and zero rows.
VGS_HD void eval_point(const EvalArgs &a, const Frame &fr, int frame, int64_t i, double &r, double *row, double &jd)
{
    r = 0.;
    jd = 0.;
    for (int k = 0; k < 6; k++) row[k] = 0.;
    const double d = a.depth[i];
    double Xc[3], Xb[3], Xd[3], X[3];
    for (int k = 0; k < 3; k++) Xc[k] = d * a.dir[3 * i + k];
    mat_vec(a.Rb, Xc, Xb);
    for (int k = 0; k < 3; k++) Xd[k] = (Xb[k] + a.tb[k]) - fr.t[k];
    mat_vec(fr.Rinv, Xd, X);
    vg::CornerEval<6> e;
    vg::eval_corner<vg::kEUCM, true, false>(a.cam, X[0], X[1], X[2], e);
    const double pt[2] = {e.u, e.v};
    if (!(e.ok && coord_ok(pt))) return;
    double f, dfdr, dfdc;
    bicubic(a.imgs + (int64_t)frame * a.w * a.h, a.w, a.h, pt[1], pt[0], f, dfdr, dfdc);
    r = (f - a.val[i]) / a.sigma_grey;
    double dv[3], Md[3];
    dfdxi_row(X, e.P, dfdc, dfdr, fr.L11, fr.L12, fr.L22, dv, row);   // grad = (d/du, d/dv)
    for (int k = 0; k < 6; k++) row[k] = row[k] / a.sigma_grey;       // on the finished sums
    mat_vec(fr.M, a.dir + 3 * i, Md);
    jd = dot3(dv, Md) / a.sigma_grey;
}

// one lane per (frame, point): blockIdx.y the frame, blockIdx.x * 256 + threadIdx.x the point
__global__ __launch_bounds__(kLanes) void ba_eval_kernel(EvalArgs a)
{
    const int frame = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    double r = 0., row[6] = {0., 0., 0., 0., 0., 0.}, jd = 0.;
    if (i < a.m) {
        eval_point(a, a.frames[frame], frame, i, r, row, jd);
        const int64_t o = (int64_t)frame * a.m + i;
        a.res[o] = r;
        a.jd[o] = jd;
#pragma unroll
        for (int k = 0; k < 6; k++) a.jp[o * 6 + k] = row[k];
    }
    double s[kSums];
    row_products(row, r, s);
    block_sums<kSums, kLanes>(s, a.partials + ((int64_t)frame * a.blocks + blockIdx.x) * kSums);
}

struct PointArgs {
    int F, m, blocks;
    double lambda;
    const double *res, *jd, *depth, *d0, *s0;
    double *a, *gd;
    double *prior_partials;   // [blocks]
};

// lambda / sigma0 of a point; 0 without a prior
VGS_HD double prior_scale(double lambda, double s0) { return lambda > 0. ? lambda / s0 : 0.; }

// one lane per point: the diagonal entry and the gradient of its depth over the frames in order, and 1/2 p^2
__global__ __launch_bounds__(kLanes) void ba_point_kernel(PointArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    double c[1] = {0.};
    if (i < a.m) {
        double aa = 0., g = 0.;
        for (int f = 0; f < a.F; f++) {
            const double jd = a.jd[(int64_t)f * a.m + i];
            aa += jd * jd;
            g += jd * a.res[(int64_t)f * a.m + i];
        }
        const double ps = prior_scale(a.lambda, a.s0[i]);
        const double p = ps * (a.depth[i] - a.d0[i]);
        a.a[i] = aa + ps * ps;
        a.gd[i] = g + ps * p;
        c[0] = 0.5 * (p * p);
    }
    block_sums<1, kLanes>(c, a.prior_partials + blockIdx.x);
}

// The second pass of every sum here, by one wave: the n values p[i stride] in index order, split into 64 contiguous runs -- lane
// t adds run t in order, lane 0 adds the 64 run sums in order (the association of vg_compact.hpp's scan).  A chain of n / 64 + 64
// additions instead of n; the order depends on n alone.  MAX: the maximum instead.  The result is lane 0's.
template <bool MAX>
__device__ __forceinline__ double run_sum64(const double *p, int64_t stride, int n, double *lds)
{
    const int t = threadIdx.x & 63, chunk = (n + 63) / 64;
    const int lo = min(t * chunk, n), hi = min(lo + chunk, n);
    double s = 0.;
    for (int i = lo; i < hi; i++) s = MAX ? fmax(s, p[i * stride]) : s + p[i * stride];
    lds[t] = s;
    __syncthreads();
    double r = 0.;
    if (t == 0)
        for (int k = 0; k < 64; k++) r = MAX ? fmax(r, lds[k]) : r + lds[k];
    return r;
}

// workgroup 28 f + k: sum k of frame f over the workgroups of ba_eval_kernel; workgroup 28 F: the prior's cost
__global__ __launch_bounds__(64) void ba_sums_kernel(const double *partials, const double *prior_partials, int F, int blocks, double *sums)
{
    __shared__ double lds[64];
    const int f = blockIdx.x / kSums, k = blockIdx.x % kSums;
    const double s = f < F ? run_sum64<false>(partials + (int64_t)f * blocks * kSums + k, kSums, blocks, lds) : run_sum64<false>(prior_partials, 1, blocks, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// ---- reduce(mu) ------------------------------------------------------------------------------------------------------

VGS_HD double clamp_diag(double a, double dmin, double dmax) { return a < dmin ? dmin : (a > dmax ? dmax : a); }

struct SchurArgs {
    int F, K, m, run;            // run: points of a wave, a multiple of 4
    double mu, dmin, dmax;
    const double *jp, *jd, *a, *gd;
    double *tiles;               // [waves][tile][4][64]
    int waves;
    const double *sums;          // [F][kSums] | prior cost
    double *S, *rhs;             // [K][K], [K]
};

// D(16x16) += A(16x4) * B(4x16); lane l supplies A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15];
// lane l, register r holds D[row = (l>>4) + 4r][col = l&15]
__device__ __forceinline__ f64x4 mfma_f64_16x16x4(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// tiles (ti, tj >= ti) of the K x (K + 1) matrix [sum (w / e) w^T | sum (w / e) g_d], numbered row by row
VGS_HD constexpr int tile_count(int TA, int TB)
{
    int n = 0;
    for (int ti = 0; ti < TA; ti++) n += TB - ti;
    return n;
}
VGS_HD int tile_index(int ti, int tj, int TB)
{
    int n = 0;
    for (int t = 0; t < ti; t++) n += TB - t;
    return n + (tj - ti);
}

// A wave walks its run of points four at a time: lane l holds point (l >> 4) of the four and the elements (l & 15) + 16 t of
// its w = (J_pose[f] jd[f])_f; A = w / e, B = [w | g_d].  TA = ceil(K / 16) row tiles, TB = ceil((K + 1) / 16) column tiles.
template <int TA, int TB>
__global__ __launch_bounds__(kLanes) void ba_schur_kernel(SchurArgs a)
{
    const int lane = threadIdx.x & 63, wave = blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int q = lane & 15, sub = lane >> 4;
    const int64_t first = (int64_t)wave * a.run, last = min(first + (int64_t)a.run, (int64_t)a.m);
    f64x4 acc[TA][TB];
#pragma unroll
    for (int ti = 0; ti < TA; ti++)
#pragma unroll
        for (int tj = 0; tj < TB; tj++) acc[ti][tj] = f64x4{0., 0., 0., 0.};
    int fr[TB], col[TB];   // the frame and the pose column of element q + 16 t; frame F: the g_d column; frame -1: padding
#pragma unroll
    for (int t = 0; t < TB; t++) {
        const int e = q + 16 * t;
        fr[t] = e < a.K ? e / 6 : (e == a.K ? a.F : -1);
        col[t] = e % 6;
    }
    // kGroups groups of four points in flight: a wave runs alone on its SIMD, so the loads of the later groups hide the latency
    // of the first's; the groups enter the accumulators in order, and one past the run's end adds zeros
    // Every load is unconditional, at an index clamped into the arrays (a dead lane reads point m - 1, a padding element
    // frame 0), and what it brought is dropped by a select: no branch stands between the loads of a round.
    constexpr int kGroups = 4;
    int fc[TB];
#pragma unroll
    for (int t = 0; t < TB; t++) fc[t] = fr[t] < 0 ? 0 : (fr[t] >= a.F ? a.F - 1 : fr[t]);
    for (int64_t base = first; base < last; base += 4 * kGroups) {
        double vB[kGroups][TB], vA[kGroups][TA];
#pragma unroll
        for (int u = 0; u < kGroups; u++) {
            const int64_t p = base + 4 * u + sub;
            const bool live = p < last;
            const int64_t pc = live ? p : (int64_t)a.m - 1;
            const double aa = a.a[pc], g = a.gd[pc];
            const double e_p = aa + a.mu * clamp_diag(aa, a.dmin, a.dmax);
#pragma unroll
            for (int t = 0; t < TB; t++) {
                const int64_t o = (int64_t)fc[t] * a.m + pc;
                const double w = a.jp[o * 6 + col[t]] * a.jd[o];
                const bool pose = live && fr[t] >= 0 && fr[t] < a.F;
                vB[u][t] = pose ? w : (live && fr[t] == a.F ? g : 0.);
                if (t < TA) vA[u][t] = pose ? w / e_p : 0.;
            }
        }
#pragma unroll
        for (int u = 0; u < kGroups; u++)
#pragma unroll
            for (int ti = 0; ti < TA; ti++)
#pragma unroll
                for (int tj = ti; tj < TB; tj++) acc[ti][tj] = mfma_f64_16x16x4(vA[u][ti], vB[u][tj], acc[ti][tj]);
    }
    constexpr int NT = tile_count(TA, TB);
    double *out = a.tiles + (int64_t)wave * NT * 256;
#pragma unroll
    for (int ti = 0; ti < TA; ti++)
#pragma unroll
        for (int tj = ti; tj < TB; tj++) {
            const int n = tile_index(ti, tj, TB);
#pragma unroll
            for (int r = 0; r < 4; r++) out[(n * 4 + r) * 64 + lane] = acc[ti][tj][r];
        }
}

// workgroup i, thread (j, c): entry (i, j >= i) of the K x (K + 1) matrix over the waves in index order, split into 8 contiguous
// runs -- thread (j, c) adds run c in order, thread (j, 0) the 8 run sums in order; then S and rhs
constexpr int kFinalRuns = 8;
__global__ __launch_bounds__(64 * kFinalRuns) void ba_schur_final_kernel(SchurArgs a, int TB, int NT)
{
    __shared__ double runs[kFinalRuns][64];
    const int i = blockIdx.x, j = threadIdx.x, c = threadIdx.y;
    const bool entry = j >= i && j <= a.K;
    const int ti = i / 16, tj = (entry ? j : i) / 16, ri = i % 16, cj = j % 16;
    const int n = tile_index(ti, tj, TB);
    const int64_t o = (int64_t)(n * 4 + ri / 4) * 64 + (ri % 4) * 16 + cj;
    const int chunk = (a.waves + kFinalRuns - 1) / kFinalRuns, lo = min(c * chunk, a.waves), hi = min(lo + chunk, a.waves);
    double u = 0.;
    for (int w = lo; entry && w < hi; w++) u += a.tiles[(int64_t)w * NT * 256 + o];
    runs[c][j] = u;
    __syncthreads();
    if (!entry || c != 0) return;
    u = 0.;
    for (int k = 0; k < kFinalRuns; k++) u += runs[k][j];
    const int fi = i / 6, ci = i % 6;
    const double *G = a.sums + (int64_t)fi * kSums;
    if (j == a.K) {
        a.rhs[i] = G[21 + ci] - u;
        return;
    }
    double h = 0.;
    if (j / 6 == fi) {
        const int cj6 = j % 6;
        h = G[ci * 6 - ci * (ci - 1) / 2 + (cj6 - ci)];   // row ci of the upper triangle starts at 6 ci - ci (ci - 1) / 2
    }
    if (i == j) h += a.mu * clamp_diag(h, a.dmin, a.dmax);
    const double s = h - u;
    a.S[i * a.K + j] = s;
    a.S[j * a.K + i] = s;
}

// ---- back-substitution -----------------------------------------------------------------------------------------------

struct BacksubArgs {
    int F, m, blocks;
    double mu, dmin, dmax;
    double dp[6 * kMaxFrames];
    const double *jp, *jd, *a, *gd, *depth;
    double *cand;        // [m] the candidate depths
    double *partials;    // [blocks][kTail]
};

__global__ __launch_bounds__(kLanes) void ba_backsub_kernel(BacksubArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    double s[kTail] = {0., 0., 0., 0., 0.};
    if (i < a.m) {
        double wdp = 0.;
        for (int f = 0; f < a.F; f++) {
            const int64_t o = (int64_t)f * a.m + i;
            double t = 0.;
#pragma unroll
            for (int c = 0; c < 6; c++) t += a.jp[o * 6 + c] * a.dp[6 * f + c];
            wdp += a.jd[o] * t;
        }
        const double aa = a.a[i], D = clamp_diag(aa, a.dmin, a.dmax), g = a.gd[i], d = a.depth[i];
        const double dd = -(g + wdp) / (aa + a.mu * D);
        a.cand[i] = d + dd;
        s[0] = D * dd * dd;
        s[1] = g * dd;
        s[2] = dd * dd;
        s[3] = d * d;
        s[4] = fabs(g);
    }
    block_sums<kTail, kLanes, 4>(s, a.partials + (int64_t)blockIdx.x * kTail);   // slot 4 is the maximum
}

// workgroup k: entry k of the tail over the workgroups of ba_backsub_kernel
__global__ __launch_bounds__(64) void ba_tail_kernel(const double *partials, int blocks, double *tail)
{
    __shared__ double lds[64];
    const int k = blockIdx.x;
    const double s = k == 4 ? run_sum64<true>(partials + k, kTail, blocks, lds) : run_sum64<false>(partials + k, kTail, blocks, lds);
    if (threadIdx.x == 0) tail[k] = s;
}

// ---- the maps --------------------------------------------------------------------------------------------------------

// the pack's cells of the output maps: the depths, and 1 / sqrt(a)
__global__ __launch_bounds__(kLanes) void ba_scatter_kernel(const int32_t *idx, const double *depth, const double *a, int m, double *depth_map, double *sigma_map)
{
    const int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= m) return;
    if (depth_map) depth_map[idx[i]] = depth[i];
    if (sigma_map) sigma_map[idx[i]] = 1. / sqrt(a[i]);
}

}  // namespace vgba
