// vg_sparse_odom.hpp -- kernels of the sparse visual odometry (section 13 of the C ABI): the reference's
// SparseOdometry::feedData (src/localization/sparse_odom.cpp:240-437) from the image to the pose increment.
//
//   harrisCorners   :161-203   integer Harris response (three launches: gradients, row sums, column sums + response),
//                              strict 3 x 3 maxima into a candidate list, top-k by radix selection in ONE workgroup per image
//   descriptors     :205-238   written by the selection kernel, feature by feature in the final order
//   BFMatcher       :266-300   distance matrix (FP64 sums of float differences, patch order), nearest neighbours of both
//                              sides, cross-check + threshold compacted in the order of the first index
//   computeTransfSparse :440-469   one wave per problem, the whole trust-region LM inside the launch
//   ransacNPoints scoring :552-580 one lane per hypothesis x match
//
// All arithmetic is FP64 or integer; every floating-point sum has a fixed order (the only atomics are integer counters).
#pragma once

#include <cstdint>

#include "vg_lm6.hpp"
#include "vg_local.hpp"
#include "vg_motion_prior.hpp"
#include "vg_image_device.hpp"

namespace vgso {

using vgs::reflect101;

constexpr int kThreads = 256;
constexpr int kSelectThreads = 1024;
constexpr int kMaxFeatures = 1024;   // the selection kernel holds the chosen keys in LDS
constexpr int kPatch = 4, kDesc = (2 * kPatch + 1) * (2 * kPatch + 1);   // DESC_SIZE = 4: 9 x 9
constexpr int kBorder = 7;           // harrisCorners' loop bounds; the handle refuses a side below 2 kBorder + 1 = 15
constexpr int kBox = 3;              // blockSize 7; an overhang of at most kBox < 15, so reflect101's clamp never acts
constexpr int kTile = 16;            // distance matrix tile

// Sobel 3 x 3 (scale 1) with BORDER_REFLECT_101: dx in the low, dy in the high half of one int32 (|.| <= 1020)
__global__ __launch_bounds__(kThreads) void gradient_kernel(const uint8_t *__restrict__ img, int w, int h, int32_t *__restrict__ grad)
{
    const int64_t P = (int64_t)w * h, p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    const uint8_t *im = img + blockIdx.y * P;
    const int v = (int)(p / w), u = (int)(p - (int64_t)v * w);
    const int um = reflect101(u - 1, w), up = reflect101(u + 1, w), vm = reflect101(v - 1, h), vp = reflect101(v + 1, h);
    const int a = im[(int64_t)vm * w + um], b = im[(int64_t)vm * w + u], c = im[(int64_t)vm * w + up];
    const int d = im[(int64_t)v * w + um], f = im[(int64_t)v * w + up];
    const int g = im[(int64_t)vp * w + um], hh = im[(int64_t)vp * w + u], i = im[(int64_t)vp * w + up];
    const int dx = (c + 2 * f + i) - (a + 2 * d + g), dy = (g + 2 * hh + i) - (a + 2 * b + c);
    grad[blockIdx.y * P + p] = (int32_t)(((uint32_t)dy << 16) | ((uint32_t)dx & 0xffffu));
}

// sums of dx^2, dx dy, dy^2 over the seven columns around a pixel (each <= 7 * 1020^2: int32): planes [3][n * P]
__global__ __launch_bounds__(kThreads) void row_sum_kernel(const int32_t *__restrict__ grad, int w, int h, int64_t plane, int32_t *__restrict__ sums)
{
    const int64_t P = (int64_t)w * h, p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    const int v = (int)(p / w), u = (int)(p - (int64_t)v * w);
    const int32_t *row = grad + blockIdx.y * P + (int64_t)v * w;
    int a = 0, b = 0, c = 0;
#pragma unroll
    for (int du = -kBox; du <= kBox; du++) {
        const int32_t g = row[reflect101(u + du, w)];
        const int dx = (int16_t)(g & 0xffff), dy = g >> 16;
        a += dx * dx;
        b += dx * dy;
        c += dy * dy;
    }
    const int64_t o = blockIdx.y * P + p;
    sums[o] = a;
    sums[plane + o] = b;
    sums[2 * plane + o] = c;
}

// the seven rows summed in int64 and R = 20 (a c - b^2) - (a + c)^2
__global__ __launch_bounds__(kThreads) void response_kernel(const int32_t *__restrict__ sums, int w, int h, int64_t plane, int64_t *__restrict__ resp)
{
    const int64_t P = (int64_t)w * h, p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    const int v = (int)(p / w), u = (int)(p - (int64_t)v * w);
    const int32_t *s = sums + blockIdx.y * P + u;
    int64_t a = 0, b = 0, c = 0;
#pragma unroll
    for (int dv = -kBox; dv <= kBox; dv++) {
        const int64_t o = (int64_t)reflect101(v + dv, h) * w;
        a += s[o];
        b += s[plane + o];
        c += s[2 * plane + o];
    }
    resp[blockIdx.y * P + p] = 20 * (a * c - b * b) - (a + c) * (a + c);
}

// strict maxima of the 3 x 3 neighbourhood inside the 7-pixel border, appended to the image's candidate list (the order of
// the list does not matter: the selection orders by value)
__global__ __launch_bounds__(kThreads) void maxima_kernel(const int64_t *__restrict__ resp, int w, int h, int64_t cap, int64_t *__restrict__ cand_r,
                                                          int32_t *__restrict__ cand_i, unsigned int *__restrict__ cand_n)
{
    const int iw = w - 2 * kBorder, ih = h - 2 * kBorder;
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= (int64_t)iw * ih) return;
    const int v = (int)(q / iw) + kBorder, u = (int)(q % iw) + kBorder;
    const int64_t *r = resp + (int64_t)blockIdx.y * w * h;
    const int64_t val = r[(int64_t)v * w + u];
    bool is_max = true;
#pragma unroll
    for (int dv = -1; dv <= 1; dv++)
#pragma unroll
        for (int du = -1; du <= 1; du++)
            if ((du || dv) && val <= r[(int64_t)(v + dv) * w + (u + du)]) is_max = false;
    if (!is_max) return;
    const unsigned int slot = atomicAdd(cand_n + blockIdx.y, 1u);
    if (slot < cap) {
        cand_r[blockIdx.y * cap + slot] = val;
        cand_i[blockIdx.y * cap + slot] = v * w + u;
    }
}

struct SelectArgs {
    const uint8_t *img;         // [n][h][w]
    const int64_t *cand_r;      // [n][cap]
    const int32_t *cand_i;
    const unsigned int *cand_n; // [n]
    const double *weights;      // [81]
    int32_t *keypoints;         // [n][max_features][2]
    float *descriptors;         // [n][max_features][81]
    int32_t *count;             // [n]
    int64_t cap;
    int w, h, max_features;
};

// The max_features largest candidates of an image under the total order (R, raster index), both descending, by a radix
// selection of twelve 8-bit digits (eight of the biased response, four of the index): every pass streams the candidate
// list from memory, so the list may be of any length; only the chosen max_features keys live in LDS, where they are
// ranked by counting.  Then the key points and the descriptors in that order.  One workgroup per image.
__global__ __launch_bounds__(kSelectThreads) void select_kernel(SelectArgs a)
{
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long s_hi[kMaxFeatures];
    __shared__ unsigned int s_lo[kMaxFeatures], s_ord[kMaxFeatures];
    __shared__ unsigned long long sh_hi;
    __shared__ unsigned int sh_lo, sh_rem, sh_n;
    const int tid = threadIdx.x, img = blockIdx.x;
    const unsigned int found = a.cand_n[img];
    const int64_t M = found < (unsigned long long)a.cap ? found : a.cap;
    const int k = M < a.max_features ? (int)M : a.max_features;
    const int64_t *cr = a.cand_r + img * a.cap;
    const int32_t *ci = a.cand_i + img * a.cap;
    const unsigned long long bias = 1ull << 63;
    unsigned long long phi = 0;
    unsigned int plo = 0, rem = (unsigned)k;
    const bool all = M <= a.max_features;
    if (!all) {
        for (int d = 0; d < 12; d++) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int64_t c = tid; c < M; c += kSelectThreads) {
                const unsigned long long hi = (unsigned long long)cr[c] + bias;
                const unsigned int lo = (unsigned)ci[c];
                bool match;
                unsigned int digit;
                if (d < 8) {
                    match = d == 0 || (hi >> (64 - 8 * d)) == (phi >> (64 - 8 * d));
                    digit = (unsigned)(hi >> (56 - 8 * d)) & 255u;
                } else {
                    const int sh = 32 - 8 * (d - 8);
                    match = hi == phi && (d == 8 || (lo >> sh) == (plo >> sh));
                    digit = (lo >> (sh - 8)) & 255u;
                }
                if (match) atomicAdd(&hist[digit], 1u);
            }
            __syncthreads();
            if (tid < 256) {
                unsigned int above = 0;
                for (int D = 255; D > tid; D--) above += hist[D];
                if (above < rem && rem <= above + hist[tid]) {   // exactly one digit holds the rem-th largest key
                    sh_rem = rem - above;
                    if (d < 8) {
                        sh_hi = phi | ((unsigned long long)tid << (56 - 8 * d));
                        sh_lo = plo;
                    } else {
                        sh_hi = phi;
                        sh_lo = plo | ((unsigned)tid << (24 - 8 * (d - 8)));
                    }
                }
            }
            __syncthreads();
            phi = sh_hi;
            plo = sh_lo;
            rem = sh_rem;
            __syncthreads();
        }
    }
    if (tid == 0) sh_n = 0;
    __syncthreads();
    for (int64_t c = tid; c < M; c += kSelectThreads) {
        const unsigned long long hi = (unsigned long long)cr[c] + bias;
        const unsigned int lo = (unsigned)ci[c];
        if (all || hi > phi || (hi == phi && lo >= plo)) {
            const unsigned int slot = atomicAdd(&sh_n, 1u);
            if (slot < (unsigned)kMaxFeatures) {
                s_hi[slot] = hi;
                s_lo[slot] = lo;
            }
        }
    }
    __syncthreads();
    const int n_sel = sh_n < (unsigned)k ? (int)sh_n : k;   // == k: the order is total
    for (int t = tid; t < n_sel; t += kSelectThreads) {
        const unsigned long long hi = s_hi[t];
        const unsigned int lo = s_lo[t];
        int rank = 0;
        for (int j = 0; j < n_sel; j++) rank += (s_hi[j] > hi || (s_hi[j] == hi && s_lo[j] > lo)) ? 1 : 0;
        s_ord[rank] = lo;
    }
    __syncthreads();
    int32_t *kp = a.keypoints + (int64_t)img * a.max_features * 2;
    float *desc = a.descriptors + (int64_t)img * a.max_features * kDesc;
    for (int t = tid; t < a.max_features; t += kSelectThreads) {
        const int idx = t < n_sel ? (int)s_ord[t] : 0;
        kp[2 * t] = t < n_sel ? idx % a.w : 0;
        kp[2 * t + 1] = t < n_sel ? idx / a.w : 0;
    }
    const uint8_t *im = a.img + (int64_t)img * a.w * a.h;
    for (int e = tid; e < a.max_features * kDesc; e += kSelectThreads) {
        const int f = e / kDesc, j = e - f * kDesc;
        float out = 0.f;
        if (f < n_sel) {
            const int idx = (int)s_ord[f], u = idx % a.w + (j % 9 - kPatch), v = idx / a.w + (j / 9 - kPatch);
            out = (float)(a.weights[j] * (double)im[(int64_t)v * a.w + u]);
        }
        desc[e] = out;
    }
    if (tid == 0) a.count[img] = n_sel;
}

struct MatchArgs {
    const float *desc1, *desc2;      // [n][max_features][81]
    const int32_t *count1, *count2;  // [n]
    double *dist;                    // [n][max_features][max_features]
    double *dist_t;                  // the same transposed: both directions of nearest_kernel read along the lanes
    int32_t *nn1, *nn2;              // [n][max_features]
    int32_t *matches;                // [n][max_features][2]
    double *distance;                // [n][max_features]
    int32_t *match_count;            // [n]
    double threshold;
    int max_features;
};

// L1 distance of every descriptor pair: 16 x 16 tile, both sides staged in LDS, one FP64 accumulator per pair added in
// patch order
__global__ __launch_bounds__(kTile *kTile) void distance_kernel(MatchArgs a)
{
    __shared__ float s1[kTile][kDesc], s2[kTile][kDesc];
    const int pair = blockIdx.z, k1 = a.count1[pair], k2 = a.count2[pair];
    const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
    if (i0 >= k1 || j0 >= k2) return;
    const int tid = threadIdx.y * kTile + threadIdx.x;
    const float *d1 = a.desc1 + (int64_t)pair * a.max_features * kDesc, *d2 = a.desc2 + (int64_t)pair * a.max_features * kDesc;
    for (int e = tid; e < kTile * kDesc; e += kTile * kTile) {
        const int r = e / kDesc, c = e - r * kDesc;
        s1[r][c] = i0 + r < k1 ? d1[(int64_t)(i0 + r) * kDesc + c] : 0.f;
        s2[r][c] = j0 + r < k2 ? d2[(int64_t)(j0 + r) * kDesc + c] : 0.f;
    }
    __syncthreads();
    const int i = i0 + threadIdx.y, j = j0 + threadIdx.x;
    if (i >= k1 || j >= k2) return;
    double acc = 0.;
    for (int e = 0; e < kDesc; e++) acc += fabs((double)s1[threadIdx.y][e] - (double)s2[threadIdx.x][e]);
    a.dist[((int64_t)pair * a.max_features + i) * a.max_features + j] = acc;
    a.dist_t[((int64_t)pair * a.max_features + j) * a.max_features + i] = acc;
}

// blockIdx.y = 0: the nearest second-side descriptor of every first-side one; 1: the other direction.  Lowest index on ties.
__global__ __launch_bounds__(kThreads) void nearest_kernel(MatchArgs a)
{
    const int pair = blockIdx.z, k1 = a.count1[pair], k2 = a.count2[pair];
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const bool rows = blockIdx.y == 0;
    if (t >= (rows ? k1 : k2)) return;
    const int n = rows ? k2 : k1;
    // lane t walks column t of the matrix whose rows are the other side: consecutive lanes, consecutive doubles
    const double *p = (rows ? a.dist_t : a.dist) + (int64_t)pair * a.max_features * a.max_features + t;
    const int64_t stride = a.max_features;
    int best = -1;
    double bd = 0.;
    for (int o = 0; o < n; o++) {
        const double d = p[o * stride];
        if (best < 0 || d < bd) {
            best = o;
            bd = d;
        }
    }
    (rows ? a.nn1 : a.nn2)[(int64_t)pair * a.max_features + t] = best;
}

// cross-check and threshold, compacted in the order of the first index: one wave per pair
__global__ __launch_bounds__(64) void cross_check_kernel(MatchArgs a)
{
    const int pair = blockIdx.x, lane = threadIdx.x, k1 = a.count1[pair], k2 = a.count2[pair];
    const int64_t o = (int64_t)pair * a.max_features;
    const double *D = a.dist + o * a.max_features;
    int base = 0;
    for (int i0 = 0; i0 < k1 && k2 > 0; i0 += 64) {
        const int i = i0 + lane;
        bool keep = false;
        int j = 0;
        double d = 0.;
        if (i < k1) {
            j = a.nn1[o + i];
            d = D[(int64_t)i * a.max_features + j];
            keep = a.nn2[o + j] == i && !(d > a.threshold);
        }
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
        if (keep) {
            const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
            a.matches[2 * (o + pos)] = i;
            a.matches[2 * (o + pos) + 1] = j;
            a.distance[o + pos] = d;
        }
        base += __popcll(mask);
    }
    if (lane == 0) a.match_count[pair] = base;
}

// matched pixels lifted to rays (reconstructPointCloud; a pixel that does not reconstruct gives the zero vector), the second
// pixel as the observation, size 1
__global__ __launch_bounds__(kThreads) void rays_kernel(const double *__restrict__ cam, const int32_t *__restrict__ kp1, const int32_t *__restrict__ kp2,
                                                        const int32_t *__restrict__ matches, int m, double *__restrict__ x1, double *__restrict__ x2,
                                                        double *__restrict__ p2, double *__restrict__ size)
{
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= m) return;
    const int i = matches[2 * k], j = matches[2 * k + 1];
    const double u1 = kp1[2 * i], v1 = kp1[2 * i + 1], u2 = kp2[2 * j], v2 = kp2[2 * j + 1];
    double X[3];
    if (!vgs::eucm_reconstruct(cam, u1, v1, X)) X[0] = X[1] = X[2] = 0.;
    x1[3 * k] = X[0]; x1[3 * k + 1] = X[1]; x1[3 * k + 2] = X[2];
    if (!vgs::eucm_reconstruct(cam, u2, v2, X)) X[0] = X[1] = X[2] = 0.;
    x2[3 * k] = X[0]; x2[3 * k + 1] = X[1]; x2[3 * k + 2] = X[2];
    p2[2 * k] = u2;
    p2[2 * k + 1] = v2;
    size[k] = 1.;
}

// ---- computeTransfSparse -------------------------------------------------------------------------------------------
// what every problem of a call shares, uploaded once: [A (36) | J (36) | cam (6) | xiBaseCam (6) | base constants (28) | xiOdom (6)]
constexpr int kConstA = 0, kConstJ = 36, kConstCam = 72, kConstXb = 78, kConstBase = 84, kConstOdom = 84 + vg::kBaseConst;
constexpr int kConstDoubles = kConstOdom + 6;
constexpr int kSums = 28;        // J^T J (21, upper triangle row-major) | J^T r (6) | cost
constexpr int kSolveOut = 10;    // xi (6) | iterations | initial cost | final cost | termination
constexpr int kPartStride = kSums + 1;

struct SolveArgs {
    const double *consts;     // [kConstDoubles]
    const double *x1, *x2;    // [m][3]
    const double *p2;         // [m][2]
    const double *size;       // [m]
    const int32_t *index;     // [offsets[n_blocks]] the point of every block entry, or NULL: entry e is point e
    const int64_t *offsets;   // [n_blocks + 1]
    double *out;              // [n_blocks][kSolveOut]
    vglm6::Rule rule;         // the iteration cap and the trust-region constants
};

// One wave per problem: the block's frame by lane 0, the points strided over the lanes (residual pair and rows from
// vg_local.hpp's sparse_point_eval), the 28 sums of the lanes added in lane order, the prior added, and the damped 6 x 6
// Cholesky step with its acceptance (vg_lm6.hpp, the rule the photometric solve runs on the host) executed by every lane on the
// same numbers.  What a problem computes does not depend on the launch it is part of.
__global__ __launch_bounds__(64) void solve_kernel(SolveArgs a)
{
    using d2 = HIP_vector_type<double, 2>;
    __shared__ __attribute__((aligned(16))) double frame[vg::kSparseFrame];
    __shared__ double part[64 * kPartStride];
    __shared__ double Gs[2][kSums];
    const int lane = threadIdx.x;
    const int64_t first = a.offsets[blockIdx.x];
    const int cnt = (int)(a.offsets[blockIdx.x + 1] - first);
    const double *C = a.consts;

    auto evaluate = [&](const double(&xp)[6], double *G) {
        if (lane == 0) vg::sparse_frame_c(C + kConstXb, C + kConstBase, xp, frame);
        __syncthreads();
        double acc[kSums];
#pragma unroll
        for (int e = 0; e < kSums; e++) acc[e] = 0.;
        for (int k = lane; k < cnt; k += 64) {
            const int64_t pt = a.index ? (int64_t)a.index[first + k] : first + k;
            d2 r;
            vg::sparse_point_eval<vg::kEUCM>(
                C + kConstCam, frame, a.x1 + 3 * pt, a.x2 + 3 * pt,
                [&] {   // two loads: the caller's p2 need not be 16-byte aligned
                    d2 obs;
                    obs.x = a.p2[2 * pt];
                    obs.y = a.p2[2 * pt + 1];
                    return obs;
                },
                a.size + pt, true, [&](const d2 v) { r = v; },
                [&](const double(&rows)[12]) {
                    int q = 0;
#pragma unroll
                    for (int i = 0; i < 6; i++)
#pragma unroll
                        for (int j = i; j < 6; j++, q++) acc[q] += rows[i] * rows[j] + rows[6 + i] * rows[6 + j];
#pragma unroll
                    for (int i = 0; i < 6; i++) acc[21 + i] += rows[i] * r.x + rows[6 + i] * r.y;
                });
            acc[27] += r.x * r.x + r.y * r.y;
        }
#pragma unroll
        for (int e = 0; e < kSums; e++) part[lane * kPartStride + e] = acc[e];
        __syncthreads();
        if (lane < kSums) {
            double s = 0.;
            for (int l = 0; l < 64; l++) s += part[l * kPartStride + lane];
            G[lane] = lane == 27 ? 0.5 * s : s;
        }
        __syncthreads();
        if (lane == 0) {
            double d[6], Gl[kSums];
            for (int e = 0; e < kSums; e++) Gl[e] = G[e];
            vg::transf_inverse_compose(C + kConstOdom, xp, d);
            vgmp::accumulate(C + kConstA, C + kConstJ, d, Gl);
            for (int e = 0; e < kSums; e++) G[e] = Gl[e];
        }
        __syncthreads();
    };

    vglm6::State S;
#pragma unroll
    for (int k = 0; k < 6; k++) S.x[k] = C[kConstOdom + k];
    int cur = 0;
    evaluate(S.x, Gs[0]);
    vglm6::start(a.rule, S, Gs[0][27]);
    const double initial_cost = S.cost;
    while (!S.done) {
        vglm6::Step st;
        vglm6::step(a.rule, S, Gs[cur], st);
        double cost_c = 0.;
        if (st.ok) {   // the same decision in every lane
            evaluate(st.xc, Gs[1 - cur]);
            cost_c = Gs[1 - cur][27];
        }
        if (vglm6::accept(a.rule, S, st, cost_c)) cur = 1 - cur;
    }
    if (lane == 0) {
        double *o = a.out + (int64_t)blockIdx.x * kSolveOut;
        for (int k = 0; k < 6; k++) o[k] = S.x[k];
        o[6] = S.iterations;
        o[7] = initial_cost;
        o[8] = S.cost;
        o[9] = S.term;
    }
}

// ---- scoring -------------------------------------------------------------------------------------------------------
constexpr int kScoreFrame = 21;   // of the camera motion xi_c: t (3) | rotMat (9) | rotMatInv (9)

struct ScoreArgs {
    const double *frames;    // [n_hyp][kScoreFrame]
    const double *cam;       // [6]
    const double *x1, *x2;   // [..][3]
    const double *p2;        // [..][2]
    const int32_t *index;    // [m] or NULL
    double *residual;        // [n_hyp][m] or NULL
    int32_t *inliers;        // [n_hyp], zero at launch
    double threshold;
    int m;
};

// Triangulator(xi_c).computeRegular, the scaled ray moved by xi_c^-1, projection, pixel distance: one lane per hypothesis x
// match.  A point that does not project has the residual +inf.
__global__ __launch_bounds__(kThreads) void score_kernel(ScoreArgs a)
{
    const int k = blockIdx.x * kThreads + threadIdx.x, hyp = blockIdx.y;
    bool inlier = false;
    if (k < a.m) {
        const double *f = a.frames + (int64_t)hyp * kScoreFrame;
        const int64_t pt = a.index ? a.index[k] : k;
        const double *x1 = a.x1 + 3 * pt;
        const double lam = vg::triangulate_regular(f + 3, f, 1e-3, x1, a.x2 + 3 * pt, nullptr);
        const double d[3] = {x1[0] * lam - f[0], x1[1] * lam - f[1], x1[2] * lam - f[2]};
        double X[3];
        vg::mat3_vec(f + 12, d, X);
        vg::CornerEval<6> e;
        vg::eval_corner<vg::kEUCM, false, false>(a.cam, X[0], X[1], X[2], e);
        const double du = a.p2[2 * pt] - e.u, dv = a.p2[2 * pt + 1] - e.v;
        const double res = e.ok ? sqrt(du * du + dv * dv) : __builtin_inf();
        inlier = res < a.threshold;
        if (a.residual) a.residual[(int64_t)hyp * a.m + k] = res;
    }
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(inlier);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(a.inliers + hyp, __popcll(mask));
}

}  // namespace vgso
