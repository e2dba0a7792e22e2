// vg_corners.hpp -- checkerboard corner detection (the reference's CornerDetector, include/calibration/corner_detector.h,
// src/calibration/corner_detector.cpp): the pixel and per-candidate stages as HIP kernels for gfx950.  The graph stages are
// host C++ (vg_corners_graph.hpp); the entries and the orchestration are in vg_corners_tu.hip.
//
// Stages of one detection pass at one sigma (detectPattern .cpp:223-260), every image of the pass in the same launch:
//   1. vg_corner_response_kernel  computeResponse (.cpp:262-330): both Gaussian blurs, the sharp gradient, |grad|, the saddle
//                                 response and per-tile partial sums of the kept responses (one pass over a tile in LDS)
//   2. vg_corner_mean_kernel      _avgVal: the tile partials of an image summed in a fixed order
//   3. vg_corner_maxima_kernel    selectCandidates' local maxima (.cpp:494-521), compacted per image as sortable keys
//   4. vg_corner_select_kernel    the top M keys of an image, sorted (radix select + bitonic sort in LDS); for M = Nx Ny it
//                                 also gives VAL_THRESH (.cpp:525-537)
//   5. vg_corner_check_kernel     checkCorner (.cpp:331-442) and scaleInvarient (.cpp:444-492), one lane per candidate above
//                                 VAL_THRESH; the accepted ones are compacted again, then stage 4 keeps the first 10 Nx Ny
//   6. vg_corner_transitions_kernel  getTransitions (.cpp:1135-1259) of every kept candidate (constructGraph's seeds and
//                                 initPoin's lines) and its gradient threshold (.cpp:627-634)
//   7. vg_corner_refine_kernel    improveCorners / SubpixelCorner (.cpp:162-198, :31-103): one lane per detected corner
//
// Deterministic throughout: no float atomics; the integer atomics that compact candidates only decide where a key lands, and
// every compacted list is sorted by its key before it is used.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "vg_image_device.hpp"

namespace vg {

constexpr int kCornerTileW = 64, kCornerTileH = 16;     // output tile of the stencil kernels: 256 lanes x 4 rows
constexpr int kCornerHalo = 3;                           // ceil(sigma_2) + 1 for sigma_2 <= 2
constexpr int kCornerMaxSigmaRadius = 2;                 // ceil(sigma_2) of the sigmas {1.4, 2, 1}
constexpr int kCornerMinDim = 16, kCornerMaxDim = 16384; // image sides; pixel offsets inside one image < 2^28
constexpr int kCircMaxR = 5;                             // checkCorner reaches radius 2 INIT_RADIUS - 1 = 5 (INIT_RADIUS <= 3)
constexpr int kCircMaxLen = 32, kCircTableLen = 128;     // the radius-5 circle has 28 points; all five fit in 128
constexpr int kSelectMax = 4096;                         // the sorted lists of stage 4: 10 Nx Ny <= 4000
constexpr int kSelectThreads = 1024;

// getCircle (.cpp:1079-1108) of every radius 1..5 around (0, 0): the rasterised circles are translation invariant for integer
// centres, so a kernel adds the centre and clamps (normalizePoint) -- built once on the host (vg_corners_graph.hpp)
struct CircleTable {
    int8_t du[kCircTableLen], dv[kCircTableLen];
    int start[kCircMaxR + 1], len[kCircMaxR + 1];
};

// cv::getGaussianKernel weights (double, normalised) rounded to float; w2 has 2 r2 + 1 taps
struct BlurWeights {
    float w1[3];
    float w2[2 * kCornerMaxSigmaRadius + 1];
    int r2;
};

using vgs::reflect101;   // BORDER_REFLECT_101 for |overhang| < n, then clamped

__device__ __forceinline__ float round_u8(float v) { return fminf(fmaxf(rintf(v), 0.f), 255.f); }

struct ResponseArgs {
    const uint8_t *images;     // caller's batch [n][H][W]
    const int64_t *list;       // image of every slot
    int W, H, tiles_x, tiles_per_image;
    BlurWeights bw;
    uint8_t *src1;             // [slots][H][W] or nullptr (the stage entry only)
    uint8_t *src2;             // [slots][H][W]
    float *gradx, *grady, *imgrad, *resp;   // [slots][H][W]
    double *part_sum;          // [slots][tiles_per_image]
    int *part_cnt;
};

// One workgroup: a 64 x 16 tile of one image.  The tile and a 3-pixel halo of the input go to LDS once; the row passes of both
// blurs, their column passes (rounded to u8) on the tile +- 1 and then the derivatives and the response of every tile pixel are
// computed from LDS.  Every output map is written once.  The blurs are float32 with the taps summed in order, no FMA
// contraction (-ffp-contract=off), rounded half to even -- the computation tests/corners_ref.py restates.
__global__ __launch_bounds__(256) void vg_corner_response_kernel(ResponseArgs a)
{
    constexpr int TW = kCornerTileW, TH = kCornerTileH, HA = kCornerHalo;
    constexpr int IW = TW + 2 * HA, IH = TH + 2 * HA;   // input rows / cols -3 .. T+2
    constexpr int EW = TW + 2, EH = TH + 2;             // blurred maps on rows / cols -1 .. T
    __shared__ float in[IH][IW + 1];
    __shared__ float h1[EH + 2][EW + 1];   // row pass of blur 1 on rows -2 .. T+1
    __shared__ float h2[IH][EW + 1];       // row pass of blur 2 on rows -3 .. T+2
    __shared__ float s1[EH][EW + 1], s2[EH][EW + 1];
    __shared__ double red_sum[256];
    __shared__ int red_cnt[256];
    const int slot = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    const int tx0 = (tile % a.tiles_x) * TW, ty0 = (tile / a.tiles_x) * TH;
    const int W = a.W, H = a.H;
    const size_t plane = (size_t)W * (size_t)H;
    const uint8_t *src = a.images + (size_t)a.list[slot] * plane;
    for (int k = t; k < IH * IW; k += 256) {
        const int r = k / IW, c = k % IW;
        const int y = reflect101(ty0 - HA + r, H), x = reflect101(tx0 - HA + c, W);
        in[r][c] = (float)src[(size_t)y * W + x];
    }
    __syncthreads();
    const BlurWeights &bw = a.bw;
    const int r2 = bw.r2;
    for (int k = t; k < (EH + 2) * EW; k += 256) {
        const int r = k / EW, c = k % EW;   // row ty0-2+r = in row r+1; col tx0-1+c = in col c+2
        float acc = bw.w1[0] * in[r + 1][c + 1];
        acc = acc + bw.w1[1] * in[r + 1][c + 2];
        acc = acc + bw.w1[2] * in[r + 1][c + 3];
        h1[r][c] = acc;
    }
    for (int k = t; k < IH * EW; k += 256) {
        const int r = k / EW, c = k % EW;
        float acc = bw.w2[0] * in[r][c + 2 - r2];
        for (int i = 1; i <= 2 * r2; i++) acc = acc + bw.w2[i] * in[r][c + 2 - r2 + i];
        h2[r][c] = acc;
    }
    __syncthreads();
    for (int k = t; k < EH * EW; k += 256) {
        const int r = k / EW, c = k % EW;   // row ty0-1+r = h1 row r+1 = h2 row r+2
        float acc = bw.w1[0] * h1[r][c];
        acc = acc + bw.w1[1] * h1[r + 1][c];
        acc = acc + bw.w1[2] * h1[r + 2][c];
        s1[r][c] = round_u8(acc);
        float acc2 = bw.w2[0] * h2[r + 2 - r2][c];
        for (int j = 1; j <= 2 * r2; j++) acc2 = acc2 + bw.w2[j] * h2[r + 2 - r2 + j][c];
        s2[r][c] = round_u8(acc2);
    }
    __syncthreads();
    const int col = t % TW, row0 = (t / TW) * 4;
    double sum = 0.;
    int cnt = 0;
    const size_t obase = (size_t)slot * plane;
    for (int q = 0; q < 4; q++) {
        const int row = row0 + q, x = tx0 + col, y = ty0 + row;
        if (x >= W || y >= H) continue;
        const int r = row + 1, c = col + 1;
        const size_t o = obase + (size_t)y * W + x;
        a.src2[o] = (uint8_t)s2[r][c];
        if (a.src1) a.src1[o] = (uint8_t)s1[r][c];
        float gxo = 0.f, gyo = 0.f, go = 0.f, ro = 0.f;
        if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2) {
            // .cpp:284-296: the sharp gradient (u8 differences are ints; 0.3 x int in double)
            const int d1x = (int)s1[r][c + 1] - (int)s1[r][c - 1], d2x = (int)s2[r][c + 1] - (int)s2[r][c - 1];
            const int d1y = (int)s1[r + 1][c] - (int)s1[r - 1][c], d2y = (int)s2[r + 1][c] - (int)s2[r - 1][c];
            const double gxS = ((double)d1x - 0.3 * (double)d2x) / 2.;
            const double gyS = ((double)d1y - 0.3 * (double)d2y) / 2.;
            gxo = (float)(gxS * 0.01);
            gyo = (float)(gyS * 0.01);
            go = (float)(sqrt(gxS * gxS + gyS * gyS) * 0.01);
            // .cpp:302-322: Hessian of the sigma_2 image; gx / gy are INTEGER divisions by 2 in the reference
            const int c0 = (int)s2[r][c];
            const double iuu = (double)((int)s2[r][c - 1] + (int)s2[r][c + 1] - 2 * c0);
            const double ivv = (double)((int)s2[r - 1][c] + (int)s2[r + 1][c] - 2 * c0);
            double iuv = (double)((int)s2[r - 1][c - 1] + (int)s2[r + 1][c + 1] - (int)s2[r + 1][c - 1] - (int)s2[r - 1][c + 1]);
            iuv /= 4;
            const double gx = (double)(d2x / 2), gy = (double)(d2y / 2);
            const double gsq = gx * gx + gy * gy;
            const double rv = -iuu * ivv + iuv * iuv - 0.001 * (gsq * gsq);
            if (rv > 0.01) {
                ro = (float)rv;
                sum += rv;
                cnt++;
            }
        }
        a.gradx[o] = gxo;
        a.grady[o] = gyo;
        a.imgrad[o] = go;
        a.resp[o] = ro;
    }
    red_sum[t] = sum;
    red_cnt[t] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            red_sum[t] += red_sum[t + s];
            red_cnt[t] += red_cnt[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        a.part_sum[(size_t)slot * a.tiles_per_image + tile] = red_sum[0];
        a.part_cnt[(size_t)slot * a.tiles_per_image + tile] = red_cnt[0];
    }
}

// _avgVal = acc / count of every slot: lane t sums tiles t, t + 256, ... in order, then a fixed tree (count 0 -> NaN, as 0. / 0)
__global__ __launch_bounds__(256) void vg_corner_mean_kernel(const double *part_sum, const int *part_cnt, int tiles_per_image,
                                                             double *avg)
{
    __shared__ double s[256];
    __shared__ long long n[256];
    const int slot = blockIdx.x, t = threadIdx.x;
    double acc = 0.;
    long long cnt = 0;
    for (int k = t; k < tiles_per_image; k += 256) {
        acc += part_sum[(size_t)slot * tiles_per_image + k];
        cnt += part_cnt[(size_t)slot * tiles_per_image + k];
    }
    s[t] = acc;
    n[t] = cnt;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) {
            s[t] += s[t + h];
            n[t] += n[t + h];
        }
        __syncthreads();
    }
    if (t == 0) avg[slot] = s[0] / (double)n[0];
}

// candidate key: the response's float bits above the complemented pixel index, so that a descending key order is the
// value order with ties broken by the smaller raster index (v W + u) first.  Kept responses are > 0.01: their bits order
// like their values.
__device__ __forceinline__ uint64_t corner_key(float val, int idx)
{
    return ((uint64_t)__float_as_uint(val) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)idx);
}
__device__ __forceinline__ float key_value(uint64_t k) { return __uint_as_float((uint32_t)(k >> 32)); }
__device__ __forceinline__ int key_index(uint64_t k) { return (int)(0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFu)); }

struct MaximaArgs {
    const float *resp;         // [slots][H][W]
    const double *avg;         // [slots]
    int W, H, tiles_x, radius;
    uint64_t *keys;            // [slots][cap]
    int *count;                // [slots]
    int64_t cap;
};

// selectCandidates' scan (.cpp:497-521): a pixel of [R, W-R) x [R, H-R) whose response is not below _avgVal and that beats
// every neighbour of the disc i^2 + j^2 <= R^2 + 1; an equal neighbour at i > 0, or i == 0 and j > 0, does not count (the
// reference's tie rule).  Two maxima never share a 2 x 2 block, so ceil(W/2) ceil(H/2) keys per image always suffice.
__global__ __launch_bounds__(256) void vg_corner_maxima_kernel(MaximaArgs a)
{
    constexpr int TW = kCornerTileW, TH = kCornerTileH, HA = kCornerHalo;
    constexpr int IW = TW + 2 * HA, IH = TH + 2 * HA;
    __shared__ float tileR[IH][IW + 1];
    const int slot = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    const int tx0 = (tile % a.tiles_x) * TW, ty0 = (tile / a.tiles_x) * TH;
    const int W = a.W, H = a.H, R = a.radius;
    const float *resp = a.resp + (size_t)slot * (size_t)W * (size_t)H;
    for (int k = t; k < IH * IW; k += 256) {
        const int r = k / IW, c = k % IW;
        const int y = ty0 - HA + r, x = tx0 - HA + c;
        tileR[r][c] = (x >= 0 && x < W && y >= 0 && y < H) ? resp[(size_t)y * W + x] : 0.f;
    }
    __syncthreads();
    const double avg = a.avg[slot];
    const int col = t % TW, row0 = (t / TW) * 4;
    for (int q = 0; q < 4; q++) {
        const int row = row0 + q, x = tx0 + col, y = ty0 + row;
        if (x < R || x >= W - R || y < R || y >= H - R) continue;
        const float val = tileR[row + HA][col + HA];
        if ((double)val < avg) continue;
        bool isMax = true;
        for (int j = -R; j <= R && isMax; j++)
            for (int i = -R; i <= R; i++) {
                if (i == 0 && j == 0) continue;
                if (i * i + j * j > R * R + 1) continue;
                const float nb = tileR[row + HA + j][col + HA + i];
                if (val <= nb) {
                    if (val == nb && (i > 0 || (i == 0 && j > 0))) continue;
                    isMax = false;
                    break;
                }
            }
        if (!isMax) continue;
        const int pos = atomicAdd(a.count + slot, 1);
        if (pos < a.cap) a.keys[(size_t)slot * a.cap + pos] = corner_key(val, y * W + x);
    }
}

struct SelectArgs {
    const uint64_t *keys;      // [slots][cap]
    const int *count;          // [slots]
    int64_t cap;
    int M;                     // how many of the largest keys to keep (<= kSelectMax)
    int ref_count;             // > 0: thresh[slot] = 0.05 sum of the values of the top keys / ref_count (VAL_THRESH)
    uint64_t *out;             // [slots][kSelectMax] sorted descending
    int *out_count;            // [slots]
    double *thresh;            // [slots] or nullptr
};

// The M largest keys of one image, sorted descending.  More than M: an MSB-first radix select (8 passes of 8 bits, LDS
// histograms) finds the M-th largest key -- keys are unique, so exactly M keys are >= it -- then they are gathered and sorted
// by a bitonic sort in LDS.
__global__ __launch_bounds__(kSelectThreads) void vg_corner_select_kernel(SelectArgs a)
{
    __shared__ uint64_t buf[kSelectMax];
    __shared__ int hist[256];
    __shared__ uint64_t s_prefix, s_mask;
    __shared__ int s_need, s_fill;
    const int slot = blockIdx.x, t = threadIdx.x;
    const uint64_t *keys = a.keys + (size_t)slot * a.cap;
    const int n = (int)min((int64_t)a.count[slot], a.cap);
    uint64_t lo = 0;   // keep keys >= lo
    if (n > a.M) {
        if (t == 0) {
            s_prefix = 0;
            s_mask = 0;
            s_need = a.M;
        }
        __syncthreads();
        for (int d = 7; d >= 0; d--) {
            for (int b = t; b < 256; b += kSelectThreads) hist[b] = 0;
            __syncthreads();
            const uint64_t prefix = s_prefix, mask = s_mask;
            for (int i = t; i < n; i += kSelectThreads) {
                const uint64_t k = keys[i];
                if ((k & mask) == prefix) atomicAdd(&hist[(int)((k >> (8 * d)) & 0xFF)], 1);
            }
            __syncthreads();
            if (t == 0) {
                int need = s_need, b = 255;
                for (; b > 0; b--) {
                    if (hist[b] >= need) break;
                    need -= hist[b];
                }
                s_need = need;
                s_prefix = prefix | ((uint64_t)b << (8 * d));
                s_mask = mask | ((uint64_t)0xFF << (8 * d));
            }
            __syncthreads();
        }
        lo = s_prefix;
    }
    const int m = min(n, a.M);
    int P = 1;
    while (P < m) P <<= 1;
    if (t == 0) s_fill = 0;
    for (int i = t; i < P; i += kSelectThreads) buf[i] = 0;
    __syncthreads();
    for (int i = t; i < n; i += kSelectThreads) {
        const uint64_t k = keys[i];
        if (k >= lo) buf[atomicAdd(&s_fill, 1)] = k;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = t; i < P; i += kSelectThreads) {
                const int j = i ^ stride;
                if (j > i) {
                    const bool desc = (i & size) == 0;
                    const uint64_t x = buf[i], y = buf[j];
                    if (desc ? (x < y) : (x > y)) {
                        buf[i] = y;
                        buf[j] = x;
                    }
                }
            }
            __syncthreads();
        }
    uint64_t *out = a.out + (size_t)slot * kSelectMax;
    for (int i = t; i < m; i += kSelectThreads) out[i] = buf[i];
    if (t == 0) {
        a.out_count[slot] = m;
        if (a.thresh) {   // .cpp:525-535: the top values summed in descending order, in double
            double acc = 0.;
            for (int i = 0; i < m; i++) acc += (double)key_value(buf[i]);
            a.thresh[slot] = 0.05 * acc / a.ref_count;
        }
    }
}

// ---- per-candidate checks: one lane per candidate, its circle samples in an LDS row of its own ----

constexpr int kCheckLanes = 64;

__device__ __forceinline__ void circle_transitions(const uint8_t *img, int W, int H, int u, int v, const CircleTable &ct, int radius,
                                                   int *tv, int &n)
{
    const int s0 = ct.start[radius];
    n = ct.len[radius];
    int smp[kCircMaxLen];
#pragma unroll
    for (int k = 0; k < kCircMaxLen; k++) {
        if (k < n) {
            const int x = min(max(u + ct.du[s0 + k], 0), W - 1), y = min(max(v + ct.dv[s0 + k], 0), H - 1);   // normalizePoint
            smp[k] = img[(size_t)y * W + x];
        }
    }
    // centralDifferences (.cpp:1122-1133)
    tv[0] = smp[1] - smp[n - 1];
    for (int k = 1; k < n - 1; k++) tv[k] = smp[k + 1] - smp[k - 1];
    tv[n - 1] = smp[0] - smp[n - 2];
}

__device__ __forceinline__ int arg_max(const int *tv, int b, int e)   // std::max_element: the first maximum; b == e -> b
{
    int best = b;
    for (int k = b + 1; k < e; k++)
        if (tv[k] > tv[best]) best = k;
    return best;
}
__device__ __forceinline__ int arg_min(const int *tv, int b, int e)
{
    int best = b;
    for (int k = b + 1; k < e; k++)
        if (tv[k] < tv[best]) best = k;
    return best;
}

// CornerDetector::setZero (corner_detector.h:150-167)
__device__ __forceinline__ void set_zero(int *tv, int n, int it)
{
    const int ref = tv[it];
    int d = it;
    do {
        tv[d] = 0;
        d++;
        if (d == n) d = 0;
    } while (tv[d] * ref > 0);
    int b = it;
    do {
        tv[b] = 0;
        if (b == 0) b = n;
        b--;
    } while (tv[b] * ref > 0);
}

// checkCorner (.cpp:331-442) with MAX_FAULTS = 0: every radius in [checkRadius, checkRadius + max(3, checkRadius)) must pass
__device__ bool check_corner(const uint8_t *img, int W, int H, int u, int v, int checkRadius, const CircleTable &ct, int *tv)
{
    const double ALPHA_1 = 0.3, ALPHA_2 = 0.5;
    const int RADIUS_MAX = checkRadius + max(3, checkRadius);
    for (int radius = checkRadius; radius < RADIUS_MAX; radius++) {
        int n;
        circle_transitions(img, W, H, u, v, ct, radius, tv, n);
        const int distThresh = n / 2 - 2, distThresh2 = n - distThresh;
        const int iMax = arg_max(tv, 0, n);
        const double transMax = tv[iMax];
        set_zero(tv, n, iMax);
        const int iMax2 = arg_max(tv, 0, n);
        if (tv[iMax2] < transMax * ALPHA_1) return false;
        const double transMax2 = tv[iMax2];
        set_zero(tv, n, iMax2);
        int dist = abs(iMax - iMax2);
        if (dist < distThresh || dist > distThresh2) return false;
        const int iMax3 = arg_max(tv, 0, n);
        if (tv[iMax3] > transMax2 * ALPHA_2) return false;
        set_zero(tv, n, iMax3);
        const int iMin = arg_min(tv, 0, n);
        const double transMin = tv[iMin];
        if (transMin > transMax * -ALPHA_1) return false;
        set_zero(tv, n, iMin);
        const int iMin2 = arg_min(tv, 0, n);
        if (tv[iMin2] > transMin * -ALPHA_1) return false;
        const double transMin2 = tv[iMin2];
        set_zero(tv, n, iMin2);
        dist = abs(iMin - iMin2);
        if (dist < distThresh || dist > distThresh2) return false;
        const int iMin3 = arg_min(tv, 0, n);
        if (tv[iMin3] < transMin2 * ALPHA_2) return false;
        set_zero(tv, n, iMin3);
    }
    return true;
}

// scaleInvarient (.cpp:444-492)
__device__ bool scale_invariant(const float *gradx, const float *grady, int W, int H, int u0, int v0, int R)
{
    for (int radius = R; radius < 2 * R; radius++) {
        double acc = 0., normAcc = 1e-10;
        for (int dv = -radius; dv <= radius; dv++)
            for (int du = -radius; du <= radius; du++) {
                const double sqNorm = du * du + dv * dv;
                if (sqNorm > radius * radius + 1 || sqNorm < 1) continue;
                const int u = u0 + du, v = v0 + dv;
                if (u < 0 || u >= W || v < 0 || v >= H) continue;
                const double gx = gradx[(size_t)v * W + u], gy = grady[(size_t)v * W + u];
                const double gradSqNorm = gx * gx + gy * gy;
                if (gradSqNorm < 1e-3) continue;
                const double p = gx * du + gy * dv;
                acc += p * p / sqNorm;
                normAcc += gradSqNorm;
            }
        if (acc / normAcc < 0.3) return true;
    }
    return false;
}

struct CheckArgs {
    const uint8_t *images;
    const int64_t *list;
    const float *gradx, *grady;   // [slots][H][W]
    int W, H, init_radius;
    const uint64_t *keys;         // [slots][cap] maxima
    const int *count;
    const double *thresh;         // VAL_THRESH per slot
    int64_t cap;
    CircleTable ct;
    uint64_t *acc_keys;           // [slots][cap] accepted
    int *acc_count;
};

// .cpp:540-600: a maximum above VAL_THRESH is kept when checkCorner passes at some radius 1..INIT_RADIUS and scaleInvarient
// passes.  Each check depends only on its own candidate, so all of them run side by side; stage 4 then restores the order.
__global__ __launch_bounds__(kCheckLanes) void vg_corner_check_kernel(CheckArgs a)
{
    __shared__ int tvs[kCheckLanes][kCircMaxLen + 1];
    const int slot = blockIdx.y;
    const int n = (int)min((int64_t)a.count[slot], a.cap);
    const size_t plane = (size_t)a.W * (size_t)a.H;
    const uint8_t *img = a.images + (size_t)a.list[slot] * plane;
    const double thresh = a.thresh[slot];
    int *tv = tvs[threadIdx.x];
    for (int i = blockIdx.x * kCheckLanes + threadIdx.x; i < n; i += gridDim.x * kCheckLanes) {
        const uint64_t k = a.keys[(size_t)slot * a.cap + i];
        if (!((double)key_value(k) > thresh)) continue;
        const int idx = key_index(k), u = idx % a.W, v = idx / a.W;
        bool checked = false;
        for (int radius = 1; radius <= a.init_radius && !checked; radius++) checked = check_corner(img, a.W, a.H, u, v, radius, a.ct, tv);
        if (!checked) continue;
        if (!scale_invariant(a.gradx + slot * plane, a.grady + slot * plane, a.W, a.H, u, v, a.init_radius)) continue;
        const int pos = atomicAdd(a.acc_count + slot, 1);
        a.acc_keys[(size_t)slot * a.cap + pos] = k;
    }
}

struct TransitionArgs {
    const uint8_t *images;
    const int64_t *list;
    const float *imgrad;          // [slots][H][W]
    int W, H, init_radius;
    const uint64_t *hyp;          // [slots][kSelectMax] sorted accepted keys
    const int *hyp_count;
    CircleTable ct;
    int *trans;                   // [slots][kSelectMax][9]: u, v, then 4 points (max1, max2, min1, min2) or count 0 -> u, v, -1...
    double *grad_thresh;          // [slots][kSelectMax]
};

// getTransitions (.cpp:1135-1259): the strongest rising / falling transitions on circles of radius 1..INIT_RADIUS+1 and the
// strongest ones on the opposite side; the seeds of constructGraph and the lines of initPoin.  Also _gradThresh (.cpp:627-634).
__global__ __launch_bounds__(kCheckLanes) void vg_corner_transitions_kernel(TransitionArgs a)
{
    __shared__ int tvs[kCheckLanes][kCircMaxLen + 1];
    const int slot = blockIdx.y;
    const int n_h = a.hyp_count[slot];
    const size_t plane = (size_t)a.W * (size_t)a.H;
    const uint8_t *img = a.images + (size_t)a.list[slot] * plane;
    int *tv = tvs[threadIdx.x];
    for (int h = blockIdx.x * kCheckLanes + threadIdx.x; h < n_h; h += gridDim.x * kCheckLanes) {
        const int idx = key_index(a.hyp[(size_t)slot * kSelectMax + h]), u = idx % a.W, v = idx / a.W;
        int res[8];
        bool detected = false, found = false;
        double bestMaxTransition = 0.;
        for (int radius = 1; radius <= a.init_radius + 1; radius++) {
            int n;
            circle_transitions(img, a.W, a.H, u, v, a.ct, radius, tv, n);
            const int maxIdx1 = arg_max(tv, 0, n);
            int sl1 = maxIdx1 + n / 4, sl2 = sl1 + n / 2, maxIdx2;
            if (sl1 < n && sl2 >= n) {
                sl2 %= n;
                const int i21 = arg_max(tv, sl1, n), i22 = arg_max(tv, 0, sl2);
                maxIdx2 = tv[i21] > tv[i22] ? i21 : i22;
            } else {
                sl1 %= n;
                sl2 %= n;
                maxIdx2 = arg_max(tv, sl1, sl2);
            }
            const int minIdx1 = arg_min(tv, 0, n);
            sl1 = minIdx1 + n / 4;
            sl2 = sl1 + n / 2;
            int minIdx2;
            if (sl1 < n && sl2 >= n) {
                sl2 %= n;
                const int i21 = arg_min(tv, sl1, n), i22 = arg_min(tv, 0, sl2);
                minIdx2 = tv[i21] < tv[i22] ? i21 : i22;
            } else {
                sl1 %= n;
                sl2 %= n;
                minIdx2 = arg_min(tv, sl1, sl2);
            }
            if (detected) {
                if (bestMaxTransition > 0.7 * tv[maxIdx1]) break;
                detected = false;
                found = false;
            }
            if (tv[maxIdx2] < 0.4 * tv[maxIdx1]) continue;
            if (tv[minIdx2] > 0.4 * tv[minIdx1]) continue;
            const int s0 = a.ct.start[radius];
            const int pick[4] = {maxIdx1, maxIdx2, minIdx1, minIdx2};
            for (int q = 0; q < 4; q++) {
                res[2 * q] = min(max(u + a.ct.du[s0 + pick[q]], 0), a.W - 1);
                res[2 * q + 1] = min(max(v + a.ct.dv[s0 + pick[q]], 0), a.H - 1);
            }
            bestMaxTransition = tv[maxIdx1];
            detected = true;
            found = true;
        }
        int *out = a.trans + ((size_t)slot * kSelectMax + h) * 9;
        out[0] = u;
        out[1] = v;
        out[2] = found ? 4 : 0;
        double gt = DBL_MAX;
        for (int q = 0; q < 4; q++) {
            out[3 + q] = found ? res[2 * q] | (res[2 * q + 1] << 16) : -1;
            if (found) gt = fmin((double)a.imgrad[slot * plane + (size_t)res[2 * q + 1] * a.W + res[2 * q]] / 2, gt);
        }
        out[7] = out[8] = 0;
        a.grad_thresh[(size_t)slot * kSelectMax + h] = gt;
    }
}

// ---- SubpixelCorner + the minimiser (improveCorners .cpp:162-198) ----

// ceres::CubicHermiteSpline: Catmull-Rom through p1, p2 with central-difference tangents
__device__ __forceinline__ void hermite(double p0, double p1, double p2, double p3, double x, double &f, double &dfdx)
{
    const double a = 0.5 * (-p0 + 3.0 * p1 - 3.0 * p2 + p3);
    const double b = 0.5 * (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3);
    const double c = 0.5 * (-p0 + p2);
    const double d = p1;
    f = d + x * (c + x * (b + x * a));
    dfdx = c + x * (2.0 * b + 3.0 * a * x);
}

// ceres::BiCubicInterpolator::Evaluate(r, c) over Grid2D (include/ceres.h:48-69: indices clamped into the image)
__device__ __forceinline__ void bicubic(const float *g, int W, int H, double r, double c, double &f, double &dfdr, double &dfdc)
{
    const double rf = floor(r), cf = floor(c);
    const int row = (int)fmin(fmax(rf, -4.), (double)H + 4.), col = (int)fmin(fmax(cf, -4.), (double)W + 4.);
    double fr[4], dc[4];
    for (int k = 0; k < 4; k++) {
        const int rr = min(max(row - 1 + k, 0), H - 1);
        double p[4];
        for (int q = 0; q < 4; q++) p[q] = (double)g[(size_t)rr * W + min(max(col - 1 + q, 0), W - 1)];
        hermite(p[0], p[1], p[2], p[3], c - cf, fr[k], dc[k]);
    }
    hermite(fr[0], fr[1], fr[2], fr[3], r - rf, f, dfdr);
    double unused;
    hermite(dc[0], dc[1], dc[2], dc[3], r - rf, dfdc, unused);
}

struct SubpixelProblem {
    const float *gu, *gv;
    int W, H;
    double pu, pv, stepLength;   // the prior (the integer corner) and length / steps
};

// SubpixelCorner::Evaluate (.cpp:48-103), steps = 7: parameters (u, v, theta_1, theta_2, h)
__device__ void subpixel_cost(const SubpixelProblem &P, const double *x, double &cost, double *grad)
{
    const double u = x[0], v = x[1];
    cost = 0.1 * ((P.pu - u) * (P.pu - u) + (P.pv - v) * (P.pv - v));
    grad[0] = 0.2 * (u - P.pu);
    grad[1] = 0.2 * (v - P.pv);
    grad[2] = grad[3] = grad[4] = 0.;
    const double h = x[4];
    for (int direction = 0; direction < 2; direction++) {
        const int thIdx = 2 + direction;
        const double s = sin(x[thIdx]), c = cos(x[thIdx]);
        const double flowDir = direction ? 1 : -1;
        for (int k = 0; k < 14; k++) {   // stepVec = -1 l, 1 l, -2 l, 2 l, ...
            const int i = k / 2 + 1;
            const double length = (k & 1) ? i * P.stepLength : -i * P.stepLength;
            const double eta = (length > 0 ? 1 : -1) * flowDir;
            const double ui = u + c * length - s * h * eta;
            const double vi = v + s * length + c * h * eta;
            double fu, fuu, fuv, fv, fvu, fvv;
            bicubic(P.gu, P.W, P.H, vi, ui, fu, fuv, fuu);
            bicubic(P.gv, P.W, P.H, vi, ui, fv, fvv, fvu);
            cost += eta * (fv * c - fu * s);
            const double dudth = -s * length - c * h * eta;
            const double dvdth = c * length - s * h * eta;
            grad[0] += eta * (fvu * c - fuu * s);
            grad[1] += eta * (fvv * c - fuv * s);
            grad[thIdx] += eta * ((fvv * dvdth + fvu * dudth) * c - (fuv * dvdth + fuu * dudth) * s - fu * c - fv * s);
            grad[4] += fvv * c * c + fuu * s * s - s * c * (fvu + fuv);
        }
    }
}

constexpr int kLbfgsRank = 5;

struct RefineArgs {
    const float *gradx, *grady;  // [slots][H][W]
    int W, H;
    int64_t n;                   // corners
    const int *slot;             // [n]
    const double *init;          // [n][5] initPoin
    const double *prior;         // [n][2]
    const double *radius;        // [n] radVec
    double *out;                 // [n][2]
};

__device__ __forceinline__ double dot5(const double *a, const double *b)
{
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4];
}
__device__ __forceinline__ double maxabs5(const double *a)
{
    return fmax(fmax(fmax(fabs(a[0]), fabs(a[1])), fmax(fabs(a[2]), fabs(a[3]))), fabs(a[4]));
}

// The minimiser: ceres::GradientProblemSolver's defaults restated as an equivalent: L-BFGS (rank 5, initial
// Hessian scaled by s.y / y.y), a strong-Wolfe line search (sufficient decrease 1e-4, curvature 0.9; bracketing by doubling, zoom
// by bisection, at most 20 evaluations each), at most 50 iterations; stops on |df| <= 1e-6 |f|, max|g| <= 1e-10 or
// |dx| <= 1e-8 (|x| + 1e-8).  FP64.
__global__ __launch_bounds__(64) void vg_corner_refine_kernel(RefineArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const size_t plane = (size_t)a.W * (size_t)a.H;
    SubpixelProblem P;
    P.gu = a.gradx + (size_t)a.slot[i] * plane;
    P.gv = a.grady + (size_t)a.slot[i] * plane;
    P.W = a.W;
    P.H = a.H;
    P.pu = a.prior[2 * i];
    P.pv = a.prior[2 * i + 1];
    P.stepLength = a.radius[i] / 7;
    double x[5], g[5], f;
    for (int k = 0; k < 5; k++) x[k] = a.init[5 * i + k];
    subpixel_cost(P, x, f, g);
    double S[kLbfgsRank][5], Y[kLbfgsRank][5], rho[kLbfgsRank];
    int m = 0;
    const double c1 = 1e-4, c2 = 0.9;
    for (int iter = 1; iter <= 50 && isfinite(f); iter++) {
        if (maxabs5(g) <= 1e-10) break;
        double d[5], q[5], al[kLbfgsRank];
        for (int k = 0; k < 5; k++) q[k] = g[k];
#pragma unroll
        for (int j = 0; j < kLbfgsRank; j++)   // newest pair first (slot 0)
            if (j < m) {
                al[j] = rho[j] * dot5(S[j], q);
                for (int k = 0; k < 5; k++) q[k] -= al[j] * Y[j][k];
            }
        const double gamma = m > 0 ? dot5(S[0], Y[0]) / dot5(Y[0], Y[0]) : 1.;
        for (int k = 0; k < 5; k++) q[k] *= gamma;
#pragma unroll
        for (int j = kLbfgsRank - 1; j >= 0; j--)
            if (j < m) {
                const double b = rho[j] * dot5(Y[j], q);
                for (int k = 0; k < 5; k++) q[k] += S[j][k] * (al[j] - b);
            }
        for (int k = 0; k < 5; k++) d[k] = -q[k];
        double dphi0 = dot5(g, d);
        if (!(dphi0 < 0.)) {   // not a descent direction: restart from the gradient
            m = 0;
            for (int k = 0; k < 5; k++) d[k] = -g[k];
            dphi0 = dot5(g, d);
        }
        double alpha = m == 0 && iter == 1 ? fmin(1., 1. / maxabs5(g)) : 1.;
        // strong Wolfe search
        double a_lo = 0., f_lo = f, d_lo = dphi0, a_hi = 0.;
        bool zoom = false, ok = false;
        double xn[5], gn[5], fn = f;
        for (int ls = 0; ls < 20 && !ok && !zoom; ls++) {
            for (int k = 0; k < 5; k++) xn[k] = x[k] + alpha * d[k];
            subpixel_cost(P, xn, fn, gn);
            const double dphi = dot5(gn, d);
            if (!isfinite(fn) || fn > f + c1 * alpha * dphi0 || (ls > 0 && fn >= f_lo)) {
                a_hi = alpha;
                zoom = true;
            } else if (fabs(dphi) <= -c2 * dphi0) {
                ok = true;
            } else if (dphi >= 0.) {
                a_hi = a_lo;
                a_lo = alpha;
                f_lo = fn;
                d_lo = dphi;
                zoom = true;
            } else {
                a_lo = alpha;
                f_lo = fn;
                d_lo = dphi;
                alpha *= 2.;
            }
        }
        for (int z = 0; z < 20 && zoom && !ok; z++) {
            alpha = 0.5 * (a_lo + a_hi);
            if (fabs(a_hi - a_lo) * maxabs5(d) < 1e-12) break;
            for (int k = 0; k < 5; k++) xn[k] = x[k] + alpha * d[k];
            subpixel_cost(P, xn, fn, gn);
            const double dphi = dot5(gn, d);
            if (!isfinite(fn) || fn > f + c1 * alpha * dphi0 || fn >= f_lo) {
                a_hi = alpha;
            } else {
                if (fabs(dphi) <= -c2 * dphi0) {
                    ok = true;
                    break;
                }
                if (dphi * (a_hi - a_lo) >= 0.) a_hi = a_lo;
                a_lo = alpha;
                f_lo = fn;
                d_lo = dphi;
            }
        }
        if (!ok) {   // no Wolfe point: take the best sufficient-decrease point seen, if any, and stop
            if (a_lo > 0.) {
                for (int k = 0; k < 5; k++) x[k] += a_lo * d[k];
                subpixel_cost(P, x, f, g);
            }
            break;
        }
        (void)d_lo;
        double s[5], y[5];
        for (int k = 0; k < 5; k++) {
            s[k] = xn[k] - x[k];
            y[k] = gn[k] - g[k];
        }
        const double sy = dot5(s, y);
        if (sy > 1e-300) {
#pragma unroll
            for (int j = kLbfgsRank - 1; j > 0; j--) {
                for (int k = 0; k < 5; k++) {
                    S[j][k] = S[j - 1][k];
                    Y[j][k] = Y[j - 1][k];
                }
                rho[j] = rho[j - 1];
            }
            for (int k = 0; k < 5; k++) {
                S[0][k] = s[k];
                Y[0][k] = y[k];
            }
            rho[0] = 1. / sy;
            m = min(m + 1, kLbfgsRank);
        }
        const double fprev = f;
        const double xnorm = sqrt(dot5(x, x)), snorm = sqrt(dot5(s, s));
        for (int k = 0; k < 5; k++) {
            x[k] = xn[k];
            g[k] = gn[k];
        }
        f = fn;
        if (fabs(fprev - f) <= 1e-6 * fabs(fprev)) break;
        if (snorm <= 1e-8 * (xnorm + 1e-8)) break;
    }
    a.out[2 * i] = x[0];
    a.out[2 * i + 1] = x[1];
}

}  // namespace vg
