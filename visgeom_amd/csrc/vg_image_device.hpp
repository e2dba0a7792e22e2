// vg_image_device.hpp -- the small device pieces the image pipelines share, one definition each: the depth grid, the
// BORDER_REFLECT_101 index, the float Sobel / 8 at one pixel, the u8 -> float conversion, the per-wave counters and the ordered
// reduction of a workgroup.  Everything is evaluated in the order written (-ffp-contract=off); the restatements in tests/ follow
// that order, so a change here moves the bits of every pipeline that includes it together.  DESIGN.md section 5.23.
#pragma once

#include "vg_stereo_device.hpp"

namespace vgs {

struct Grid {   // ScaleParameters of a depth map
    int scale, u0, v0, x_max, y_max;
};

// BORDER_REFLECT_101 for an overhang below n, then clamped: a one-pixel axis has only itself.  With a = |i| the reflected index
// is a below n and 2 n - 2 - a from n on, which is the smaller of the two in both cases (they add up to 2 n - 2); the smaller one
// never exceeds n - 1, so only the clamp at 0 is left.
VGS_HD int reflect101(int i, int n)
{
    const int a = i < 0 ? -i : i, b = 2 * n - 2 - a;
    const int m = a < b ? a : b;
    return m < 0 ? 0 : m;
}

// Sobel(img, CV_32F, 1, 0, 3, 1./8) and (0, 1) at pixel (u, v) of the w x h image s: smoothing [1 2 1] across, difference
// [-1 0 1] along, in float, ((d0 + 2 d1) + d2) * 0.125
VGS_HD void sobel8_at(const float *s, int w, int h, int u, int v, float &gu, float &gv)
{
    const int um = reflect101(u - 1, w), up = reflect101(u + 1, w), vm = reflect101(v - 1, h), vp = reflect101(v + 1, h);
    const float *r0 = s + (int64_t)vm * w, *r1 = s + (int64_t)v * w, *r2 = s + (int64_t)vp * w;
    const float du0 = r0[up] - r0[um], du1 = r1[up] - r1[um], du2 = r2[up] - r2[um];
    const float dv0 = r2[um] - r0[um], dv1 = r2[u] - r0[u], dv2 = r2[up] - r0[up];
    gu = ((du0 + 2.f * du1) + du2) * 0.125f;
    gv = ((dv0 + 2.f * dv1) + dv2) * 0.125f;
}

// Mat8u::convertTo(CV_32F) of gridDim.y images of P pixels; image i goes to dst + i * item_stride.  A template, so that every
// translation unit that launches it may hold its instantiation.
template <int LANES>
__global__ __launch_bounds__(LANES) void u8_to_float_kernel(const uint8_t *src, float *dst, int64_t P, int64_t item_stride)
{
    const int64_t item = blockIdx.y, pix = (int64_t)blockIdx.x * LANES + threadIdx.x;
    if (pix < P) dst[item * item_stride + pix] = (float)src[item * P + pix];
}

// every lane of the block calls these: one atomic per wave and counter
__device__ __forceinline__ void count_wave(unsigned long long *c, bool hit)
{
    const int k = __popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(c, (unsigned long long)k);
}
__device__ __forceinline__ void count_wave(unsigned long long *c, int k)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) k += __shfl_xor(k, off);
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(c, (unsigned long long)k);
}

// The ordered reduction of a workgroup of LANES = 256 lanes: N values per lane, each through the xor butterfly 32 -> 1 (a fixed
// tree: every lane of a wave ends with the same bits), lane 0 of every wave to LDS, then thread k < N stores
// ((w0 + w1) + w2) + w3 to out[k].  Slot MAX (none by default) is a maximum instead of a sum.  It holds a barrier: every thread
// of the workgroup calls it.
template <int N, int LANES, int MAX = -1>
__device__ __forceinline__ void block_sums(double (&s)[N], double *out)
{
    static_assert(LANES == 256, "the association ((w0 + w1) + w2) + w3 is written out for four waves");
    __shared__ double wave_sums[LANES / 64][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double o = __shfl_xor(s[k], off, 64);
            s[k] = k == MAX ? fmax(s[k], o) : s[k] + o;
        }
        if (lane == 0) wave_sums[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int k = threadIdx.x;
        const double *w0 = wave_sums[0], *w1 = wave_sums[1], *w2 = wave_sums[2], *w3 = wave_sums[3];
        out[k] = (MAX >= 0 && k == MAX) ? fmax(fmax(fmax(w0[k], w1[k]), w2[k]), w3[k]) : ((w0[k] + w1[k]) + w2[k]) + w3[k];
    }
}

}  // namespace vgs
