// vg_rectify.hpp -- fisheye rectification (the reference's `rectify` program, test/calibration/rectify.cpp): the
// pinhole -> camera undistortion maps (initRemap, :27-58) and a batched bilinear remap (cv::remap INTER_LINEAR,
// BORDER_CONSTANT) of many same-size images through one map pair.  Kernels only; the entries are in vg_rectify_tu.hip.
//
// Both kernels work on 2-D output tiles of kTileW x kTileH pixels: a workgroup is 64 x 4 lanes, every lane owns 4
// horizontally adjacent pixels of one row.  When the row length is a multiple of 4 (and the buffers are 16-byte aligned)
// a lane's map entries are one float4 each and its outputs whole dwords / float4s (VEC); otherwise every element is
// loaded and stored on its own, with the same arithmetic.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "vg_camera.hpp"

namespace vg {

constexpr int kRectLanesX = 64, kRectLanesY = 4, kRectPix = 4;
constexpr int kTileW = kRectLanesX * kRectPix, kTileH = kRectLanesY;
constexpr int kRectMaxDim = 16384;   // every image / map side: pixel offsets inside one image stay below 2^30 elements

struct RectifyMapArgs {
    double intr[10];
    double R[9], t[3];            // X' = R X + t   (Transformation::transform, transformation.h:167-171)
    double u0, v0, f;             // the pinhole (pinhole.h:40-49)
    int width, height;
    float *map_x, *map_y;         // [height][width]
};

// one pixel: reconstruct through the pinhole, move, project in the reference's FP64 order; a failed projection -> (-1, -1)
template <int MODEL>
__device__ __forceinline__ void rectify_pixel(const RectifyMapArgs &a, double j, double i, float &mx, float &my)
{
    const double X0 = (j - a.u0) / a.f, X1 = (i - a.v0) / a.f, X2 = 1.;
    const double x = a.R[0] * X0 + a.R[1] * X1 + a.R[2] * X2 + a.t[0];
    const double y = a.R[3] * X0 + a.R[4] * X1 + a.R[5] * X2 + a.t[1];
    const double z = a.R[6] * X0 + a.R[7] * X1 + a.R[8] * X2 + a.t[2];
    CornerEval<CameraTraits<MODEL>::K> e;
    eval_corner<MODEL, false, false>(a.intr, x, y, z, e);
    mx = e.ok ? (float)e.u : -1.f;
    my = e.ok ? (float)e.v : -1.f;
}

template <int MODEL, bool VEC>
__global__ __launch_bounds__(256) void vg_rectify_map_kernel(RectifyMapArgs a)
{
    const int row = blockIdx.y * kRectLanesY + threadIdx.y;
    const int col0 = (blockIdx.x * kRectLanesX + threadIdx.x) * kRectPix;
    if (row >= a.height || col0 >= a.width) return;
    float mx[kRectPix], my[kRectPix];
#pragma unroll
    for (int k = 0; k < kRectPix; k++) rectify_pixel<MODEL>(a, (double)(col0 + k), (double)row, mx[k], my[k]);
    const size_t o = (size_t)row * (size_t)a.width + (size_t)col0;
    if (VEC) {
        *reinterpret_cast<float4 *>(a.map_x + o) = make_float4(mx[0], mx[1], mx[2], mx[3]);
        *reinterpret_cast<float4 *>(a.map_y + o) = make_float4(my[0], my[1], my[2], my[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kRectPix; k++)
            if (col0 + k < a.width) {
                a.map_x[o + k] = mx[k];
                a.map_y[o + k] = my[k];
            }
    }
}

struct RemapArgs {
    const void *src;               // [n][src_h][src_w][C]
    void *dst;                     // [n][map_h][map_w][C]
    const float *map_x, *map_y;    // [map_h][map_w]
    int64_t n_images;
    int src_w, src_h, map_w, map_h;
    float fill;
};

__device__ __forceinline__ float remap_out(float v, float) { return v; }
__device__ __forceinline__ uint8_t remap_out(float v, uint8_t)   // saturate_cast<uchar>: round half to even, clamp
{
    return (uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f);
}

// One lane: 4 output pixels of a row.  Their map entries are read once, the tap offset / weights / border mask computed
// once, then the lane walks every image of the batch (the map traffic is paid once per launch, not once per image).
template <typename T, int C, bool VEC>
__global__ __launch_bounds__(256) void vg_remap_kernel(RemapArgs a)
{
    const int row = blockIdx.y * kRectLanesY + threadIdx.y;
    const int col0 = (blockIdx.x * kRectLanesX + threadIdx.x) * kRectPix;
    if (row >= a.map_h || col0 >= a.map_w) return;
    const size_t opix = (size_t)row * (size_t)a.map_w + (size_t)col0;
    float mx[kRectPix], my[kRectPix];
    if (VEC) {
        const float4 vx = *reinterpret_cast<const float4 *>(a.map_x + opix);
        const float4 vy = *reinterpret_cast<const float4 *>(a.map_y + opix);
        mx[0] = vx.x; mx[1] = vx.y; mx[2] = vx.z; mx[3] = vx.w;
        my[0] = vy.x; my[1] = vy.y; my[2] = vy.z; my[3] = vy.w;
    } else {
#pragma unroll
        for (int k = 0; k < kRectPix; k++) {
            const bool in = col0 + k < a.map_w;
            mx[k] = in ? a.map_x[opix + k] : -1.f;
            my[k] = in ? a.map_y[opix + k] : -1.f;
        }
    }
    const float W = (float)a.src_w, H = (float)a.src_h;
    // tap addresses are clamped into the image so that every load is unconditional; the taps outside it are replaced by fill
    // after the load (bits of m)
    int off[kRectPix], dx[kRectPix], dy[kRectPix];   // elements: tap (x0, y0) of one image; to (x1, .); to (., y1)
    unsigned m[kRectPix];    // bit 0: (x0,y0)  1: (x1,y0)  2: (x0,y1)  3: (x1,y1) inside the image; bit 4: the pixel is fill
    float ax[kRectPix], ay[kRectPix];
#pragma unroll
    for (int k = 0; k < kRectPix; k++) {
        // tested before any float -> int conversion: NaN and huge values land here
        const bool inside = mx[k] > -1.f && mx[k] < W && my[k] > -1.f && my[k] < H;
        const float fx = inside ? floorf(mx[k]) : 0.f, fy = inside ? floorf(my[k]) : 0.f;
        ax[k] = inside ? mx[k] - fx : 0.f;
        ay[k] = inside ? my[k] - fy : 0.f;
        const int x0 = (int)fx, y0 = (int)fy;   // in [-1, W-1] x [-1, H-1]
        const bool vx0 = x0 >= 0, vx1 = x0 + 1 < a.src_w, vy0 = y0 >= 0, vy1 = y0 + 1 < a.src_h;
        m[k] = inside ? (unsigned)(vx0 && vy0) | (unsigned)(vx1 && vy0) << 1 | (unsigned)(vx0 && vy1) << 2 | (unsigned)(vx1 && vy1) << 3
                      : 16u;
        const int xa = vx0 ? x0 : 0, ya = vy0 ? y0 : 0;
        off[k] = (ya * a.src_w + xa) * C;
        dx[k] = (vx0 && vx1) ? C : 0;
        dy[k] = (vy0 && vy1) ? a.src_w * C : 0;
    }
    const size_t src_img = (size_t)a.src_w * (size_t)a.src_h * C, dst_img = (size_t)a.map_w * (size_t)a.map_h * C;
    const T *src = static_cast<const T *>(a.src);
    T *dst = static_cast<T *>(a.dst) + opix * C;
    const float fill = a.fill;
    for (int64_t n = 0; n < a.n_images; n++, src += src_img, dst += dst_img) {
        alignas(16) T out[kRectPix * C];
#pragma unroll
        for (int k = 0; k < kRectPix; k++) {
            const T *p = src + off[k];
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float t00 = (float)p[c], t01 = (float)p[dx[k] + c], t10 = (float)p[dy[k] + c], t11 = (float)p[dy[k] + dx[k] + c];
                const float p00 = (m[k] & 1u) ? t00 : fill;
                const float p01 = (m[k] & 2u) ? t01 : fill;
                const float p10 = (m[k] & 4u) ? t10 : fill;
                const float p11 = (m[k] & 8u) ? t11 : fill;
                const float bx = 1.f - ax[k], by = 1.f - ay[k];
                const float v = by * (bx * p00 + ax[k] * p01) + ay[k] * (bx * p10 + ax[k] * p11);
                out[k * C + c] = remap_out((m[k] & 16u) ? fill : v, T());
            }
        }
        if (VEC) {
            // 4 C sizeof(T) bytes per lane: whole 16-byte chunks when they divide it, dwords otherwise (u8 with C = 1 or 3)
            constexpr int kWords = kRectPix * C * (int)sizeof(T) / 4;
            const uint32_t *w = reinterpret_cast<const uint32_t *>(out);
            if (kWords % 4 == 0) {
#pragma unroll
                for (int q = 0; q < kWords / 4; q++)
                    reinterpret_cast<uint4 *>(dst)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
            } else {
#pragma unroll
                for (int q = 0; q < kWords; q++) reinterpret_cast<uint32_t *>(dst)[q] = w[q];
            }
        } else {
#pragma unroll
            for (int k = 0; k < kRectPix; k++)
                if (col0 + k < a.map_w)
#pragma unroll
                    for (int c = 0; c < C; c++) dst[k * C + c] = out[k * C + c];
        }
    }
}

}  // namespace vg
