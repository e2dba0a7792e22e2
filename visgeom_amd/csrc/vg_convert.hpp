// vg_convert.hpp -- conversion between camera models (include/visgeom_amd.h section 20): the batched
// pixel -> unit ray kernel, the destination-camera -> source-camera remap maps, and the evaluation kernel of the intrinsic fit.
// Kernels only; the entries are in vg_convert_tu.hip.
//
// The map kernel keeps the layout of vg_rectify_map_kernel (vg_rectify.hpp): 2-D output tiles of kTileW x kTileH pixels, a
// workgroup of 64 x 4 lanes, every lane 4 horizontally adjacent pixels of one row, float4 stores when the row length is a
// multiple of 4 and the buffers are 16-byte aligned (VEC), element stores otherwise: 5 x 5 x 2 = 50 instantiations (DESIGN.md
// section 5.27 has the unit's compile time).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "vg_camera.hpp"
#include "vg_image_device.hpp"
#include "vg_rectify.hpp"
#include "vg_unproject.hpp"

namespace vg {

constexpr int kConvertLanes = 256;
constexpr int kConvertMaxK = 10;                                                // Mei
constexpr int kConvertMaxSums = kConvertMaxK * (kConvertMaxK + 1) / 2 + kConvertMaxK + 1;   // J^T J upper | J^T r | cost
constexpr int kConvertMaxGrid = 1 << 20;                                        // samples of a fit

struct UnprojectArgs {
    double intr[kConvertMaxK];
    int64_t n;
    const double *uv;    // [n][2]
    double *rays;        // [n][3]
    uint8_t *ok;         // [n]
};

// one lane per pixel: the unit ray, (0, 0, 0) and ok = 0 where the pixel is outside the model's domain
template <int MODEL>
__global__ __launch_bounds__(kConvertLanes) void vg_unproject_kernel(UnprojectArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kConvertLanes + threadIdx.x;
    if (i >= a.n) return;
    double X[3];
    const bool ok = unproject_unit<MODEL>(a.intr, a.uv[2 * i], a.uv[2 * i + 1], X);
    a.rays[3 * i] = X[0];
    a.rays[3 * i + 1] = X[1];
    a.rays[3 * i + 2] = X[2];
    a.ok[i] = ok ? 1 : 0;
}

struct ConvertMapArgs {
    double dst_intr[kConvertMaxK], src_intr[kConvertMaxK];
    double R[9];                  // destination -> source frame; the models are central: no translation
    int width, height;
    float *map_x, *map_y;         // [height][width]
};

// one pixel (j, i) of the destination camera: its ray (not normalised), turned, projected by the source camera in eval_corner's
// order; a failed unprojection or projection -> (-1, -1)
template <int DST, int SRC>
__device__ __forceinline__ void convert_pixel(const ConvertMapArgs &a, double j, double i, float &mx, float &my)
{
    double X[3] = {0., 0., 0.};
    const bool seen = unproject<DST>(a.dst_intr, j, i, X);
    const double x = a.R[0] * X[0] + a.R[1] * X[1] + a.R[2] * X[2];
    const double y = a.R[3] * X[0] + a.R[4] * X[1] + a.R[5] * X[2];
    const double z = a.R[6] * X[0] + a.R[7] * X[1] + a.R[8] * X[2];
    CornerEval<CameraTraits<SRC>::K> e;
    eval_corner<SRC, false, false>(a.src_intr, x, y, z, e);
    const bool ok = seen && e.ok;
    mx = ok ? (float)e.u : -1.f;
    my = ok ? (float)e.v : -1.f;
}

template <int DST, int SRC, bool VEC>
__global__ __launch_bounds__(256) void vg_convert_map_kernel(ConvertMapArgs a)
{
    const int row = blockIdx.y * kRectLanesY + threadIdx.y;
    const int col0 = (blockIdx.x * kRectLanesX + threadIdx.x) * kRectPix;
    if (row >= a.height || col0 >= a.width) return;
    float mx[kRectPix], my[kRectPix];
#pragma unroll
    for (int k = 0; k < kRectPix; k++) convert_pixel<DST, SRC>(a, (double)(col0 + k), (double)row, mx[k], my[k]);
    const size_t o = (size_t)row * (size_t)a.width + (size_t)col0;
    if (VEC) {   // the width is a multiple of 4: col0 + 3 < width
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

struct ConvertEvalArgs {
    double intr[kConvertMaxK];    // the destination model's intrinsics at the point of evaluation
    int n;                        // kept samples
    const double *rays;           // [n][3] unit rays of the source camera
    const double *uv;             // [n][2] the pixels they came from
    double *partials;             // [gridDim.x][S], S = K (K + 1) / 2 + K + 1
    int *first_bad;               // the lowest sample index whose projection failed (starts at INT_MAX)
    double *residuals;            // [n][2] or NULL
};

// One evaluation of the fit's cost 1/2 sum |pi_dst(ray) - uv|^2: one lane per sample, the residual pair and the two intrinsic
// Jacobian rows through eval_corner<DST, false, true>, then the sums [J^T J upper triangle row-major | J^T r | cost] of the
// workgroup in the fixed order of vgs::block_sums (butterfly inside a wave, ((w0 + w1) + w2) + w3 across the waves): one row of
// partials per workgroup, summed by the host in index order.  No floating-point atomics: two launches give the same bits.
template <int DST>
__global__ __launch_bounds__(kConvertLanes) void vg_convert_eval_kernel(ConvertEvalArgs a)
{
    constexpr int K = CameraTraits<DST>::K, S = K * (K + 1) / 2 + K + 1;
    const int i = blockIdx.x * kConvertLanes + threadIdx.x;
    double s[S];
#pragma unroll
    for (int q = 0; q < S; q++) s[q] = 0.;
    if (i < a.n) {
        CornerEval<K> e;
        eval_corner<DST, false, true>(a.intr, a.rays[3 * i], a.rays[3 * i + 1], a.rays[3 * i + 2], e);
        if (!e.ok) atomicMin(a.first_bad, i);
        const double ru = e.ok ? e.u - a.uv[2 * i] : 0., rv = e.ok ? e.v - a.uv[2 * i + 1] : 0.;
        if (a.residuals) {
            a.residuals[2 * i] = ru;
            a.residuals[2 * i + 1] = rv;
        }
        int q = 0;
#pragma unroll
        for (int r = 0; r < K; r++)
#pragma unroll
            for (int c = r; c < K; c++, q++) s[q] = e.ok ? e.Ju[r] * e.Ju[c] + e.Jv[r] * e.Jv[c] : 0.;
#pragma unroll
        for (int r = 0; r < K; r++, q++) s[q] = e.ok ? e.Ju[r] * ru + e.Jv[r] * rv : 0.;
        s[q] = 0.5 * (ru * ru + rv * rv);
    }
    vgs::block_sums<S, kConvertLanes>(s, a.partials + (size_t)blockIdx.x * S);
}

}  // namespace vg
