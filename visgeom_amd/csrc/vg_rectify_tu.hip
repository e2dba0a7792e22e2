// vg_rectify_tu.hip -- translation unit of libvisgeom_amd.so: fisheye rectification (vg_rectify_map, vg_remap).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
// Both entries are stateless and asynchronous on the caller's stream: no allocation, no synchronisation, no host round trip
// (a caller may capture them in a graph).
#include <cmath>
#include <cstdint>
#include <string>

#include "vg_internal.hpp"
#include "vg_rectify.hpp"
#include "vg_transf_host.hpp"

namespace {

using vgi::fail;

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

bool valid_dim(int d) { return d >= 1 && d <= vg::kRectMaxDim; }

template <int MODEL>
void launch_map(const vg::RectifyMapArgs &a, bool vec, hipStream_t st)
{
    const dim3 grid((unsigned)((a.width + vg::kTileW - 1) / vg::kTileW), (unsigned)((a.height + vg::kTileH - 1) / vg::kTileH));
    const dim3 blk(vg::kRectLanesX, vg::kRectLanesY);
    if (vec) hipLaunchKernelGGL((vg::vg_rectify_map_kernel<MODEL, true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((vg::vg_rectify_map_kernel<MODEL, false>), grid, blk, 0, st, a);
}

template <typename T, int C>
void launch_remap(const vg::RemapArgs &a, bool vec, hipStream_t st)
{
    const dim3 grid((unsigned)((a.map_w + vg::kTileW - 1) / vg::kTileW), (unsigned)((a.map_h + vg::kTileH - 1) / vg::kTileH));
    const dim3 blk(vg::kRectLanesX, vg::kRectLanesY);
    if (vec) hipLaunchKernelGGL((vg::vg_remap_kernel<T, C, true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((vg::vg_remap_kernel<T, C, false>), grid, blk, 0, st, a);
}

template <typename T>
void launch_remap_channels(int channels, const vg::RemapArgs &a, bool vec, hipStream_t st)
{
    switch (channels) {
    case 1: launch_remap<T, 1>(a, vec, st); break;
    case 3: launch_remap<T, 3>(a, vec, st); break;
    default: launch_remap<T, 4>(a, vec, st); break;
    }
}

}  // namespace

extern "C" {

int vg_rectify_map(int device, void *hip_stream, int model, const double *intrinsics, const double *pinhole5, const double *xi6,
                   float *map_x, float *map_y)
{
    const int K = vg::num_intrinsics(model);
    if (K < 0) return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
    if (!intrinsics || !pinhole5 || !xi6 || !map_x || !map_y) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const double w = pinhole5[0], h = pinhole5[1];
    if (!(w == std::floor(w) && h == std::floor(h) && w >= 1. && h >= 1. && w <= vg::kRectMaxDim && h <= vg::kRectMaxDim))
        return fail(VG_ERR_INVALID_ARGUMENT, "pinhole width / height must be integers in [1, 16384]");
    if (!(std::isfinite(pinhole5[2]) && std::isfinite(pinhole5[3]) && std::isfinite(pinhole5[4]) && pinhole5[4] != 0.))
        return fail(VG_ERR_INVALID_ARGUMENT, "pinhole u0, v0, f must be finite and f non-zero");
    if (const int rc = vgi::check_device(device, "rectification")) return rc;
    vg::RectifyMapArgs a;
    for (int k = 0; k < 10; k++) a.intr[k] = k < K ? intrinsics[k] : 0.;
    const vg::RotTrig g = vg::rot_trig(xi6 + 3, true, false);
    vg::rotation_matrix(xi6 + 3, 1., g, a.R);   // Transformation::rotMat
    for (int i = 0; i < 3; i++) a.t[i] = xi6[i];
    a.u0 = pinhole5[2];
    a.v0 = pinhole5[3];
    a.f = pinhole5[4];
    a.width = (int)w;
    a.height = (int)h;
    a.map_x = map_x;
    a.map_y = map_y;
    const bool vec = a.width % vg::kRectPix == 0 && aligned16(map_x) && aligned16(map_y);
    VG_HIP(hipSetDevice(device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (!vg::dispatch_model(model, vg::AllModels{}, [&](auto m) { launch_map<decltype(m)::value>(a, vec, st); }))
        return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
    VG_HIP(hipGetLastError());
    return VG_OK;
}

int vg_remap(int device, void *hip_stream, int pixel_type, int channels, int64_t n_images, int src_w, int src_h, const void *src,
             int map_w, int map_h, const float *map_x, const float *map_y, double fill, void *dst)
{
    if (pixel_type != VG_PIXEL_U8 && pixel_type != VG_PIXEL_F32) return fail(VG_ERR_INVALID_ARGUMENT, "unknown pixel type");
    if (channels != 1 && channels != 3 && channels != 4) return fail(VG_ERR_INVALID_ARGUMENT, "channels must be 1, 3 or 4");
    if (n_images < 0) return fail(VG_ERR_INVALID_ARGUMENT, "negative image count");
    if (!valid_dim(src_w) || !valid_dim(src_h) || !valid_dim(map_w) || !valid_dim(map_h))
        return fail(VG_ERR_INVALID_ARGUMENT, "image and map sides must be in [1, 16384]");
    if (!map_x || !map_y || (n_images > 0 && (!src || !dst))) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = vgi::check_device(device, "remap")) return rc;
    if (n_images == 0) return VG_OK;
    vg::RemapArgs a;
    a.src = src;
    a.dst = dst;
    a.map_x = map_x;
    a.map_y = map_y;
    a.n_images = n_images;
    a.src_w = src_w;
    a.src_h = src_h;
    a.map_w = map_w;
    a.map_h = map_h;
    a.fill = (float)fill;
    const bool vec = map_w % vg::kRectPix == 0 && aligned16(map_x) && aligned16(map_y) && aligned16(dst);
    VG_HIP(hipSetDevice(device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    if (pixel_type == VG_PIXEL_U8) launch_remap_channels<uint8_t>(channels, a, vec, st);
    else launch_remap_channels<float>(channels, a, vec, st);
    VG_HIP(hipGetLastError());
    return VG_OK;
}

}  // extern "C"
