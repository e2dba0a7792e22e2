// vg_depth_tu.hip -- translation unit of libvisgeom_amd.so: depth map propagation and fusion (section 11 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_depth_fusion handle owns the scratch of its three operations: the warp's z-buffer and winner buffer (12 bytes per
// depth pixel and item, all ones between calls: the gather kernel restores what it read), the per-item poses and counters in
// one pinned and one device array, and the copy the noise filter reads when it runs in place.  Buffers only grow.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>

#include "vg_depth.hpp"
#include "vg_internal.hpp"
#include "vg_stereo_host.hpp"
#include "vg_transf_host.hpp"

struct vg_depth_fusion {
    int device = 0;
    hipStream_t stream = nullptr;
    double cam[6];
    vgd::Grid g;
    int64_t P = 0;
    int64_t cap_items = 0;    // items d_item / h_item / d_counts / h_counts hold
    int64_t cap_warp = 0;     // items the z-buffer and the winner buffer hold
    int64_t cap_filter = 0;   // items the filter's copy holds
    bool warp_clean = false;  // the z-buffer and the winner buffer are all ones
    vgi::DeviceMem<vgd::WarpItem> d_item;
    vgi::PinnedMem<vgd::WarpItem> h_item;
    vgi::DeviceMem<unsigned long long> d_counts, d_zbuf;
    vgi::PinnedMem<unsigned long long> h_counts;
    vgi::DeviceMem<unsigned> d_winner;
    vgi::DeviceMem<double> d_copy;   // [2][n][P]
#ifdef VG_DEPTH_WARP_STORE
    vgi::DeviceMem<int> d_src_target;
    vgi::DeviceMem<double> d_src_dist;
#endif
};

namespace {

using vgi::fail;
using vgsh::blocks_of;
constexpr int64_t kMaxItems = 65535;   // items ride on gridDim.y
constexpr int kMaxCounters = 6;

int ensure_items(vg_depth_fusion *s, int64_t n)
{
    if (n <= s->cap_items) return VG_OK;
    s->cap_items = 0;
    const size_t items = (size_t)n * sizeof(vgd::WarpItem), counts = (size_t)n * kMaxCounters * sizeof(unsigned long long);
    if (s->d_item.alloc(items) != hipSuccess || s->d_counts.alloc(counts) != hipSuccess)
        return fail(VG_ERR_ALLOC, "device allocation of the depth fusion items failed");
    if (s->h_item.alloc(items, hipHostMallocDefault) != hipSuccess || s->h_counts.alloc(counts, hipHostMallocDefault) != hipSuccess)
        return fail(VG_ERR_ALLOC, "pinned allocation of the depth fusion staging failed");
    s->cap_items = n;
    return VG_OK;
}

bool overlap(const void *a, const void *b, size_t bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

// true when two of the k arrays of `bytes` bytes overlap
bool any_overlap(const void *const *p, int k, size_t bytes)
{
    for (int i = 0; i < k; i++)
        for (int j = i + 1; j < k; j++)
            if (overlap(p[i], p[j], bytes)) return true;
    return false;
}

int check_call(const vg_depth_fusion *s, int64_t n)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "depth fusion handle is NULL");
    if (n < 0 || n > kMaxItems) return fail(VG_ERR_INVALID_ARGUMENT, "the item count must be in [0, 65535]");
    return VG_OK;
}

// an elementwise call's counters: zeroed before the launch, read back after it
int counts_begin(vg_depth_fusion *s, int64_t n, int k, int64_t *counts, unsigned long long **dev)
{
    *dev = nullptr;
    if (!counts) return VG_OK;
    if (const int rc = ensure_items(s, n)) return rc;
    VG_HIP(hipMemsetAsync(s->d_counts, 0, (size_t)n * k * sizeof(unsigned long long), s->stream));
    *dev = s->d_counts.get();
    return VG_OK;
}

int counts_end(vg_depth_fusion *s, int64_t n, int k, int64_t *counts, vgi::StreamDrain &drain)
{
    if (counts) VG_HIP(hipMemcpyAsync(s->h_counts, s->d_counts, (size_t)n * k * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    drain.armed = false;
    VG_HIP(hipStreamSynchronize(s->stream));
    if (counts)
        for (int64_t i = 0; i < n * k; i++) counts[i] = (int64_t)s->h_counts.get()[i];
    return VG_OK;
}

}  // namespace

extern "C" {

int vg_depth_fusion_create(vg_depth_fusion **out, int device, void *hip_stream, const double *eucm, const vg_stereo_params *params)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (!eucm || !params) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const vg_stereo_params &p = *params;   // only the ScaleParameters fields are read, under vg_stereo_create's ranges
    if (p.scale < 1 || p.scale > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "scale must be in [1, 16384]");
    if (p.u_max < 1 || p.u_max > 16384 || p.v_max < 1 || p.v_max > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "uMax / vMax must be in [1, 16384]");
    if (std::abs(p.u0) > 16384 || std::abs(p.v0) > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "|u0|, |v0| must be at most 16384");
    int x_max = p.x_max, y_max = p.y_max;
    if (p.equal_margins) {   // ScaleParameters::setEqualMargin (scale_parameters.cpp:44-52)
        x_max = (p.u_max - 2 * p.u0) / p.scale + 1;
        y_max = (p.v_max - 2 * p.v0) / p.scale + 1;
    }
    if (x_max < 1 || y_max < 1) return fail(VG_ERR_INVALID_ARGUMENT, "the scaled image is empty: xMax < 1 or yMax < 1");
    if (x_max > 16384 || y_max > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "xMax / yMax must be at most 16384");
    if (!vgsh::finite_n(eucm, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "camera parameters must be finite");
    if (!vgsh::focal_nonzero(eucm, eucm)) return fail(VG_ERR_INVALID_ARGUMENT, "fu, fv must be non-zero");
    std::unique_ptr<vg_depth_fusion> s(new (std::nothrow) vg_depth_fusion());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    for (int i = 0; i < 6; i++) s->cam[i] = eucm[i];
    s->g = vgd::Grid{p.scale, p.u0, p.v0, x_max, y_max};
    s->P = (int64_t)x_max * y_max;
    if (const int rc = vgi::check_device(device, "depth fusion")) return rc;
    s->device = device;
    s->stream = reinterpret_cast<hipStream_t>(hip_stream);
    *out = s.release();
    return VG_OK;
}

void vg_depth_fusion_destroy(vg_depth_fusion *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    delete s;
}

int vg_depth_fusion_size(const vg_depth_fusion *s, int *x_max, int *y_max)
{
    if (!s || !x_max || !y_max) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *x_max = s->g.x_max;
    *y_max = s->g.y_max;
    return VG_OK;
}

int vg_depth_warp(vg_depth_fusion *s, int64_t n, const double *xi12, const double *depth_in, const double *sigma_in, const double *cost_in,
                  double *depth, double *sigma, double *cost, int64_t *counts)
{
    if (const int rc = check_call(s, n)) return rc;
    if (n == 0) return VG_OK;
    if (!xi12 || !depth_in || !sigma_in || !cost_in || !depth || !sigma || !cost) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const size_t bytes = (size_t)(n * s->P) * sizeof(double);
    const void *const out[3] = {depth, sigma, cost}, *const in[3] = {depth_in, sigma_in, cost_in};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            if (overlap(out[i], in[j], bytes)) return fail(VG_ERR_INVALID_ARGUMENT, "the warp is a scatter: its outputs must not alias its inputs");
    if (any_overlap(out, 3, bytes)) return fail(VG_ERR_INVALID_ARGUMENT, "the outputs overlap each other");
    if (!vgsh::finite_n(xi12, 6 * (int)n)) return fail(VG_ERR_INVALID_ARGUMENT, "the transformations must be finite");
    VG_HIP(hipSetDevice(s->device));
    if (const int rc = ensure_items(s, n)) return rc;
    if (n > s->cap_warp) {
        s->cap_warp = 0;
        s->warp_clean = false;
        if (s->d_zbuf.alloc((size_t)(n * s->P) * sizeof(unsigned long long)) != hipSuccess ||
            s->d_winner.alloc((size_t)(n * s->P) * sizeof(unsigned)) != hipSuccess)
            return fail(VG_ERR_ALLOC, "device allocation of the warp's z-buffer failed");
#ifdef VG_DEPTH_WARP_STORE
        if (s->d_src_target.alloc((size_t)(n * s->P) * sizeof(int)) != hipSuccess || s->d_src_dist.alloc(bytes) != hipSuccess)
            return fail(VG_ERR_ALLOC, "device allocation of the warp's source records failed");
#endif
        s->cap_warp = n;
    }
    for (int64_t k = 0; k < n; k++) {   // R^T and t in FP64, with the rotation code of vg_stereo_host.hpp's build_geometry
        vgd::WarpItem &it = s->h_item.get()[k];
        const double *xi = xi12 + 6 * k;
        const vg::RotTrig rt = vg::rot_trig(xi + 3, true, false);
        vg::rotation_matrix(xi + 3, -1., rt, it.Rinv);
        for (int i = 0; i < 3; i++) it.t[i] = xi[i];
        for (int i = 0; i < 6; i++) it.counts[i] = 0;
    }
    vgi::StreamDrain drain{s->stream};
    if (!s->warp_clean) {
        VG_HIP(hipMemsetAsync(s->d_zbuf, 0xff, (size_t)(s->cap_warp * s->P) * sizeof(unsigned long long), s->stream));
        VG_HIP(hipMemsetAsync(s->d_winner, 0xff, (size_t)(s->cap_warp * s->P) * sizeof(unsigned), s->stream));
    }
    s->warp_clean = false;
    VG_HIP(hipMemcpyAsync(s->d_item, s->h_item, (size_t)n * sizeof(vgd::WarpItem), hipMemcpyHostToDevice, s->stream));
    vgd::WarpArgs a;
    a.item = s->d_item;
    for (int i = 0; i < 6; i++) a.cam[i] = s->cam[i];
    a.g = s->g;
    a.P = s->P;
    a.depth_in = depth_in;
    a.sigma_in = sigma_in;
    a.cost_in = cost_in;
    a.zbuf = s->d_zbuf;
    a.winner = s->d_winner;
    a.depth = depth;
    a.sigma = sigma;
    a.cost = cost;
    a.count = counts != nullptr;
#ifdef VG_DEPTH_WARP_STORE
    a.src_target = s->d_src_target;
    a.src_dist = s->d_src_dist;
#endif
    const dim3 grid(blocks_of(s->P, vgd::kLanes), (unsigned)n), block(vgd::kLanes);
    hipLaunchKernelGGL(vgd::depth_warp_zbuf_kernel, grid, block, 0, s->stream, a);
    hipLaunchKernelGGL(vgd::depth_warp_winner_kernel, grid, block, 0, s->stream, a);
    hipLaunchKernelGGL(vgd::depth_warp_gather_kernel, grid, block, 0, s->stream, a);
    VG_HIP(hipGetLastError());
    if (counts) VG_HIP(hipMemcpyAsync(s->h_item, s->d_item, (size_t)n * sizeof(vgd::WarpItem), hipMemcpyDeviceToHost, s->stream));
    drain.armed = false;
    VG_HIP(hipStreamSynchronize(s->stream));
    s->warp_clean = true;
    if (counts)
        for (int64_t k = 0; k < n; k++) {
            const unsigned long long *c = s->h_item.get()[k].counts;   // c[4]: reached a target, c[5]: targets written
            for (int i = 0; i < 4; i++) counts[6 * k + i] = (int64_t)c[i];
            counts[6 * k + 4] = (int64_t)(c[4] - c[5]);   // lost the depth test (ties on the range included)
            counts[6 * k + 5] = (int64_t)c[5];
        }
    return VG_OK;
}

int vg_depth_merge(vg_depth_fusion *s, int64_t n, double *depth, double *sigma, const double *depth2, const double *sigma2, int64_t *counts)
{
    if (const int rc = check_call(s, n)) return rc;
    if (n == 0) return VG_OK;
    if (!depth || !sigma || !depth2 || !sigma2) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const void *const p[4] = {depth, sigma, depth2, sigma2};
    if (any_overlap(p, 4, (size_t)(n * s->P) * sizeof(double))) return fail(VG_ERR_INVALID_ARGUMENT, "the four maps of a merge must not overlap");
    VG_HIP(hipSetDevice(s->device));
    vgi::StreamDrain drain{s->stream};
    unsigned long long *dc = nullptr;
    if (const int rc = counts_begin(s, n, 5, counts, &dc)) return rc;
    hipLaunchKernelGGL(vgd::depth_merge_kernel, dim3(blocks_of(s->P, vgd::kLanes), (unsigned)n), dim3(vgd::kLanes), 0, s->stream, depth, sigma,
                       depth2, sigma2, s->P, dc);
    VG_HIP(hipGetLastError());
    return counts_end(s, n, 5, counts, drain);
}

int vg_depth_filter_noise(vg_depth_fusion *s, int64_t n, const double *depth_in, const double *sigma_in, double *depth, double *sigma,
                          int64_t *counts)
{
    if (const int rc = check_call(s, n)) return rc;
    if (n == 0) return VG_OK;
    if (!depth_in || !sigma_in || !depth || !sigma) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const size_t bytes = (size_t)(n * s->P) * sizeof(double);
    const bool alias_d = depth == depth_in, alias_s = sigma == sigma_in;   // allowed: that input is read from the handle's copy
    if (overlap(depth, sigma, bytes) || (!alias_d && overlap(depth, depth_in, bytes)) || overlap(depth, sigma_in, bytes) ||
        overlap(sigma, depth_in, bytes) || (!alias_s && overlap(sigma, sigma_in, bytes)))
        return fail(VG_ERR_INVALID_ARGUMENT, "an output of the noise filter must be its own input or overlap no input");
    VG_HIP(hipSetDevice(s->device));
    if ((alias_d || alias_s) && n > s->cap_filter) {
        s->cap_filter = 0;
        if (s->d_copy.alloc(2 * bytes) != hipSuccess) return fail(VG_ERR_ALLOC, "device allocation of the noise filter's copy failed");
        s->cap_filter = n;
    }
    vgi::StreamDrain drain{s->stream};
    if (alias_d) {   // the reference's myCopy
        VG_HIP(hipMemcpyAsync(s->d_copy, depth_in, bytes, hipMemcpyDeviceToDevice, s->stream));
        depth_in = s->d_copy;
    }
    if (alias_s) {
        VG_HIP(hipMemcpyAsync(s->d_copy.get() + n * s->P, sigma_in, bytes, hipMemcpyDeviceToDevice, s->stream));
        sigma_in = s->d_copy.get() + n * s->P;
    }
    unsigned long long *dc = nullptr;
    if (const int rc = counts_begin(s, n, 3, counts, &dc)) return rc;
    hipLaunchKernelGGL(vgd::depth_filter_noise_kernel, dim3(blocks_of(s->P, vgd::kLanes), (unsigned)n), dim3(vgd::kLanes), 0, s->stream, depth_in,
                       sigma_in, depth, sigma, s->g, s->P, dc);
    VG_HIP(hipGetLastError());
    return counts_end(s, n, 3, counts, drain);
}

int vg_transform_inverse(const double *xi, double *out6)
{
    if (!xi || !out6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    vgth::Array6d a;
    std::memcpy(a.data(), xi, sizeof(double) * 6);
    const vgth::Array6d r = vgth::inverse(a);
    std::memcpy(out6, r.data(), sizeof(double) * 6);
    return VG_OK;
}

int vg_transform_inverse_compose(const double *a6, const double *b6, double *out6)
{
    if (!a6 || !b6 || !out6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    vgth::Array6d a, b;
    std::memcpy(a.data(), a6, sizeof(double) * 6);
    std::memcpy(b.data(), b6, sizeof(double) * 6);
    const vgth::Array6d r = vgth::inverse_compose(a, b);
    std::memcpy(out6, r.data(), sizeof(double) * 6);
    return VG_OK;
}

}  // extern "C"
