// vg_depth_tu.hip -- translation unit of libvisgeom_amd.so: depth map propagation and fusion (section 11 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_depth_fusion handle owns the scratch of its three operations: the warp's z-buffer and winner buffer (12 bytes per
// depth pixel and item, all ones between calls: the gather kernel restores what it read), the per-item poses with the warp's
// counters in one pinned and one device array, the counters of merge and the noise filter, and the copy the noise filter
// reads when it runs in place, and the block counts of the multi-hypothesis pack.  Buffers only grow.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>

#include "vg_depth.hpp"
#include "vg_handle.hpp"
#include "vg_stereo_host.hpp"
#include "vg_pose_host.hpp"

struct vg_depth_fusion : vgi::HandleBase {
    double cam[6];
    vgd::Grid g;
    int64_t P = 0;
    bool warp_clean = false;  // the z-buffer and the winner buffer are all ones
    vgi::Grow<vgd::WarpItem> d_item;
    vgi::GrowPinned<vgd::WarpItem> h_item;
    vgi::Counters counters;   // of merge and filter_noise; the warp's travel in its items
    vgi::Grow<unsigned long long> d_zbuf;   // [n][P], like the winner buffer
    vgi::Grow<unsigned> d_winner;
    vgi::Grow<double> d_copy;   // [2][n][P]
    vgi::PackScratch pack;   // of the multi-hypothesis pack: per block of 256 pixels; one total
#ifdef VG_DEPTH_WARP_STORE
    vgi::Grow<int> d_src_target;
    vgi::Grow<double> d_src_dist;
#endif
};

namespace {

using vgi::fail;
using vgsh::blocks_of;

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
    return vgi::check_items(n, 0, "item");
}

}  // namespace

extern "C" {

int vg_depth_fusion_create(vg_depth_fusion **out, int device, void *hip_stream, const double *eucm, const vg_stereo_params *params)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (!eucm || !params) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const vg_stereo_params &p = *params;   // only the ScaleParameters fields are read
    int x_max = 0, y_max = 0;
    if (const int rc = vgsh::scaled_grid(p, true, x_max, y_max)) return rc;
    if (const int rc = vgsh::check_camera(eucm)) return rc;
    std::unique_ptr<vg_depth_fusion> s(new (std::nothrow) vg_depth_fusion());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    for (int i = 0; i < 6; i++) s->cam[i] = eucm[i];
    s->g = vgd::Grid{p.scale, p.u0, p.v0, x_max, y_max};
    s->P = (int64_t)x_max * y_max;
    if (const int rc = s->open(device, hip_stream, "depth fusion")) return rc;
    *out = s.release();
    return VG_OK;
}

void vg_depth_fusion_destroy(vg_depth_fusion *s) { vgi::destroy(s); }

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
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (const int rc = s->d_item.grow((size_t)n, "the depth fusion items")) return rc;
    if (const int rc = s->h_item.grow((size_t)n, "the depth fusion staging")) return rc;
    const size_t np = (size_t)(n * s->P);
    if (np > s->d_zbuf.capacity() || np > s->d_winner.capacity()) s->warp_clean = false;   // a new block is not all ones
    if (const int rc = s->d_zbuf.grow(np, "the warp's z-buffer")) return rc;
    if (const int rc = s->d_winner.grow(np, "the warp's z-buffer")) return rc;
#ifdef VG_DEPTH_WARP_STORE
    if (const int rc = s->d_src_target.grow(np, "the warp's source records")) return rc;
    if (const int rc = s->d_src_dist.grow(np, "the warp's source records")) return rc;
#endif
    for (int64_t k = 0; k < n; k++) {   // R^T and t in FP64
        vgd::WarpItem &it = s->h_item.get()[k];
        vgth::inverse_frame(xi12 + 6 * k, it.Rinv, it.t);
        for (int i = 0; i < 6; i++) it.counts[i] = 0;
    }
    if (!s->warp_clean) {   // the whole blocks: a later call of fewer items relies on it
        VG_HIP(hipMemsetAsync(s->d_zbuf, 0xff, s->d_zbuf.capacity() * sizeof(unsigned long long), s->stream));
        VG_HIP(hipMemsetAsync(s->d_winner, 0xff, s->d_winner.capacity() * sizeof(unsigned), s->stream));
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
    if (const int rc = call.finish()) return rc;
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
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    unsigned long long *dc = nullptr;
    if (const int rc = s->counters.begin(call, n, 5, counts, &dc)) return rc;
    hipLaunchKernelGGL(vgd::depth_merge_kernel, dim3(blocks_of(s->P, vgd::kLanes), (unsigned)n), dim3(vgd::kLanes), 0, s->stream, depth, sigma,
                       depth2, sigma2, s->P, dc);
    VG_HIP(hipGetLastError());
    return s->counters.end(call, n, 5, counts);
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
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (alias_d || alias_s)
        if (const int rc = s->d_copy.grow(2 * (size_t)(n * s->P), "the noise filter's copy")) return rc;
    if (alias_d) {   // the reference's myCopy
        VG_HIP(hipMemcpyAsync(s->d_copy, depth_in, bytes, hipMemcpyDeviceToDevice, s->stream));
        depth_in = s->d_copy;
    }
    if (alias_s) {
        VG_HIP(hipMemcpyAsync(s->d_copy.get() + n * s->P, sigma_in, bytes, hipMemcpyDeviceToDevice, s->stream));
        sigma_in = s->d_copy.get() + n * s->P;
    }
    unsigned long long *dc = nullptr;
    if (const int rc = s->counters.begin(call, n, 3, counts, &dc)) return rc;
    hipLaunchKernelGGL(vgd::depth_filter_noise_kernel, dim3(blocks_of(s->P, vgd::kLanes), (unsigned)n), dim3(vgd::kLanes), 0, s->stream, depth_in,
                       sigma_in, depth, sigma, s->g, s->P, dc);
    VG_HIP(hipGetLastError());
    return s->counters.end(call, n, 3, counts);
}

int vg_depth_regularize(vg_depth_fusion *s, int64_t n, int hyp_max, double *depth, double *sigma, double *cost)
{
    if (const int rc = check_call(s, n)) return rc;
    if (hyp_max < 1 || hyp_max > vgd::kMaxHyp) return fail(VG_ERR_INVALID_ARGUMENT, "hyp_max must be in [1, 8]");
    if (n == 0) return VG_OK;
    if (!depth || !sigma || !cost) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const void *const p[3] = {depth, sigma, cost};
    if (any_overlap(p, 3, (size_t)(n * hyp_max * s->P) * sizeof(double))) return fail(VG_ERR_INVALID_ARGUMENT, "the three maps must not overlap");
    if (hyp_max == 1) return VG_OK;   // one plane has nothing above it
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    hipLaunchKernelGGL(vgd::depth_regularize_kernel, dim3(blocks_of(s->P, vgd::kLanes), (unsigned)n), dim3(vgd::kLanes), 0, s->stream, depth, sigma,
                       cost, hyp_max, s->P);
    VG_HIP(hipGetLastError());
    return call.finish();
}

int vg_depth_pack_mh(vg_depth_fusion *s, int hyp_max, const double *depth, const double *sigma, int64_t *count, int32_t *indices, int32_t *hyp,
                     double *cloud, double *sigma_out)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "depth fusion handle is NULL");
    if (hyp_max < 1 || hyp_max > vgd::kMaxHyp) return fail(VG_ERR_INVALID_ARGUMENT, "hyp_max must be in [1, 8]");
    if (!depth || !count) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (sigma_out && !sigma) return fail(VG_ERR_INVALID_ARGUMENT, "sigma_out needs the sigma planes");
    const unsigned nb = blocks_of(s->P, vgd::kLanes);
    vgd::PackMhArgs a;
    for (int i = 0; i < 6; i++) a.cam[i] = s->cam[i];
    a.g = s->g;
    a.hyp_max = hyp_max;
    a.depth = depth;
    a.sigma = sigma;
    a.indices = indices;
    a.hyp = hyp;
    a.cloud = cloud;
    a.sigma_out = sigma_out;
    {   // the count: the entries of every block, scanned
        vgi::Call call(s);
        if (const int rc = call.begin()) return rc;
        if (const int rc = s->pack.grow(nb, 1, "the pack's block counts")) return rc;
        a.block_counts = s->pack.counts;
        a.block_offsets = s->pack.offsets;
        hipLaunchKernelGGL((vgd::depth_pack_mh_kernel<false>), dim3(nb), dim3(vgd::kLanes), 0, s->stream, a);
        s->pack.scan<vgd::kLanes>(s->stream, (int)nb, 0);
        VG_HIP(hipGetLastError());
        if (const int rc = s->pack.fetch(s->stream, 1)) return rc;
        if (const int rc = call.finish()) return rc;
    }
    *count = (int64_t)s->pack.h_totals.get()[0];
    if (*count == 0 || (!indices && !hyp && !cloud && !sigma_out)) return VG_OK;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    hipLaunchKernelGGL((vgd::depth_pack_mh_kernel<true>), dim3(nb), dim3(vgd::kLanes), 0, s->stream, a);
    VG_HIP(hipGetLastError());
    return call.finish();
}

int vg_transform_inverse(const double *xi, double *out6)
{
    if (!xi || !out6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    vgth::inverse(xi, out6);
    return VG_OK;
}

int vg_transform_inverse_compose(const double *a6, const double *b6, double *out6)
{
    if (!a6 || !b6 || !out6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    vgth::inverse_compose(a6, b6, out6);
    return VG_OK;
}

}  // extern "C"
