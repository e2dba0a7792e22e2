// vg_depth_tu.hip -- translation unit of libvisgeom_amd.so: depth map propagation and fusion (section 11 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_depth_fusion handle owns the scratch of its three operations: the warp's z-buffer and winner buffer (12 bytes per
// depth pixel and item, all ones between calls: the gather kernel restores what it read), the per-item poses with the warp's
// counters in one pinned and one device array, the counters of merge and the noise filter, and the copy the noise filter
// reads when it runs in place, the block counts of the multi-hypothesis pack, and of the point cloud (vg_depth_reconstruct) its
// block counts per item, the items' offsets and poses, and of vg_depth_compare the partial sums per workgroup.  Buffers only grow.
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
    int u_max = 0, v_max = 0;               // the image the grid samples: the truth of vg_depth_compare
    vgi::PackScratch recon;                 // of vg_depth_reconstruct: counts [item][block], one total per item
    vgi::Grow<unsigned> d_first;            // [n]: the entries of the items in front
    vgi::GrowPinned<unsigned> h_first;
    vgi::Grow<double> d_pose;               // [n][12]
    vgi::GrowPinned<double> h_pose;
    vgi::Grow<double> d_partial, d_sums;    // of vg_depth_compare: [n][blocks][6], [n][6]: three sums, three counts
    vgi::GrowPinned<double> h_sums;
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
    s->u_max = p.u_max;
    s->v_max = p.v_max;
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

int vg_depth_reconstruct(vg_depth_fusion *s, int64_t n, int hyp_max, uint32_t flags, const double *depth, const double *sigma, int64_t n_query,
                         const double *query_points, const int32_t *query_indices, const double *xi, int64_t *counts, const vg_recon_outputs *out)
{
    // what needs no handle is checked first, the handle next
    if (const int rc = vgi::check_items(n, 0, "item")) return rc;
    if (flags & VG_RECON_IMAGE_VALUES) return fail(VG_ERR_INVALID_ARGUMENT, "IMAGE_VALUES is not provided (the reference asserts on it)");
    constexpr uint32_t known = VG_RECON_QUERY_POINTS | VG_RECON_MINMAX | VG_RECON_ALL_HYPOTHESES | VG_RECON_DEFAULT_VALUES | VG_RECON_SIGMA_VALUE |
                               VG_RECON_QUERY_INDICES | VG_RECON_INDEX_MAPPING;
    if (flags & ~known) return fail(VG_ERR_INVALID_ARGUMENT, "unknown reconstruct flags");
    if (hyp_max < 1 || hyp_max > vgd::kMaxHyp) return fail(VG_ERR_INVALID_ARGUMENT, "hyp_max must be in [1, 8]");
    if (n > 0 && (!depth || !counts)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > 0 && (flags & (VG_RECON_SIGMA_VALUE | VG_RECON_MINMAX)) && !sigma) return fail(VG_ERR_INVALID_ARGUMENT, "SIGMA_VALUE and MINMAX need the sigma planes");
    const bool by_index = (flags & VG_RECON_QUERY_INDICES) != 0, by_point = !by_index && (flags & VG_RECON_QUERY_POINTS);
    if (by_index || by_point) {
        if (n_query < 0 || n_query >= (int64_t)1 << 31) return fail(VG_ERR_INVALID_ARGUMENT, "the query count must be in [0, 2^31)");
        if (n_query > 0 && !(by_index ? (const void *)query_indices : (const void *)query_points))
            return fail(VG_ERR_INVALID_ARGUMENT, "the query flag is set but its array is NULL");
    }
    const vg_recon_outputs none = {};
    const vg_recon_outputs &o = out ? *out : none;
    if (o.sigma_out && !(flags & VG_RECON_SIGMA_VALUE)) return fail(VG_ERR_INVALID_ARGUMENT, "sigma_out needs SIGMA_VALUE");
    if (o.index_map && !((flags & VG_RECON_INDEX_MAPPING) && (by_index || by_point)))
        return fail(VG_ERR_INVALID_ARGUMENT, "index_map needs INDEX_MAPPING and a query");
    if (xi && !vgsh::finite_n(xi, 6 * (int)n)) return fail(VG_ERR_INVALID_ARGUMENT, "the poses must be finite");
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "depth fusion handle is NULL");
    if (n == 0) return VG_OK;
    const int64_t units = (by_index || by_point) ? n_query : s->P;
    const int num_hyps = (flags & VG_RECON_ALL_HYPOTHESES) ? hyp_max : 1;
    if (n * units * num_hyps >= (int64_t)1 << 31) return fail(VG_ERR_INVALID_ARGUMENT, "the entries could reach 2^31: fewer items or queries per call");
    for (int64_t k = 0; k < n; k++) counts[k] = 0;
    if (units == 0) return VG_OK;
    const unsigned nb = blocks_of(units, vgd::kLanes);
    vgd::ReconArgs a = {};
    for (int i = 0; i < 6; i++) a.cam[i] = s->cam[i];
    a.g = s->g;
    a.P = s->P;
    a.units = units;
    a.hyp_max = hyp_max;
    a.num_hyps = num_hyps;
    a.flags = flags;
    a.depth = depth;
    a.sigma = sigma;
    a.query_idx = by_index ? query_indices : nullptr;
    a.query_pts = by_point ? query_points : nullptr;
    a.nb = (int)nb;
    const dim3 grid(nb, (unsigned)n), block(vgd::kLanes);
    {   // the count: the entries of every block, scanned per item
        vgi::Call call(s);
        if (const int rc = call.begin()) return rc;
        if (const int rc = s->recon.grow((size_t)n * nb, (size_t)n, "the reconstruct block counts")) return rc;
        a.block_counts = s->recon.counts;
        a.block_offsets = s->recon.offsets;
        hipLaunchKernelGGL((vgd::depth_reconstruct_kernel<false>), grid, block, 0, s->stream, a);
        hipLaunchKernelGGL(vgc::scan_block_counts_items_kernel<vgd::kLanes>, dim3((unsigned)n), block, 0, s->stream,
                           (const unsigned *)s->recon.counts.get(), s->recon.offsets.get(), (int)nb, s->recon.totals.get());
        VG_HIP(hipGetLastError());
        if (const int rc = s->recon.fetch(s->stream, (size_t)n)) return rc;
        if (const int rc = call.finish()) return rc;
    }
    int64_t total = 0;
    for (int64_t k = 0; k < n; k++) total += counts[k] = (int64_t)s->recon.h_totals.get()[k];
    if (total == 0 || !(o.indices || o.hyp || o.points || o.sigma_out || o.index_map || o.item || o.valid || o.cloud)) return VG_OK;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (n > 1) {
        if (const int rc = s->d_first.grow((size_t)n, "the reconstruct item offsets")) return rc;
        if (const int rc = s->h_first.grow((size_t)n, "the reconstruct item offsets")) return rc;
        unsigned run = 0;
        for (int64_t k = 0; k < n; k++) {
            s->h_first.get()[k] = run;
            run += (unsigned)counts[k];
        }
        VG_HIP(hipMemcpyAsync(s->d_first, s->h_first, (size_t)n * sizeof(unsigned), hipMemcpyHostToDevice, s->stream));
        a.item_first = s->d_first;
    }
    if (xi) {
        if (const int rc = s->d_pose.grow((size_t)n * 12, "the reconstruct poses")) return rc;
        if (const int rc = s->h_pose.grow((size_t)n * 12, "the reconstruct poses")) return rc;
        for (int64_t k = 0; k < n; k++) {
            double *p = s->h_pose.get() + 12 * k;
            vgth::rotation(xi + 6 * k, p);
            for (int i = 0; i < 3; i++) p[9 + i] = xi[6 * k + i];
        }
        VG_HIP(hipMemcpyAsync(s->d_pose, s->h_pose, (size_t)n * 12 * sizeof(double), hipMemcpyHostToDevice, s->stream));
        a.pose = s->d_pose;
    }
    a.indices = o.indices;
    a.hyp = o.hyp;
    a.index_map = o.index_map;
    a.item = o.item;
    a.points = o.points;
    a.sigma_out = o.sigma_out;
    a.cloud = o.cloud;
    a.valid = o.valid;
    hipLaunchKernelGGL((vgd::depth_reconstruct_kernel<true>), grid, block, 0, s->stream, a);
    VG_HIP(hipGetLastError());
    return call.finish();
}

int vg_depth_generate_plane(vg_depth_fusion *s, const double *xi_cam_plane, int k, const double *polygon, double *depth, double *sigma, double *cost)
{
    if (k < 3 || k > vgd::kMaxPolygon) return fail(VG_ERR_INVALID_ARGUMENT, "the polygon must have 3 to 16 vertices");
    if (!xi_cam_plane || !polygon || !depth || !sigma) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi_cam_plane, 6) || !vgsh::finite_n(polygon, 3 * k)) return fail(VG_ERR_INVALID_ARGUMENT, "the pose and the polygon must be finite");
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "depth fusion handle is NULL");
    const size_t bytes = (size_t)s->P * sizeof(double);
    const void *const p[3] = {depth, sigma, cost};
    if (any_overlap(p, cost ? 3 : 2, bytes)) return fail(VG_ERR_INVALID_ARGUMENT, "the outputs overlap each other");
    vgd::PlaneArgs a = {};
    double R[9];
    vgth::rotation(xi_cam_plane, R);
    for (int i = 0; i < 6; i++) a.cam[i] = s->cam[i];
    a.g = s->g;
    for (int i = 0; i < 3; i++) {
        a.t[i] = xi_cam_plane[i];
        a.z[i] = R[3 * i + 2];   // rotMat().col(2)
    }
    for (int j = 0; j < k; j++) {   // Transformation::transform
        double w[3];
        vgs::mat_vec(R, polygon + 3 * j, w);
        for (int i = 0; i < 3; i++) a.poly[j][i] = w[i] + xi_cam_plane[i];
    }
    a.k = k;
    a.depth = depth;
    a.sigma = sigma;
    a.cost = cost;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    hipLaunchKernelGGL(vgd::depth_generate_plane_kernel, dim3(blocks_of(s->P, vgd::kLanes)), dim3(vgd::kLanes), 0, s->stream, a);
    VG_HIP(hipGetLastError());
    return call.finish();
}

int vg_depth_compare(vg_depth_fusion *s, int64_t n, const double *depth, const double *sigma, const float *truth, double sigma_max, int64_t *counts,
                     double *sums, uint8_t *inliers)
{
    if (const int rc = check_call(s, n)) return rc;
    if (n == 0) return VG_OK;
    if (!depth || !sigma || !truth || !counts || !sums) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (std::isnan(sigma_max)) return fail(VG_ERR_INVALID_ARGUMENT, "sigma_max is NaN");
    const vgd::Grid &g = s->g;   // uConv / vConv of every map pixel must lie in the image the truth covers
    if (g.u0 < 0 || g.v0 < 0 || (int64_t)(g.x_max - 1) * g.scale + g.u0 >= s->u_max || (int64_t)(g.y_max - 1) * g.scale + g.v0 >= s->v_max)
        return fail(VG_ERR_INVALID_ARGUMENT, "the depth grid leaves the uMax x vMax image: no truth to compare with");
    const unsigned nb = blocks_of(s->P, vgd::kLanes);
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    constexpr int K = vgd::kCompareSums;
    if (const int rc = s->d_partial.grow((size_t)n * nb * K, "the comparison's partial sums")) return rc;
    if (const int rc = s->d_sums.grow((size_t)n * K, "the comparison's sums")) return rc;
    if (const int rc = s->h_sums.grow((size_t)n * K, "the comparison's sums")) return rc;
    vgd::CompareArgs a = {};
    a.g = g;
    a.u_max = s->u_max;
    a.v_max = s->v_max;
    a.P = s->P;
    a.nb = (int)nb;
    a.sigma_max = sigma_max;
    a.depth = depth;
    a.sigma = sigma;
    a.truth = truth;
    a.partial = s->d_partial;
    a.inliers = inliers;
    hipLaunchKernelGGL(vgd::depth_compare_kernel, dim3(nb, (unsigned)n), dim3(vgd::kLanes), 0, s->stream, a);
    hipLaunchKernelGGL(vgd::depth_compare_sum_kernel, dim3((unsigned)n), dim3(vgd::kLanes), 0, s->stream, (const double *)s->d_partial.get(), (int)nb,
                       s->d_sums.get());
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(s->h_sums, s->d_sums, (size_t)n * K * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (const int rc = call.finish()) return rc;
    for (int64_t k = 0; k < n; k++)
        for (int i = 0; i < 3; i++) {
            sums[3 * k + i] = s->h_sums.get()[K * k + i];
            counts[3 * k + i] = (int64_t)s->h_sums.get()[K * k + 3 + i];   // whole numbers below 2^28: exact
        }
    return VG_OK;
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
