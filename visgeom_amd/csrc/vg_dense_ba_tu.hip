// vg_dense_ba_tu.hip -- translation unit of libvisgeom_amd.so: photometric bundle adjustment (section 18 of the C ABI).  Built
// with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_dense_ba handle owns the key frame's float image and maps, the pack, the frames' float images, and two slots of
// evaluation state (depths, row buffers, a, g_d, the per-frame sums): the current point and the candidate.  solve drives the
// trust-region loop from the host (vg_lmn.hpp): per iteration one reduce under mu = 1 / radius (the rows of the current slot
// are read again when a refused step changes mu), a K x K Cholesky on the host, the back-substitution into the other slot and
// one evaluation there.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>

#include "vg_dense_ba.hpp"
#include "vg_handle.hpp"
#include "vg_lmn.hpp"
#include "vg_local.hpp"
#include "vg_stereo_host.hpp"
#include "vg_pose_host.hpp"

struct vg_dense_ba : vgi::HandleBase {
    double cam[6], xbc[6], Rb[9];
    vgba::Grid g;
    int w = 0, h = 0, F = 0;
    double sigma_grey = 0., lambda = 0., grad_thresh = 0.;
    vglmn::Rule rule{};
    bool has_base = false, evaluated = false;
    int64_t m = 0;
    int cur = 0;   // the slot of the current point
    vgi::Grow<float> d_base, d_imgs;                    // [h][w]; [F][h][w]
    vgi::Grow<double> d_depth_map, d_sigma_map;         // [y_max][x_max]
    vgi::Grow<int32_t> d_idx;                           // the pack, room for every cell
    vgi::Grow<double> d_val, d_dir, d_d0, d_s0;
    vgi::PackScratch pack;                              // blocks of the grid; one total
    vgi::Grow<vgba::Frame> d_frames;
    vgi::GrowPinned<vgba::Frame> h_frames;
    // per slot: depth [m] | a [m] | gd [m] | res [F][m] | jd [F][m] | jp [F][m][6]; sums [F][28] + the prior's cost
    vgi::Grow<double> d_slot[2], d_sums[2];
    vgi::GrowPinned<double> h_sums[2];
    vgi::Grow<double> d_partials, d_prior_partials;     // [F][blocks][28]; [blocks]
    vgi::Grow<double> d_tiles, d_S, d_tail_partials, d_tail;
    vgi::GrowPinned<double> h_S, h_tail;                // [K][K] | [K]; [5]
};

namespace {

using vgi::fail;
using vgsh::blocks_of;

struct Slot {
    double *depth, *a, *gd, *res, *jd, *jp;
};

Slot slot_of(const vg_dense_ba *s, int which)
{
    double *p = s->d_slot[which].get();
    const int64_t m = s->m, F = s->F;
    return Slot{p, p + m, p + 2 * m, p + 3 * m, p + (3 + F) * m, p + (3 + 2 * F) * m};
}

int64_t cells(const vg_dense_ba *s) { return (int64_t)s->g.x_max * s->g.y_max; }

// the buffers whose size depends on the pack and the frame count
int ensure_rows(vg_dense_ba *s)
{
    if (!s->has_base || s->F == 0 || s->m == 0) return VG_OK;
    const size_t m = (size_t)s->m, F = (size_t)s->F, blocks = blocks_of(s->m, vgba::kLanes);
    const char *what = "the bundle adjustment's rows";
    for (int k = 0; k < 2; k++) {
        if (const int rc = s->d_slot[k].grow((3 + 8 * F) * m, what)) return rc;
        if (const int rc = s->d_sums[k].grow(F * vgba::kSums + 1, what)) return rc;
        if (const int rc = s->h_sums[k].grow(F * vgba::kSums + 1, "the bundle adjustment's staging")) return rc;
    }
    if (const int rc = s->d_frames.grow(F, what)) return rc;
    if (const int rc = s->h_frames.grow(F, "the bundle adjustment's staging")) return rc;
    if (const int rc = s->d_partials.grow(F * blocks * vgba::kSums, what)) return rc;
    if (const int rc = s->d_prior_partials.grow(blocks, what)) return rc;
    // the reduce: at most kSchurBlocks workgroups of four waves, ten tiles of 256 doubles each
    if (const int rc = s->d_tiles.grow((size_t)vgba::kSchurBlocks * vgba::kWaves * 10 * 256, what)) return rc;
    if (const int rc = s->d_S.grow(49 * 48, what)) return rc;
    if (const int rc = s->h_S.grow(49 * 48, "the bundle adjustment's staging")) return rc;
    if (const int rc = s->d_tail_partials.grow(blocks * vgba::kTail, what)) return rc;
    if (const int rc = s->d_tail.grow(vgba::kTail, what)) return rc;
    return s->h_tail.grow(vgba::kTail, "the bundle adjustment's staging");
}

void make_frame(const vg_dense_ba *s, const double *xi, vgba::Frame &f)
{
    double c[6];
    vgth::compose(xi, s->xbc, c);
    vgth::inverse_frame(c, f.Rinv, f.t);
    vg::mat3_mul(f.Rinv, s->Rb, f.M);
    vg::camera_jacobian_frame(xi, s->xbc, f.L11, f.L12, f.L22);
}

// rows, a, g_d and the sums of slot `which` at the poses xi and the slot's depths; the sums to h_sums[which].  Enqueues and
// synchronises.
int run_evaluate(vg_dense_ba *s, int which, const double *xi)
{
    const int F = s->F;
    const unsigned blocks = blocks_of(s->m, vgba::kLanes);
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    for (int f = 0; f < F; f++) make_frame(s, xi + 6 * f, s->h_frames.get()[f]);
    VG_HIP(hipMemcpyAsync(s->d_frames, s->h_frames, (size_t)F * sizeof(vgba::Frame), hipMemcpyHostToDevice, s->stream));
    const Slot sl = slot_of(s, which);
    vgba::EvalArgs a;
    a.frames = s->d_frames;
    a.imgs = s->d_imgs;
    a.w = s->w;
    a.h = s->h;
    for (int i = 0; i < 6; i++) a.cam[i] = s->cam[i];
    for (int i = 0; i < 9; i++) a.Rb[i] = s->Rb[i];
    for (int i = 0; i < 3; i++) a.tb[i] = s->xbc[i];
    a.sigma_grey = s->sigma_grey;
    a.val = s->d_val;
    a.dir = s->d_dir;
    a.depth = sl.depth;
    a.m = (int)s->m;
    a.blocks = (int)blocks;
    a.res = sl.res;
    a.jp = sl.jp;
    a.jd = sl.jd;
    a.partials = s->d_partials;
    hipLaunchKernelGGL(vgba::ba_eval_kernel, dim3(blocks, (unsigned)F), dim3(vgba::kLanes), 0, s->stream, a);
    vgba::PointArgs p;
    p.F = F;
    p.m = (int)s->m;
    p.blocks = (int)blocks;
    p.lambda = s->lambda;
    p.res = sl.res;
    p.jd = sl.jd;
    p.depth = sl.depth;
    p.d0 = s->d_d0;
    p.s0 = s->d_s0;
    p.a = sl.a;
    p.gd = sl.gd;
    p.prior_partials = s->d_prior_partials;
    hipLaunchKernelGGL(vgba::ba_point_kernel, dim3(blocks), dim3(vgba::kLanes), 0, s->stream, p);
    hipLaunchKernelGGL(vgba::ba_sums_kernel, dim3((unsigned)(F * vgba::kSums + 1)), dim3(64), 0, s->stream, (const double *)s->d_partials.get(),
                       (const double *)s->d_prior_partials.get(), F, (int)blocks, s->d_sums[which].get());
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(s->h_sums[which], s->d_sums[which], ((size_t)F * vgba::kSums + 1) * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    return call.finish();
}

// the frames' costs in order, then the prior's
double total_cost(const vg_dense_ba *s, int which)
{
    const double *G = s->h_sums[which].get();
    double c = 0.;
    for (int f = 0; f < s->F; f++) c += G[f * vgba::kSums + 27];
    return c + G[s->F * vgba::kSums];
}

template <int TA, int TB>
void launch_schur(const vg_dense_ba *s, const vgba::SchurArgs &a, unsigned blocks)
{
    hipLaunchKernelGGL((vgba::ba_schur_kernel<TA, TB>), dim3(blocks), dim3(vgba::kLanes), 0, s->stream, a);
    hipLaunchKernelGGL(vgba::ba_schur_final_kernel, dim3((unsigned)a.K), dim3(64, vgba::kFinalRuns), 0, s->stream, a, TB, vgba::tile_count(TA, TB));
}

// S | rhs of slot `which` under mu to h_S.  Enqueues and synchronises.
int run_reduce(vg_dense_ba *s, int which, double mu)
{
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    const Slot sl = slot_of(s, which);
    const int K = 6 * s->F;
    vgba::SchurArgs a;
    a.F = s->F;
    a.K = K;
    a.m = (int)s->m;
    // a workgroup of four waves takes 256 C points, C the smallest that keeps the workgroups at kSchurBlocks or fewer
    const int64_t C = (s->m + (int64_t)vgba::kSchurBlocks * vgba::kLanes - 1) / ((int64_t)vgba::kSchurBlocks * vgba::kLanes);
    a.run = (int)(64 * C);
    const unsigned blocks = blocks_of(s->m, (int)(vgba::kLanes * C));
    a.mu = mu;
    a.dmin = s->rule.dmin;
    a.dmax = s->rule.dmax;
    a.jp = sl.jp;
    a.jd = sl.jd;
    a.a = sl.a;
    a.gd = sl.gd;
    a.tiles = s->d_tiles;
    a.waves = (int)blocks * vgba::kWaves;
    a.sums = s->d_sums[which];
    a.S = s->d_S;
    a.rhs = s->d_S.get() + K * K;
    // by the tiles of 16 that K and K + 1 fill
    if (K + 1 <= 16) launch_schur<1, 1>(s, a, blocks);
    else if (K + 1 <= 32) launch_schur<2, 2>(s, a, blocks);
    else if (K + 1 <= 48) launch_schur<3, 3>(s, a, blocks);
    else launch_schur<3, 4>(s, a, blocks);
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(s->h_S, s->d_S, (size_t)(K * K + K) * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    return call.finish();
}

// the candidate depths of slot `which` under (mu, dp) into `cand` (DEVICE [m]) and the tail sums to h_tail
int run_backsub(vg_dense_ba *s, int which, double mu, const double *dp, double *cand)
{
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    const Slot sl = slot_of(s, which);
    const unsigned blocks = blocks_of(s->m, vgba::kLanes);
    vgba::BacksubArgs a;
    a.F = s->F;
    a.m = (int)s->m;
    a.blocks = (int)blocks;
    a.mu = mu;
    a.dmin = s->rule.dmin;
    a.dmax = s->rule.dmax;
    for (int k = 0; k < 6 * vgba::kMaxFrames; k++) a.dp[k] = k < 6 * s->F ? dp[k] : 0.;
    a.jp = sl.jp;
    a.jd = sl.jd;
    a.a = sl.a;
    a.gd = sl.gd;
    a.depth = sl.depth;
    a.cand = cand;
    a.partials = s->d_tail_partials;
    hipLaunchKernelGGL(vgba::ba_backsub_kernel, dim3(blocks), dim3(vgba::kLanes), 0, s->stream, a);
    hipLaunchKernelGGL(vgba::ba_tail_kernel, dim3(vgba::kTail), dim3(64), 0, s->stream, (const double *)s->d_tail_partials.get(), (int)blocks, s->d_tail.get());
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(s->h_tail, s->d_tail, vgba::kTail * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    return call.finish();
}

int check_ready(const vg_dense_ba *s)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "dense_ba handle is NULL");
    if (!s->has_base) return fail(VG_ERR_STATE, "no key frame: call vg_dense_ba_set_base first");
    if (s->F == 0) return fail(VG_ERR_STATE, "no frames: call vg_dense_ba_set_frames first");
    return VG_OK;
}

}  // namespace

extern "C" {

int vg_dense_ba_create(vg_dense_ba **out, int device, void *hip_stream, const double *eucm, const vg_stereo_params *params,
                       const double *xi_base_cam, int width, int height, const vg_dense_ba_options *options)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (!eucm || !params || !xi_base_cam) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const vg_stereo_params &p = *params;   // only the ScaleParameters fields are read; the image size is an argument
    int x_max = 0, y_max = 0;
    if (const int rc = vgsh::scaled_grid(p, false, x_max, y_max)) return rc;
    if (width < 1 || width > 16384 || height < 1 || height > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "the image size must be in [1, 16384]");
    if (!vgsh::finite_n(xi_base_cam, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "xi_base_cam must be finite");
    if (const int rc = vgsh::check_camera(eucm)) return rc;
    vg_dense_ba_options o = {0., 0., 0., 0, 0.};
    if (options) o = *options;
    if (!(o.sigma_grey >= 0.) || !std::isfinite(o.sigma_grey)) return fail(VG_ERR_INVALID_ARGUMENT, "sigma_grey must be finite and not negative");
    if (!std::isfinite(o.prior_weight) || !std::isfinite(o.grad_thresh)) return fail(VG_ERR_INVALID_ARGUMENT, "prior_weight and grad_thresh must be finite");
    if (o.max_iterations < 0 || !(o.function_tolerance >= 0.) || !std::isfinite(o.function_tolerance))
        return fail(VG_ERR_INVALID_ARGUMENT, "max_iterations and function_tolerance must not be negative");
    std::unique_ptr<vg_dense_ba> s(new (std::nothrow) vg_dense_ba());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    for (int i = 0; i < 6; i++) {
        s->cam[i] = eucm[i];
        s->xbc[i] = xi_base_cam[i];
    }
    vgth::rotation(s->xbc, s->Rb);
    s->g = vgba::Grid{p.scale, p.u0, p.v0, x_max, y_max};
    s->w = width;
    s->h = height;
    s->sigma_grey = o.sigma_grey == 0. ? VG_DENSE_BA_SIGMA_GREY : o.sigma_grey;
    s->lambda = o.prior_weight == 0. ? VG_DENSE_BA_PRIOR_WEIGHT : (o.prior_weight < 0. ? 0. : o.prior_weight);
    s->grad_thresh = o.grad_thresh == 0. ? VG_DENSE_BA_GRAD_THRESH : (o.grad_thresh < 0. ? 0. : o.grad_thresh);
    s->rule = vglm6::ceres_defaults(o.max_iterations == 0 ? VG_DENSE_BA_MAX_ITERATIONS : o.max_iterations);
    s->rule.ftol = o.function_tolerance == 0. ? VG_DENSE_BA_FUNCTION_TOLERANCE : o.function_tolerance;
    if (const int rc = s->open(device, hip_stream, "photometric bundle adjustment")) return rc;
    *out = s.release();
    return VG_OK;
}

void vg_dense_ba_destroy(vg_dense_ba *s) { vgi::destroy(s); }

int vg_dense_ba_set_base(vg_dense_ba *s, const uint8_t *img, const double *depth, const double *sigma)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "dense_ba handle is NULL");
    if (!img || !depth) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!sigma && s->lambda > 0.) return fail(VG_ERR_INVALID_ARGUMENT, "the depth prior needs a sigma map");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    s->has_base = s->evaluated = false;
    const int64_t P = (int64_t)s->w * s->h, n = cells(s);
    const unsigned nb = blocks_of(n, vgba::kLanes);
    const char *what = "the key frame and its pack";
    if (const int rc = s->d_base.grow((size_t)P, what)) return rc;
    if (const int rc = s->d_depth_map.grow((size_t)n, what)) return rc;
    if (const int rc = s->d_sigma_map.grow((size_t)n, what)) return rc;
    if (const int rc = s->d_idx.grow((size_t)n, what)) return rc;
    if (const int rc = s->d_val.grow((size_t)n, what)) return rc;
    if (const int rc = s->d_dir.grow((size_t)(3 * n), what)) return rc;
    if (const int rc = s->d_d0.grow((size_t)n, what)) return rc;
    if (const int rc = s->d_s0.grow((size_t)n, what)) return rc;
    if (const int rc = s->pack.grow(nb, 1, what)) return rc;
    VG_HIP(hipMemcpyAsync(s->d_depth_map, depth, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (sigma) VG_HIP(hipMemcpyAsync(s->d_sigma_map, sigma, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    else VG_HIP(hipMemsetAsync(s->d_sigma_map, 0, (size_t)n * sizeof(double), s->stream));
    hipLaunchKernelGGL(vgs::u8_to_float_kernel<vgba::kLanes>, dim3(blocks_of(P, vgba::kLanes), 1), dim3(vgba::kLanes), 0, s->stream, img, s->d_base.get(), P, P);
    vgba::SelectArgs a;
    a.img = s->d_base;
    a.w = s->w;
    a.h = s->h;
    for (int i = 0; i < 6; i++) a.cam[i] = s->cam[i];
    a.g = s->g;
    a.depth = s->d_depth_map;
    a.sigma = s->d_sigma_map;
    a.grad_thresh = s->grad_thresh;
    a.need_sigma = s->lambda > 0. ? 1 : 0;
    a.block_counts = s->pack.counts;
    a.block_offsets = s->pack.offsets;
    a.idx = s->d_idx;
    a.val = s->d_val;
    a.dir = s->d_dir;
    a.d0 = s->d_d0;
    a.s0 = s->d_s0;
    hipLaunchKernelGGL((vgba::ba_select_kernel<false>), dim3(nb), dim3(vgba::kLanes), 0, s->stream, a);
    s->pack.scan<vgba::kLanes>(s->stream, (int)nb, 0);
    hipLaunchKernelGGL((vgba::ba_select_kernel<true>), dim3(nb), dim3(vgba::kLanes), 0, s->stream, a);
    VG_HIP(hipGetLastError());
    if (const int rc = s->pack.fetch(s->stream, 1)) return rc;
    if (const int rc = call.finish()) return rc;
    s->m = s->pack.h_totals.get()[0];
    s->has_base = true;
    return ensure_rows(s);
}

int vg_dense_ba_set_frames(vg_dense_ba *s, int frames, const uint8_t *imgs)
{
    if (frames < 1 || frames > VG_DENSE_BA_MAX_FRAMES) return fail(VG_ERR_INVALID_ARGUMENT, "the frame count must be in [1, 8]");
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "dense_ba handle is NULL");
    if (!imgs) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    s->F = 0;
    s->evaluated = false;
    const int64_t P = (int64_t)s->w * s->h;
    if (const int rc = s->d_imgs.grow((size_t)(frames * P), "the frames")) return rc;
    hipLaunchKernelGGL(vgs::u8_to_float_kernel<vgba::kLanes>, dim3(blocks_of(P, vgba::kLanes), (unsigned)frames), dim3(vgba::kLanes), 0, s->stream, imgs,
                       s->d_imgs.get(), P, P);
    VG_HIP(hipGetLastError());
    if (const int rc = call.finish()) return rc;
    s->F = frames;
    return ensure_rows(s);
}

int vg_dense_ba_pack(vg_dense_ba *s, int64_t *count, int32_t *indices, double *greys, double *dirs, double *d0, double *sigma0)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "dense_ba handle is NULL");
    if (!s->has_base) return fail(VG_ERR_STATE, "no key frame: call vg_dense_ba_set_base first");
    const int64_t m = s->m;
    if (count) *count = m;
    if (m == 0 || (!indices && !greys && !dirs && !d0 && !sigma0)) return VG_OK;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (indices) VG_HIP(hipMemcpyAsync(indices, s->d_idx.get(), (size_t)m * sizeof(int32_t), hipMemcpyDeviceToDevice, s->stream));
    if (greys) VG_HIP(hipMemcpyAsync(greys, s->d_val.get(), (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (dirs) VG_HIP(hipMemcpyAsync(dirs, s->d_dir.get(), (size_t)(3 * m) * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (d0) VG_HIP(hipMemcpyAsync(d0, s->d_d0.get(), (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (sigma0) VG_HIP(hipMemcpyAsync(sigma0, s->d_s0.get(), (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    return call.finish();
}

int vg_dense_ba_evaluate(vg_dense_ba *s, const double *xi, const double *depths, double *residuals, double *jac_pose, double *jac_depth,
                         double *a, double *g_depth, double *cost, double *sums)
{
    if (const int rc = check_ready(s)) return rc;
    if (!xi) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi, 6 * s->F)) return fail(VG_ERR_INVALID_ARGUMENT, "the poses must be finite");
    if (s->m == 0) return fail(VG_ERR_INVALID_ARGUMENT, "the pack is empty");
    const size_t m = (size_t)s->m, F = (size_t)s->F;
    s->evaluated = false;
    s->cur = 0;
    const Slot sl = slot_of(s, 0);
    {
        vgi::Call call(s);
        if (const int rc = call.begin()) return rc;
        VG_HIP(hipMemcpyAsync(sl.depth, depths ? depths : s->d_d0.get(), m * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        if (const int rc = call.finish()) return rc;
    }
    if (const int rc = run_evaluate(s, 0, xi)) return rc;
    s->evaluated = true;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (residuals) VG_HIP(hipMemcpyAsync(residuals, sl.res, F * m * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (jac_pose) VG_HIP(hipMemcpyAsync(jac_pose, sl.jp, 6 * F * m * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (jac_depth) VG_HIP(hipMemcpyAsync(jac_depth, sl.jd, F * m * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (a) VG_HIP(hipMemcpyAsync(a, sl.a, m * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (g_depth) VG_HIP(hipMemcpyAsync(g_depth, sl.gd, m * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (const int rc = call.finish()) return rc;
    if (cost) *cost = total_cost(s, 0);
    if (sums) std::memcpy(sums, s->h_sums[0].get(), F * vgba::kSums * sizeof(double));
    return VG_OK;
}

int vg_dense_ba_reduce(vg_dense_ba *s, double mu, double *S, double *rhs)
{
    if (const int rc = check_ready(s)) return rc;
    if (!(mu > 0.) || !std::isfinite(mu)) return fail(VG_ERR_INVALID_ARGUMENT, "mu must be positive and finite");
    if (!s->evaluated) return fail(VG_ERR_STATE, "no rows: call vg_dense_ba_evaluate first");
    if (const int rc = run_reduce(s, s->cur, mu)) return rc;
    const int K = 6 * s->F;
    if (S) std::memcpy(S, s->h_S.get(), (size_t)(K * K) * sizeof(double));
    if (rhs) std::memcpy(rhs, s->h_S.get() + K * K, (size_t)K * sizeof(double));
    return VG_OK;
}

int vg_dense_ba_back_substitute(vg_dense_ba *s, double mu, const double *dp, double *candidate, double *tail)
{
    if (const int rc = check_ready(s)) return rc;
    if (!dp) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!(mu > 0.) || !std::isfinite(mu)) return fail(VG_ERR_INVALID_ARGUMENT, "mu must be positive and finite");
    if (!vgsh::finite_n(dp, 6 * s->F)) return fail(VG_ERR_INVALID_ARGUMENT, "the pose step must be finite");
    if (!s->evaluated) return fail(VG_ERR_STATE, "no rows: call vg_dense_ba_evaluate first");
    const Slot other = slot_of(s, 1 - s->cur);
    if (const int rc = run_backsub(s, s->cur, mu, dp, other.depth)) return rc;
    if (candidate) {
        vgi::Call call(s);
        if (const int rc = call.begin()) return rc;
        VG_HIP(hipMemcpyAsync(candidate, other.depth, (size_t)s->m * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        if (const int rc = call.finish()) return rc;
    }
    if (tail) std::memcpy(tail, s->h_tail.get(), vgba::kTail * sizeof(double));
    return VG_OK;
}

int vg_dense_ba_solve(vg_dense_ba *s, const double *xi_start, double *xi_out, double *depth_out, double *sigma_out, double *report)
{
    if (const int rc = check_ready(s)) return rc;
    if (!xi_start || !xi_out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi_start, 6 * s->F)) return fail(VG_ERR_INVALID_ARGUMENT, "the poses must be finite");
    if (s->m == 0) return fail(VG_ERR_INVALID_ARGUMENT, "the pack is empty");
    const int K = 6 * s->F;
    double x[vglmn::kMaxDense], xc[vglmn::kMaxDense], g[vglmn::kMaxDense], D[vglmn::kMaxDense];
    std::memcpy(x, xi_start, sizeof(double) * K);
    if (const int rc = vg_dense_ba_evaluate(s, x, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
    vglmn::State st;
    vglmn::start(s->rule, st, total_cost(s, s->cur));
    const double initial_cost = st.cost;
    while (!st.done) {
        vglmn::Step step;
        const double mu = 1. / st.radius;
        if (const int rc = run_reduce(s, s->cur, mu)) return rc;
        vglmn::dense_step(K, s->h_S.get(), s->h_S.get() + K * K, mu, step);
        const double *G = s->h_sums[s->cur].get();
        for (int k = 0; k < K; k++) {
            const double *Gf = G + (k / 6) * vgba::kSums;
            const int c = k % 6;
            g[k] = Gf[21 + c];
            D[k] = vglmn::clamp_diag(s->rule, Gf[c * 6 - c * (c - 1) / 2]);
        }
        vglmn::head_sums(K, x, g, D, step, xc);
        double cost_c = 0.;
        if (step.ok) {
            if (const int rc = run_backsub(s, s->cur, mu, step.dx, slot_of(s, 1 - s->cur).depth)) return rc;
            vglmn::add_tail(step, s->h_tail.get());
        }
        if (step.ok) {
            if (const int rc = run_evaluate(s, 1 - s->cur, xc)) return rc;
            cost_c = total_cost(s, 1 - s->cur);
        }
        if (vglmn::accept(s->rule, st, step, cost_c)) {
            std::memcpy(x, xc, sizeof(double) * K);
            s->cur = 1 - s->cur;
        }
    }
    std::memcpy(xi_out, x, sizeof(double) * K);
    if (depth_out || sigma_out) {
        vgi::Call call(s);
        if (const int rc = call.begin()) return rc;
        const size_t bytes = (size_t)cells(s) * sizeof(double);
        if (depth_out) VG_HIP(hipMemcpyAsync(depth_out, s->d_depth_map.get(), bytes, hipMemcpyDeviceToDevice, s->stream));
        if (sigma_out) VG_HIP(hipMemcpyAsync(sigma_out, s->d_sigma_map.get(), bytes, hipMemcpyDeviceToDevice, s->stream));
        const Slot sl = slot_of(s, s->cur);
        hipLaunchKernelGGL(vgba::ba_scatter_kernel, dim3(blocks_of(s->m, vgba::kLanes)), dim3(vgba::kLanes), 0, s->stream, (const int32_t *)s->d_idx.get(),
                           (const double *)sl.depth, (const double *)sl.a, (int)s->m, depth_out, sigma_out);
        VG_HIP(hipGetLastError());
        if (const int rc = call.finish()) return rc;
    }
    if (report) {
        report[0] = st.iterations;
        report[1] = initial_cost;
        report[2] = st.cost;
        report[3] = st.term;
    }
    return VG_OK;
}

}  // extern "C"
