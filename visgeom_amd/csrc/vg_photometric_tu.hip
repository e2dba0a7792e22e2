// vg_photometric_tu.hip -- translation unit of libvisgeom_amd.so: photometric pose estimation against a depth key frame
// (section 12 of the C ABI).  Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not
// rebuild the others.
//
// A vg_photometric handle owns the base pyramid with its gradients, the data pack of every scale (built once per key frame),
// the target pyramids, and the staging of a cost evaluation: the per-pose frames and the 28 sums per pose in pinned memory.
// compute_pose drives the trust-region loop from the host: per iteration one upload of the candidate frames, the cost and the
// reduce launch over all poses that still move, and one download of 28 doubles per pose.
// evaluate_mi / compute_pose_mi are the mutual-information cost and its quasi-Newton solve on the same handle: four launches per
// evaluation and one download of 72 doubles per pose (vg_photometric_mi.hpp).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "vg_handle.hpp"
#include "vg_lm6.hpp"
#include "vg_local.hpp"
#include "vg_motion_prior.hpp"
#include "vg_photometric.hpp"
#include "vg_photometric_mi.hpp"
#include "vg_stereo_host.hpp"
#include "vg_pose_host.hpp"

struct vg_photometric : vgi::HandleBase {
    double cam[6], xbc[6];
    vgp::Grid g;
    int levels = 0, w[vgp::kMaxLevels], h[vgp::kMaxLevels];
    int64_t off[vgp::kMaxLevels + 1];   // pixel offset of a level inside one pyramid; off[levels] = pixels of a pyramid
    bool has_base = false;
    int64_t n_targets = 0;
    int64_t m[vgp::kMaxLevels];         // points of the pack per scale
    vgi::Grow<float> d_base, d_targets, d_grad;   // [3][total]: img | gu | gv; [n][total]; [2][level 0] for vg_photometric_level
    vgi::Grow<int32_t> d_idx;                     // the packs: level i at off[i], room for every pixel
    vgi::Grow<double> d_val, d_cloud;
    vgi::PackScratch pack;                        // blocks of level 0; one total per level
    vgi::Grow<vgp::PoseFrame> d_frames;
    vgi::GrowPinned<vgp::PoseFrame> h_frames;
    vgi::Grow<double> d_partials, d_sums;         // [n][blocks][kSums]; [n][kSums]
    vgi::GrowPinned<double> h_sums;
    // the mutual-information cost: _hist1 per scale, and the staging of an evaluation
    vgi::Grow<double> d_hist1, d_hist1_partials;   // [kMaxLevels][8]; [workgroups of level 0][8]
    vgi::Grow<double> d_mi_hist, d_mi_grad, d_mi_log, d_mi_out;   // [n][blocks][64], [n][blocks][6], [n][64], [n][kMiOut]
    vgi::GrowPinned<double> h_mi_out;
};

namespace {

using vgi::fail;
using vgsh::blocks_of;
constexpr int kMaxIterations = 150;    // photometric.cpp:150
// Ceres' defaults, which the reference leaves in place (photometric.cpp:148-150), under the rule of vg_lm6.hpp
constexpr vglm6::Rule kRule = vglm6::ceres_defaults(kMaxIterations);

int64_t level_pixels(const vg_photometric *s, int i) { return (int64_t)s->w[i] * s->h[i]; }

// the frame of pose xi: xiCam = xi o xi_base_cam for the points, CameraJacobian(camera, xi, xi_base_cam) for the rows
void make_frame(const vg_photometric *s, const double *xi, int target, bool active, vgp::PoseFrame &f)
{
    double c[6];
    vgth::compose(xi, s->xbc, c);
    vgth::inverse_frame(c, f.Rinv, f.t);
    vg::camera_jacobian_frame(xi, s->xbc, f.L11, f.L12, f.L22);
    f.target = target;
    f.active = active ? 1 : 0;
}

int ensure_poses(vg_photometric *s, int64_t n)
{
    if (const int rc = s->d_frames.grow((size_t)n, "the photometric poses")) return rc;
    if (const int rc = s->d_sums.grow((size_t)n * vgp::kSums, "the photometric poses")) return rc;
    if (const int rc = s->h_frames.grow((size_t)n, "the photometric staging")) return rc;
    return s->h_sums.grow((size_t)n * vgp::kSums, "the photometric staging");
}

// the cost of the n frames in h_frames at one scale: residuals / rows to res / jac (DEVICE, may be NULL), the 28 sums per
// active pose to h_sums when `sums`.  Synchronous.
int run_cost(vg_photometric *s, int scale, int64_t n, double *res, double *jac, bool sums)
{
    const int64_t m = s->m[scale];
    if (m == 0) {
        if (sums) std::memset(s->h_sums.get(), 0, (size_t)n * vgp::kSums * sizeof(double));
        return VG_OK;
    }
    const unsigned blocks = blocks_of(m, vgp::kLanes);
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (sums)
        if (const int rc = s->d_partials.grow((size_t)(n * blocks) * vgp::kSums, "the photometric partial sums")) return rc;
    VG_HIP(hipMemcpyAsync(s->d_frames, s->h_frames, (size_t)n * sizeof(vgp::PoseFrame), hipMemcpyHostToDevice, s->stream));
    vgp::EvalArgs a;
    a.frames = s->d_frames;
    a.targets = s->d_targets;
    a.target_stride = s->off[s->levels];
    a.level_off = s->off[scale];
    a.w = s->w[scale];
    a.h = s->h[scale];
    const double level_scale = (double)(1 << scale);
    a.inv_scale = 1. / level_scale;
    a.margin = vgp::kMarginPixels / level_scale;
    for (int i = 0; i < 6; i++) a.cam[i] = s->cam[i];
    a.val = s->d_val.get() + s->off[scale];
    a.cloud = s->d_cloud.get() + 3 * s->off[scale];
    a.m = (int)m;
    a.blocks = (int)blocks;
    a.res = res;
    a.jac = jac;
    a.partials = sums ? s->d_partials.get() : nullptr;
    hipLaunchKernelGGL(vgp::photo_eval_kernel, dim3(blocks, (unsigned)n), dim3(vgp::kLanes), 0, s->stream, a);
    if (sums) {
        hipLaunchKernelGGL(vgp::photo_reduce_kernel, dim3((unsigned)n), dim3(64), 0, s->stream, (const vgp::PoseFrame *)s->d_frames.get(),
                           (const double *)s->d_partials.get(), (int)blocks, s->d_sums.get());
        VG_HIP(hipGetLastError());
        VG_HIP(hipMemcpyAsync(s->h_sums, s->d_sums, (size_t)n * vgp::kSums * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    } else {
        VG_HIP(hipGetLastError());
    }
    return call.finish();
}

int check_poses(const vg_photometric *s, int64_t n, const double *xi, const int32_t *target)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "photometric handle is NULL");
    if (!s->has_base) return fail(VG_ERR_INVALID_ARGUMENT, "no key frame: call vg_photometric_set_base first");
    if (s->n_targets == 0) return fail(VG_ERR_INVALID_ARGUMENT, "no target image: call vg_photometric_set_targets first");
    if (const int rc = vgi::check_items(n, 1, "pose")) return rc;
    if (!xi || !target) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi, 6 * (int)n)) return fail(VG_ERR_INVALID_ARGUMENT, "the poses must be finite");
    for (int64_t k = 0; k < n; k++)
        if (target[k] < 0 || target[k] >= s->n_targets) return fail(VG_ERR_INVALID_ARGUMENT, "target index out of range");
    return VG_OK;
}

// OdometryPrior(0.03, 0.03, 0.01, 0.01, xiOdom) of computePose (photometric.cpp:143), from the shared vg_motion_prior.hpp
using vgmp::add_prior;
using vgmp::MotionPrior;
MotionPrior make_prior(const double *xi_odom) { return vgmp::make_prior(xi_odom, 0.03, 0.03, 0.01, 0.01); }

// one pose of compute_pose under the rule of vg_lm6.hpp: its state, the step in flight and the 28 sums at s.x
struct LmPose {
    vglm6::State s{};
    vglm6::Step st{};
    double G[vgp::kSums];
};

// ---- mutual information ------------------------------------------------------------------------------------------------

int ensure_mi(vg_photometric *s, int64_t n, unsigned blocks)
{
    if (const int rc = s->d_mi_log.grow((size_t)n * vgp::kMiCells, "the mutual-information results")) return rc;
    if (const int rc = s->d_mi_out.grow((size_t)n * vgp::kMiOut, "the mutual-information results")) return rc;
    if (const int rc = s->h_mi_out.grow((size_t)n * vgp::kMiOut, "the mutual-information staging")) return rc;
    if (const int rc = s->d_mi_hist.grow((size_t)(n * blocks) * vgp::kMiCells, "the mutual-information partial sums")) return rc;
    return s->d_mi_grad.grow((size_t)(n * blocks) * 6, "the mutual-information partial sums");
}

// MutualInformation::Evaluate of the n frames in h_frames at one scale (its pack is not empty): valVec2 to values (DEVICE, may
// be NULL), hist12 | cost | gradient of every active pose to h_mi_out; the gradient launches only with `grad`.  Synchronous.
int run_mi(vg_photometric *s, int scale, int64_t n, double *values, bool grad)
{
    const int64_t m = s->m[scale];
    const unsigned blocks = blocks_of(m, vgp::kLanes);
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (const int rc = ensure_mi(s, n, blocks)) return rc;
    VG_HIP(hipMemcpyAsync(s->d_frames, s->h_frames, (size_t)n * sizeof(vgp::PoseFrame), hipMemcpyHostToDevice, s->stream));
    vgp::MiArgs a;
    a.frames = s->d_frames;
    a.targets = s->d_targets;
    a.target_stride = s->off[s->levels];
    a.level_off = s->off[scale];
    a.w = s->w[scale];
    a.h = s->h[scale];
    a.inv_scale = 1. / (double)(1 << scale);
    for (int i = 0; i < 6; i++) a.cam[i] = s->cam[i];
    a.val = s->d_val.get() + s->off[scale];
    a.cloud = s->d_cloud.get() + 3 * s->off[scale];
    a.hist1 = s->d_hist1.get() + vgp::kMiBins * scale;
    a.m = (int)m;
    a.blocks = (int)blocks;
    a.increment = 1. / (double)m;
    a.values = values;
    a.hist_partials = s->d_mi_hist;
    a.grad_partials = s->d_mi_grad;
    a.logv = s->d_mi_log;
    a.out = s->d_mi_out;
    hipLaunchKernelGGL(vgp::mi_hist_kernel, dim3(blocks, (unsigned)n), dim3(vgp::kLanes), 0, s->stream, a);
    hipLaunchKernelGGL(vgp::mi_finish_kernel, dim3((unsigned)n), dim3(64), 0, s->stream, a);
    if (grad) {
        hipLaunchKernelGGL(vgp::mi_grad_kernel, dim3(blocks, (unsigned)n), dim3(vgp::kLanes), 0, s->stream, a);
        hipLaunchKernelGGL(vgp::mi_grad_reduce_kernel, dim3((unsigned)n), dim3(64), 0, s->stream, a);
    }
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(s->h_mi_out, s->d_mi_out, (size_t)n * vgp::kMiOut * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    return call.finish();
}

// MutualInformationOdom's constructor for xiOdom and xiPrior
vgp::MiOdometry make_mi_odometry(const double *xi_odom, const double *xi_prior)
{
    double R[9], M[9];
    const vg::RotTrig rt = vg::rot_trig(xi_prior + 3, true, true);
    vg::rotation_matrix(xi_prior + 3, -1., rt, R);
    vg::inter_omega_rot(xi_prior + 3, rt, M);
    vgp::MiOdometry o;
    vgp::mi_odometry_init(o, xi_odom, xi_prior, R, M);
    return o;
}

void add_mi_odometry(const vgp::MiOdometry &o, const double *x, double *cost, double *gradient)
{
    double err[6];
    vgth::inverse_compose(o.prior, x, err);
    vgp::mi_odometry_add(o, err, cost, gradient);
}

}  // namespace

extern "C" {

int vg_photometric_create(vg_photometric **out, int device, void *hip_stream, const double *eucm, const vg_stereo_params *params,
                          const double *xi_base_cam, int width, int height, int num_scales)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (!eucm || !params || !xi_base_cam) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const vg_stereo_params &p = *params;   // only the ScaleParameters fields are read; the image size is an argument
    int x_max = 0, y_max = 0;
    if (const int rc = vgsh::scaled_grid(p, false, x_max, y_max)) return rc;
    if (width < 1 || width > 16384 || height < 1 || height > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "the image size must be in [1, 16384]");
    if (num_scales < 1 || num_scales > vgp::kMaxLevels) return fail(VG_ERR_INVALID_ARGUMENT, "num_scales must be in [1, 8]");
    if ((width >> (num_scales - 1)) < 1 || (height >> (num_scales - 1)) < 1)
        return fail(VG_ERR_INVALID_ARGUMENT, "num_scales shrinks the coarsest level to zero size");
    if (!vgsh::finite_n(xi_base_cam, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "xi_base_cam must be finite");
    if (const int rc = vgsh::check_camera(eucm)) return rc;
    std::unique_ptr<vg_photometric> s(new (std::nothrow) vg_photometric());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    for (int i = 0; i < 6; i++) {
        s->cam[i] = eucm[i];
        s->xbc[i] = xi_base_cam[i];
    }
    s->g = vgp::Grid{p.scale, p.u0, p.v0, x_max, y_max};
    s->levels = num_scales;
    s->off[0] = 0;
    for (int i = 0; i < num_scales; i++) {
        s->w[i] = i ? s->w[i - 1] / 2 : width;
        s->h[i] = i ? s->h[i - 1] / 2 : height;
        s->off[i + 1] = s->off[i] + (int64_t)s->w[i] * s->h[i];
        s->m[i] = 0;
    }
    if (const int rc = s->open(device, hip_stream, "photometric localization")) return rc;
    *out = s.release();
    return VG_OK;
}

void vg_photometric_destroy(vg_photometric *s) { vgi::destroy(s); }

int vg_photometric_level_size(const vg_photometric *s, int scale_idx, int *width, int *height)
{
    if (!s || !width || !height) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (scale_idx < 0 || scale_idx >= s->levels) return fail(VG_ERR_INVALID_ARGUMENT, "scale index out of range");
    *width = s->w[scale_idx];
    *height = s->h[scale_idx];
    return VG_OK;
}

// the pyramids of n images into dst ([n][total]): one launch per level over all images
static int build_pyramids(vg_photometric *s, int64_t n, const uint8_t *img, float *dst)
{
    const int64_t total = s->off[s->levels];
    hipLaunchKernelGGL(vgs::u8_to_float_kernel<vgp::kLanes>, dim3(blocks_of(level_pixels(s, 0), vgp::kLanes), (unsigned)n), dim3(vgp::kLanes), 0, s->stream, img,
                       dst, level_pixels(s, 0), total);
    for (int i = 1; i < s->levels; i++)
        hipLaunchKernelGGL(vgp::photo_down_kernel, dim3(blocks_of(level_pixels(s, i), vgp::kLanes), (unsigned)n), dim3(vgp::kLanes), 0, s->stream, dst,
                           total, s->off[i - 1], s->w[i - 1], s->h[i - 1], s->off[i], s->w[i], s->h[i]);
    VG_HIP(hipGetLastError());
    return VG_OK;
}

// the data pack and _hist1 of every scale from the resident pyramid and the depth map, the counts to pack.h_totals; with `sobel` the
// gradients of the pyramid first (a new image).  Enqueues only.
static int launch_packs(vg_photometric *s, const double *depth, bool sobel)
{
    const int64_t total = s->off[s->levels];
    float *base = s->d_base.get();
    vgp::SelectArgs a;
    for (int i = 0; i < 6; i++) a.cam[i] = s->cam[i];
    a.g = s->g;
    a.depth = depth;
    vgth::rotation(s->xbc, a.Rb);
    for (int i = 0; i < 3; i++) a.tb[i] = s->xbc[i];
    a.block_counts = s->pack.counts;
    a.block_offsets = s->pack.offsets;
    for (int i = 0; i < s->levels; i++) {
        const unsigned nb = blocks_of(level_pixels(s, i), vgp::kLanes);
        if (sobel)
            hipLaunchKernelGGL(vgp::photo_sobel_kernel, dim3(nb, 1), dim3(vgp::kLanes), 0, s->stream, (const float *)(base + s->off[i]),
                               base + total + s->off[i], base + 2 * total + s->off[i], (int64_t)0, s->w[i], s->h[i]);
        a.img = base + s->off[i];
        a.gu = base + total + s->off[i];
        a.gv = base + 2 * total + s->off[i];
        a.w = s->w[i];
        a.h = s->h[i];
        a.level_scale = 1 << i;
        a.idx = s->d_idx.get() + s->off[i];
        a.val = s->d_val.get() + s->off[i];
        a.cloud = s->d_cloud.get() + 3 * s->off[i];
        hipLaunchKernelGGL((vgp::photo_select_kernel<false>), dim3(nb), dim3(vgp::kLanes), 0, s->stream, a);
        s->pack.scan<vgp::kLanes>(s->stream, (int)nb, i);
        hipLaunchKernelGGL((vgp::photo_select_kernel<true>), dim3(nb), dim3(vgp::kLanes), 0, s->stream, a);
        // MutualInformation's _hist1 depends on the pack only
        hipLaunchKernelGGL(vgp::mi_hist1_kernel, dim3(nb), dim3(vgp::kLanes), 0, s->stream, (const double *)a.val, (const unsigned *)(s->pack.totals.get() + i),
                           s->d_hist1_partials.get());
        hipLaunchKernelGGL(vgp::mi_hist1_reduce_kernel, dim3(1), dim3(64), 0, s->stream, (const double *)s->d_hist1_partials.get(), (int)nb,
                           s->d_hist1.get() + vgp::kMiBins * i);
    }
    VG_HIP(hipGetLastError());
    return s->pack.fetch(s->stream, vgp::kMaxLevels);
}

int vg_photometric_set_base(vg_photometric *s, const uint8_t *img, const double *depth)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "photometric handle is NULL");
    if (!img || !depth) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    const int64_t total = s->off[s->levels];
    s->has_base = false;
    {   // fixed sizes: allocated by the first call
        const size_t nb = blocks_of(level_pixels(s, 0), vgp::kLanes);
        const char *what = "the key frame's pyramid and data packs";
        if (const int rc = s->d_base.grow((size_t)(3 * total), what)) return rc;
        if (const int rc = s->d_idx.grow((size_t)total, what)) return rc;
        if (const int rc = s->d_val.grow((size_t)total, what)) return rc;
        if (const int rc = s->d_cloud.grow((size_t)(3 * total), what)) return rc;
        if (const int rc = s->pack.grow(nb, vgp::kMaxLevels, what)) return rc;
        if (const int rc = s->d_hist1.grow((size_t)vgp::kMaxLevels * vgp::kMiBins, what)) return rc;
        if (const int rc = s->d_hist1_partials.grow(nb * vgp::kMiBins, what)) return rc;
    }
    if (const int rc = build_pyramids(s, 1, img, s->d_base.get())) return rc;
    if (const int rc = launch_packs(s, depth, true)) return rc;
    if (const int rc = call.finish()) return rc;
    for (int i = 0; i < s->levels; i++) s->m[i] = s->pack.h_totals.get()[i];
    s->has_base = true;
    return VG_OK;
}

int vg_photo_set_depth(vg_photometric *s, const double *depth)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "photometric handle is NULL");
    if (!depth) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!s->has_base) return fail(VG_ERR_STATE, "no key frame image: call vg_photometric_set_base first");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    s->has_base = false;   // the packs are rewritten: a failure below leaves no key frame
    if (const int rc = launch_packs(s, depth, false)) return rc;
    if (const int rc = call.finish()) return rc;
    for (int i = 0; i < s->levels; i++) s->m[i] = s->pack.h_totals.get()[i];
    s->has_base = true;
    return VG_OK;
}

int vg_photometric_set_targets(vg_photometric *s, int64_t n, const uint8_t *imgs)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "photometric handle is NULL");
    if (const int rc = vgi::check_items(n, 1, "target")) return rc;
    if (!imgs) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    s->n_targets = 0;
    if (const int rc = s->d_targets.grow((size_t)(n * s->off[s->levels]), "the target pyramids")) return rc;
    if (const int rc = build_pyramids(s, n, imgs, s->d_targets)) return rc;
    if (const int rc = call.finish()) return rc;
    s->n_targets = n;
    return VG_OK;
}

int vg_photometric_level(vg_photometric *s, int64_t target, int scale_idx, float *img, float *grad_u, float *grad_v)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "photometric handle is NULL");
    if (scale_idx < 0 || scale_idx >= s->levels) return fail(VG_ERR_INVALID_ARGUMENT, "scale index out of range");
    if (target < 0 ? !s->has_base : target >= s->n_targets) return fail(VG_ERR_INVALID_ARGUMENT, "no such pyramid: set_base / set_targets first");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    const int64_t total = s->off[s->levels], P = level_pixels(s, scale_idx);
    const size_t bytes = (size_t)P * sizeof(float);
    const float *src = (target < 0 ? s->d_base.get() : s->d_targets.get() + target * total) + s->off[scale_idx];
    if (img) VG_HIP(hipMemcpyAsync(img, src, bytes, hipMemcpyDeviceToDevice, s->stream));
    if (grad_u || grad_v) {
        const float *gu = nullptr, *gv = nullptr;
        if (target < 0) {
            gu = s->d_base.get() + total + s->off[scale_idx];
            gv = s->d_base.get() + 2 * total + s->off[scale_idx];
        } else {   // a target keeps no gradients (scaleSpace2 has none): made here, for the caller
            if (const int rc = s->d_grad.grow((size_t)(2 * level_pixels(s, 0)), "the gradient scratch")) return rc;
            hipLaunchKernelGGL(vgp::photo_sobel_kernel, dim3(blocks_of(P, vgp::kLanes), 1), dim3(vgp::kLanes), 0, s->stream, src, s->d_grad.get(),
                               s->d_grad.get() + P, (int64_t)0, s->w[scale_idx], s->h[scale_idx]);
            VG_HIP(hipGetLastError());
            gu = s->d_grad.get();
            gv = s->d_grad.get() + P;
        }
        if (grad_u) VG_HIP(hipMemcpyAsync(grad_u, gu, bytes, hipMemcpyDeviceToDevice, s->stream));
        if (grad_v) VG_HIP(hipMemcpyAsync(grad_v, gv, bytes, hipMemcpyDeviceToDevice, s->stream));
    }
    return call.finish();
}

int vg_photometric_pack(vg_photometric *s, int scale_idx, int64_t *count, int32_t *indices, double *values, double *cloud)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "photometric handle is NULL");
    if (!s->has_base) return fail(VG_ERR_INVALID_ARGUMENT, "no key frame: call vg_photometric_set_base first");
    if (scale_idx < 0 || scale_idx >= s->levels) return fail(VG_ERR_INVALID_ARGUMENT, "scale index out of range");
    const int64_t m = s->m[scale_idx], o = s->off[scale_idx];
    if (count) *count = m;
    if (m == 0 || (!indices && !values && !cloud)) return VG_OK;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (indices) VG_HIP(hipMemcpyAsync(indices, s->d_idx.get() + o, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToDevice, s->stream));
    if (values) VG_HIP(hipMemcpyAsync(values, s->d_val.get() + o, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    if (cloud) VG_HIP(hipMemcpyAsync(cloud, s->d_cloud.get() + 3 * o, (size_t)(3 * m) * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    return call.finish();
}

int vg_photometric_evaluate(vg_photometric *s, int scale_idx, int64_t n, const double *xi, const int32_t *target, double *residuals,
                            double *jacobians, double *cost, double *jtj, double *jtr)
{
    if (const int rc = check_poses(s, n, xi, target)) return rc;
    if (scale_idx < 0 || scale_idx >= s->levels) return fail(VG_ERR_INVALID_ARGUMENT, "scale index out of range");
    VG_HIP(hipSetDevice(s->device));
    if (const int rc = ensure_poses(s, n)) return rc;
    for (int64_t k = 0; k < n; k++) make_frame(s, xi + 6 * k, target[k], true, s->h_frames.get()[k]);
    const bool sums = cost || jtj || jtr;
    if (const int rc = run_cost(s, scale_idx, n, residuals, jacobians, sums)) return rc;
    for (int64_t k = 0; sums && k < n; k++) {
        const double *G = s->h_sums.get() + k * vgp::kSums;
        if (jtj) std::memcpy(jtj + 21 * k, G, 21 * sizeof(double));
        if (jtr) std::memcpy(jtr + 6 * k, G + 21, 6 * sizeof(double));
        if (cost) cost[k] = G[27];
    }
    return VG_OK;
}

int vg_photometric_compute_pose(vg_photometric *s, int64_t n, const double *xi_start, const int32_t *target, const double *xi_prior, double *xi_out,
                                double *report)
{
    if (const int rc = check_poses(s, n, xi_start, target)) return rc;
    if (!xi_out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (xi_prior && !vgsh::finite_n(xi_prior, 6 * (int)n)) return fail(VG_ERR_INVALID_ARGUMENT, "the priors must be finite");
    VG_HIP(hipSetDevice(s->device));
    if (const int rc = ensure_poses(s, n)) return rc;
    std::vector<LmPose> P((size_t)n);
    std::vector<MotionPrior> prior;
    for (int64_t k = 0; k < n; k++) {
        std::memcpy(P[k].s.x, xi_start + 6 * k, sizeof(double) * 6);
        if (xi_prior) prior.push_back(make_prior(xi_prior + 6 * k));
    }
    for (int scale = s->levels - 1; scale >= 0; scale--) {
        for (int64_t k = 0; k < n; k++) make_frame(s, P[k].s.x, target[k], true, s->h_frames.get()[k]);
        if (const int rc = run_cost(s, scale, n, nullptr, nullptr, true)) return rc;
        for (int64_t k = 0; k < n; k++) {
            std::memcpy(P[k].G, s->h_sums.get() + k * vgp::kSums, sizeof P[k].G);
            if (xi_prior) add_prior(prior[k], P[k].s.x, P[k].G);
            vglm6::start(kRule, P[k].s, P[k].G[27]);
            if (report) report[(k * s->levels + scale) * 4 + 1] = P[k].s.cost;
        }
        for (;;) {
            bool any = false, launch = false;
            for (int64_t k = 0; k < n; k++) {
                if (!P[k].s.done) {
                    vglm6::step(kRule, P[k].s, P[k].G, P[k].st);
                    any = true;
                }
                const bool active = !P[k].s.done && P[k].st.ok;   // a pose that has converged is masked
                make_frame(s, active ? P[k].st.xc : P[k].s.x, target[k], active, s->h_frames.get()[k]);
                launch = launch || active;
            }
            if (!any) break;
            if (launch)
                if (const int rc = run_cost(s, scale, n, nullptr, nullptr, true)) return rc;
            for (int64_t k = 0; k < n; k++) {
                if (P[k].s.done) continue;
                double Gc[vgp::kSums] = {0.};
                if (P[k].st.ok) {
                    std::memcpy(Gc, s->h_sums.get() + k * vgp::kSums, sizeof Gc);
                    if (xi_prior) add_prior(prior[k], P[k].st.xc, Gc);
                }
                if (vglm6::accept(kRule, P[k].s, P[k].st, Gc[27])) std::memcpy(P[k].G, Gc, sizeof Gc);
            }
        }
        for (int64_t k = 0; report && k < n; k++) {
            double *r = report + (k * s->levels + scale) * 4;
            r[0] = P[k].s.iterations;
            r[2] = P[k].s.cost;
            r[3] = P[k].s.term;
        }
    }
    for (int64_t k = 0; k < n; k++) std::memcpy(xi_out + 6 * k, P[k].s.x, sizeof(double) * 6);
    return VG_OK;
}

int vg_mi_evaluate(vg_photometric *s, int scale_idx, int64_t n, const double *xi, const int32_t *target, double *values, double *hist,
                   double *cost, double *gradient)
{
    if (const int rc = check_poses(s, n, xi, target)) return rc;
    if (scale_idx < 0 || scale_idx >= s->levels) return fail(VG_ERR_INVALID_ARGUMENT, "scale index out of range");
    if (s->m[scale_idx] == 0) return fail(VG_ERR_INVALID_ARGUMENT, "the data pack of this scale is empty: the histogram increment would be 1 / 0");
    VG_HIP(hipSetDevice(s->device));
    if (const int rc = ensure_poses(s, n)) return rc;
    for (int64_t k = 0; k < n; k++) make_frame(s, xi + 6 * k, target[k], true, s->h_frames.get()[k]);
    if (const int rc = run_mi(s, scale_idx, n, values, gradient != nullptr)) return rc;
    for (int64_t k = 0; k < n; k++) {
        const double *o = s->h_mi_out.get() + k * vgp::kMiOut;
        if (hist) std::memcpy(hist + vgp::kMiCells * k, o, vgp::kMiCells * sizeof(double));
        if (cost) cost[k] = o[vgp::kMiCells];
        if (gradient) std::memcpy(gradient + 6 * k, o + vgp::kMiCells + 1, 6 * sizeof(double));
    }
    return VG_OK;
}

int vg_mi_odometry(const double *xi_odom, const double *xi_prior, const double *xi, double *cost, double *gradient)
{
    if (!xi_odom || !xi_prior || !xi || !cost) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi_odom, 6) || !vgsh::finite_n(xi_prior, 6) || !vgsh::finite_n(xi, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "the poses must be finite");
    const vgp::MiOdometry o = make_mi_odometry(xi_odom, xi_prior);
    *cost = 0.;
    for (int i = 0; gradient && i < 6; i++) gradient[i] = 0.;
    add_mi_odometry(o, xi, cost, gradient);
    return VG_OK;
}

int vg_mi_compute_pose(vg_photometric *s, int64_t n, const double *xi_start, const int32_t *target, const double *xi_odom,
                       const vg_mi_options *options, double *xi_out, double *report)
{
    if (const int rc = check_poses(s, n, xi_start, target)) return rc;
    if (!xi_out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (xi_odom && !vgsh::finite_n(xi_odom, 6 * (int)n)) return fail(VG_ERR_INVALID_ARGUMENT, "the odometry poses must be finite");
    vg_mi_options opt = {0., 0., 0};
    if (options) opt = *options;
    if (!(opt.function_tolerance >= 0.) || !(opt.gradient_tolerance >= 0.) || opt.max_iterations < 0)
        return fail(VG_ERR_INVALID_ARGUMENT, "the tolerances and max_iterations must not be negative");
    if (opt.function_tolerance == 0.) opt.function_tolerance = VG_MI_FUNCTION_TOLERANCE;
    if (opt.gradient_tolerance == 0.) opt.gradient_tolerance = VG_MI_GRADIENT_TOLERANCE;
    if (opt.max_iterations == 0) opt.max_iterations = VG_MI_MAX_ITERATIONS;
    bool any_points = false;
    for (int i = 0; i < s->levels; i++) any_points = any_points || s->m[i] > 0;
    if (!any_points) return fail(VG_ERR_INVALID_ARGUMENT, "the data pack of every scale is empty");
    VG_HIP(hipSetDevice(s->device));
    if (const int rc = ensure_poses(s, n)) return rc;
    std::vector<vgp::MiBfgs> B((size_t)n);
    std::vector<vgp::MiOdometry> odom;
    std::vector<char> active((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        std::memcpy(B[k].x, xi_start + 6 * k, sizeof(double) * 6);
        B[k].ftol = opt.function_tolerance;
        B[k].gtol = opt.gradient_tolerance;
        B[k].max_iterations = opt.max_iterations;
        if (xi_odom) odom.push_back(make_mi_odometry(xi_odom + 6 * k, xi_start + 6 * k));   // xiPrior is the start pose
    }
    for (int scale = s->levels - 1; scale >= 0; scale--) {
        if (s->m[scale] == 0) {   // nothing to match at this scale: the pose passes through
            for (int64_t k = 0; report && k < n; k++) {
                double *r = report + (k * s->levels + scale) * 4;
                r[0] = r[1] = r[2] = 0.;
                r[3] = VG_TERM_NO_CONVERGENCE;
            }
            continue;
        }
        for (int64_t k = 0; k < n; k++) {
            const double x[6] = {B[k].x[0], B[k].x[1], B[k].x[2], B[k].x[3], B[k].x[4], B[k].x[5]};
            B[k].start(x);
        }
        for (;;) {
            bool any = false, launch = false;
            for (int64_t k = 0; k < n; k++) {
                active[k] = !B[k].done && B[k].trial_finite();   // a finished pose is masked; so is a trial that is not finite
                any = any || !B[k].done;
                launch = launch || active[k];
                make_frame(s, active[k] ? B[k].trial() : B[k].x, target[k], active[k] != 0, s->h_frames.get()[k]);
            }
            if (!any) break;
            if (launch)
                if (const int rc = run_mi(s, scale, n, nullptr, true)) return rc;
            for (int64_t k = 0; k < n; k++) {
                if (B[k].done) continue;
                double f = 0., g[6] = {0., 0., 0., 0., 0., 0.};
                if (active[k]) {
                    const double *o = s->h_mi_out.get() + k * vgp::kMiOut;
                    f = o[vgp::kMiCells];
                    std::memcpy(g, o + vgp::kMiCells + 1, sizeof g);
                    if (xi_odom) add_mi_odometry(odom[k], B[k].trial(), &f, g);
                }
                B[k].consume(f, g, active[k] != 0);
            }
        }
        for (int64_t k = 0; report && k < n; k++) {
            double *r = report + (k * s->levels + scale) * 4;
            r[0] = B[k].iterations;
            r[1] = B[k].initial_cost;
            r[2] = B[k].f;
            r[3] = B[k].term;
        }
    }
    for (int64_t k = 0; k < n; k++) std::memcpy(xi_out + 6 * k, B[k].x, sizeof(double) * 6);
    return VG_OK;
}

}  // extern "C"
