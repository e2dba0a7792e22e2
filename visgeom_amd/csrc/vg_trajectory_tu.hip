// vg_trajectory_tu.hip -- translation unit of libvisgeom_amd.so: calibration trajectory planning (section 17 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_trajectory handle owns the scratch of a batch on the device -- the points, the poses and covariances the prepass writes,
// the per-pose contributions -- and pinned staging for what goes up and comes back.  Buffers only grow.  The caller's arrays
// are host memory: a call is one copy up, three launches, one copy back and one synchronisation.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#include "vg_bfgs.hpp"
#include "vg_handle.hpp"
#include "vg_stereo_host.hpp"
#include "vg_trajectory.hpp"

struct vg_trajectory : vgi::HandleBase {
    vgt::Setup s;
    int PT = 0, n_poses = 0, n_slots = 0;
    int64_t launches = 0;
    vgi::Grow<double> d_in, d_xi, d_cov, d_contrib, d_pen, d_out;
    vgi::Grow<int32_t> d_bad, d_invalid;
    vgi::GrowPinned<double> h_in, h_out;
    vgi::GrowPinned<int32_t> h_invalid;
};

namespace {

using vgi::fail;
using vgsh::blocks_of;

static_assert(vgb::kTermFunction == VG_TERM_CONVERGENCE_FUNCTION && vgb::kTermGradient == VG_TERM_CONVERGENCE_GRADIENT &&
                  vgb::kTermParameter == VG_TERM_CONVERGENCE_PARAMETER && vgb::kTermNoConvergence == VG_TERM_NO_CONVERGENCE &&
                  vgb::kTermFailure == VG_TERM_FAILURE,
              "vg_bfgs.hpp restates vg_termination");
static_assert(vgt::kP == VG_TRAJECTORY_PARAMS && vgt::kMaxTraj == VG_TRAJECTORY_MAX && vgt::kMinSteps == VG_TRAJECTORY_MIN_STEPS &&
                  vgt::kMaxSteps == VG_TRAJECTORY_MAX_STEPS && vgt::kMaxCorners == VG_TRAJECTORY_MAX_CORNERS && vgt::kTerms == VG_TRAJECTORY_TERMS &&
                  vgi::kMaxItems == VG_TRAJECTORY_MAX_POINTS,
              "vg_trajectory.hpp restates the header's limits");

int check_steps(int n_trajectories, const int *steps)
{
    if (n_trajectories < 1 || n_trajectories > vgt::kMaxTraj) return fail(VG_ERR_INVALID_ARGUMENT, "1 to 8 trajectories expected");
    if (!steps) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int t = 0; t < n_trajectories; t++)
        if (steps[t] < vgt::kMinSteps || steps[t] > vgt::kMaxSteps) return fail(VG_ERR_INVALID_ARGUMENT, "a trajectory's number of steps must be in [2, 256]");
    return VG_OK;
}

int check_scene(int model, const double *intrinsics, int width, int height, const vg_trajectory_quality *q)
{
    if (model != VG_MODEL_EUCM) return fail(VG_ERR_INVALID_ARGUMENT, "trajectory planning is built for the EUCM camera only");
    if (!intrinsics || !q) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = vgsh::check_camera(intrinsics)) return rc;
    if (width < 1 || height < 1) return fail(VG_ERR_INVALID_ARGUMENT, "the image's width and height must be positive");
    if (!vgsh::finite_n(q->xi_base_cam, 6) || !vgsh::finite_n(q->xi_orig_board, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "xiBaseCam and xiOrigBoard must be finite");
    if (q->board_cols < 2 || q->board_rows < 2 || (int64_t)q->board_cols * q->board_rows > vgt::kMaxCorners)
        return fail(VG_ERR_INVALID_ARGUMENT, "the board needs cols, rows >= 2 and at most 1024 corners");
    if (!(q->board_step > 0.) || !std::isfinite(q->board_step)) return fail(VG_ERR_INVALID_ARGUMENT, "the board's step must be positive");
    if (!(q->turn_radius > 0.) || !std::isfinite(q->turn_radius)) return fail(VG_ERR_INVALID_ARGUMENT, "turn_radius must be positive");
    if (!std::isfinite(q->min_camera_dist) || !std::isfinite(q->min_margin) || !std::isfinite(q->min_cell_size))
        return fail(VG_ERR_INVALID_ARGUMENT, "min_camera_dist, min_margin and min_cell_size must be finite");
    for (int k = 0; k < 6; k++)
        if (!(q->prior_variance[k] > 0.) || !std::isfinite(q->prior_variance[k])) return fail(VG_ERR_INVALID_ARGUMENT, "prior_variance must be positive");
    if (!(q->feature_variance > 0.) || !std::isfinite(q->feature_variance)) return fail(VG_ERR_INVALID_ARGUMENT, "feature_variance must be positive");
    return VG_OK;
}

int check_points(const vg_trajectory *s, int64_t n, const double *params, int per_point)
{
    if (n < 0 || n * per_point > vgi::kMaxItems) return fail(VG_ERR_INVALID_ARGUMENT, "the point count of the batch must be in [0, 65535]");
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "trajectory handle is NULL");
    if (n > 0 && !params) return fail(VG_ERR_INVALID_ARGUMENT, "the parameters are NULL");
    for (int64_t k = 0; k < n * s->PT; k++)
        if (!std::isfinite(params[k])) return fail(VG_ERR_INVALID_ARGUMENT, "the parameters must be finite");
    return VG_OK;
}

// the points p [m][PT] (host, any memory) -> cost [m], terms [m][5], invalid [m] in the handle's pinned staging
int run_points(vg_trajectory *s, int64_t m, const double *p)
{
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    const size_t in = (size_t)m * s->PT, out = (size_t)m * (1 + vgt::kTerms);
    if (const int rc = s->h_in.grow(in, "the points' staging")) return rc;
    if (const int rc = s->d_in.grow(in, "the points")) return rc;
    if (const int rc = s->d_xi.grow((size_t)m * s->n_poses * 6, "the poses")) return rc;
    if (const int rc = s->d_cov.grow((size_t)m * s->n_poses * 36, "the odometry covariances")) return rc;
    if (const int rc = s->d_contrib.grow((size_t)m * s->n_slots * 36, "the pose contributions")) return rc;
    if (const int rc = s->d_pen.grow((size_t)m * s->n_slots * 4, "the pose penalties")) return rc;
    if (const int rc = s->d_bad.grow((size_t)m * s->n_slots, "the pose flags")) return rc;
    if (const int rc = s->d_out.grow(out, "the results")) return rc;
    if (const int rc = s->d_invalid.grow((size_t)m, "the invalid counts")) return rc;
    if (const int rc = s->h_out.grow(out, "the results' staging")) return rc;
    if (const int rc = s->h_invalid.grow((size_t)m, "the invalid counts' staging")) return rc;
    std::memcpy(s->h_in.get(), p, in * sizeof(double));
    VG_HIP(hipMemcpyAsync(s->d_in, s->h_in, in * sizeof(double), hipMemcpyHostToDevice, s->stream));
    vgt::EvalArgs a;
    a.s = s->s;
    a.n = m;
    a.PT = s->PT;
    a.n_poses = s->n_poses;
    a.n_slots = s->n_slots;
    a.params = s->d_in;
    a.xi = s->d_xi;
    a.cov = s->d_cov;
    a.contrib = s->d_contrib;
    a.pen = s->d_pen;
    a.bad = s->d_bad;
    a.cost = s->d_out;
    a.terms = s->d_out.get() + m;
    a.invalid = s->d_invalid;
    const size_t lds = (size_t)2 * s->s.nx * s->s.ny * sizeof(double);
    hipLaunchKernelGGL(vgt::trajectory_prepass_kernel, dim3(blocks_of(m * s->s.T, vgt::kWave)), dim3(vgt::kWave), 0, s->stream, a);
    hipLaunchKernelGGL(vgt::trajectory_pose_kernel<vg::kEUCM>, dim3((unsigned)s->n_slots, (unsigned)m), dim3(vgt::kWave), lds, s->stream, a);
    hipLaunchKernelGGL(vgt::trajectory_finish_kernel, dim3(blocks_of(m, vgt::kWave)), dim3(vgt::kWave), 0, s->stream, a);
    VG_HIP(hipGetLastError());
    s->launches += 3;
    VG_HIP(hipMemcpyAsync(s->h_out, s->d_out, out * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    VG_HIP(hipMemcpyAsync(s->h_invalid, s->d_invalid, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    return call.finish();
}

void gradient_points(int PT, const double *p, double *points, double *delta)
{
    for (int r = 0; r < 2 * PT + 1; r++) std::memcpy(points + (size_t)r * PT, p, sizeof(double) * PT);
    for (int i = 0; i < PT; i++) {
        const double d = std::fmax(std::fabs(p[i]) * vgt::kDiffEps, vgt::kDiffEps * vgt::kDiffEps), orig = p[i];
        points[(size_t)(1 + 2 * i) * PT + i] = orig + d;
        points[(size_t)(2 + 2 * i) * PT + i] = orig - d;
        if (delta) delta[i] = d;
    }
}

// cost, gradient and validity of the point whose 2 PT + 1 results start at row `first` of the staging
bool gradient_of(const vg_trajectory *s, int64_t first, const double *delta, double *cost, double *grad)
{
    const double *c = s->h_out.get() + first;
    const int32_t *inv = s->h_invalid.get() + first;
    bool ok = true;
    for (int r = 0; r < 2 * s->PT + 1; r++) ok = ok && inv[r] == 0 && std::isfinite(c[r]);
    *cost = c[0];
    for (int i = 0; i < s->PT; i++) grad[i] = ok ? (c[1 + 2 * i] - c[2 + 2 * i]) / (2 * delta[i]) : std::numeric_limits<double>::quiet_NaN();
    return ok;
}

}  // namespace

extern "C" {

void vg_trajectory_default_options(vg_trajectory_options *o)
{
    if (!o) return;
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->max_iterations = 1000;
}

int vg_trajectory_create(vg_trajectory **out, int device, void *hip_stream, int model, const double *intrinsics, int width, int height,
                         const vg_trajectory_quality *q, int n_trajectories, const int *steps)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (const int rc = check_scene(model, intrinsics, width, height, q)) return rc;
    if (const int rc = check_steps(n_trajectories, steps)) return rc;
    std::unique_ptr<vg_trajectory> s(new (std::nothrow) vg_trajectory());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    vgt::Setup &u = s->s;
    std::memset(&u, 0, sizeof u);
    u.model = model;
    for (int k = 0; k < 6; k++) {
        u.cam[k] = intrinsics[k];
        u.xi_cam[k] = q->xi_base_cam[k];
        u.xi_board[k] = q->xi_orig_board[k];
        u.hess_prior[k] = 1. / q->prior_variance[k];
    }
    u.width = width;
    u.height = height;
    vgt::screw_transf_inv(u.xi_cam, u.L_cam);
    u.kappa_max = 1. / q->turn_radius;
    u.min_dist = q->min_camera_dist;
    u.margin = q->min_margin;
    u.min_cell = q->min_cell_size;
    u.stiffness = std::sqrt(1. / q->feature_variance);   // both diagonal entries of LLT(I / feature_variance).matrixU()
    u.step = q->board_step;
    u.nx = q->board_cols;
    u.ny = q->board_rows;
    u.T = n_trajectories;
    for (int t = 0; t < n_trajectories; t++) {
        u.steps[t] = steps[t];
        u.pose0[t + 1] = u.pose0[t] + steps[t];
        u.slot0[t + 1] = u.slot0[t] + steps[t] - 1;
    }
    s->PT = vgt::kP * n_trajectories;
    s->n_poses = u.pose0[n_trajectories];
    s->n_slots = u.slot0[n_trajectories];
    if (const int rc = s->open(device, hip_stream, "trajectory planning")) return rc;
    *out = s.release();
    return VG_OK;
}

void vg_trajectory_destroy(vg_trajectory *s) { vgi::destroy(s); }

int vg_trajectory_size(const vg_trajectory *s, int *n_trajectories, int *n_params, int *n_poses)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "trajectory handle is NULL");
    if (n_trajectories) *n_trajectories = s->s.T;
    if (n_params) *n_params = s->PT;
    if (n_poses) *n_poses = s->n_poses;
    return VG_OK;
}

int vg_trajectory_launch_count(const vg_trajectory *s, int64_t *count)
{
    if (!s || !count) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *count = s->launches;
    return VG_OK;
}

int vg_trajectory_evaluate(vg_trajectory *s, int64_t n, const double *params, double *cost, double *terms, int32_t *invalid)
{
    if (const int rc = check_points(s, n, params, 1)) return rc;
    if (n > 0 && !cost) return fail(VG_ERR_INVALID_ARGUMENT, "the cost array is NULL");
    if (n == 0) return VG_OK;
    if (const int rc = run_points(s, n, params)) return rc;
    std::memcpy(cost, s->h_out.get(), sizeof(double) * (size_t)n);
    if (terms) std::memcpy(terms, s->h_out.get() + n, sizeof(double) * (size_t)n * vgt::kTerms);
    if (invalid) std::memcpy(invalid, s->h_invalid.get(), sizeof(int32_t) * (size_t)n);
    return VG_OK;
}

int vg_trajectory_visual_cov(vg_trajectory *s, int64_t n, const double *cam_poses, double *cov, double *info, int32_t *invalid)
{
    if (const int rc = vgi::check_items(n, 0, "pose")) return rc;
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "trajectory handle is NULL");
    if (n > 0 && (!cam_poses || !cov || !info || !invalid)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > 0 && !vgsh::finite_n(cam_poses, 6 * (int)n)) return fail(VG_ERR_INVALID_ARGUMENT, "the camera poses must be finite");
    if (n == 0) return VG_OK;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    const size_t in = (size_t)n * 6, out = (size_t)n * 72;
    if (const int rc = s->h_in.grow(in, "the poses' staging")) return rc;
    if (const int rc = s->d_in.grow(in, "the poses")) return rc;
    if (const int rc = s->d_out.grow(out, "the results")) return rc;
    if (const int rc = s->d_invalid.grow((size_t)n, "the invalid flags")) return rc;
    if (const int rc = s->h_out.grow(out, "the results' staging")) return rc;
    if (const int rc = s->h_invalid.grow((size_t)n, "the invalid flags' staging")) return rc;
    std::memcpy(s->h_in.get(), cam_poses, in * sizeof(double));
    VG_HIP(hipMemcpyAsync(s->d_in, s->h_in, in * sizeof(double), hipMemcpyHostToDevice, s->stream));
    vgt::CovArgs a;
    a.s = s->s;
    a.n = n;
    a.poses = s->d_in;
    a.cov = s->d_out;
    a.info = s->d_out.get() + n * 36;
    a.invalid = s->d_invalid;
    const size_t lds = (size_t)2 * s->s.nx * s->s.ny * sizeof(double);
    hipLaunchKernelGGL(vgt::trajectory_visual_cov_kernel<vg::kEUCM>, dim3((unsigned)n), dim3(vgt::kWave), lds, s->stream, a);
    VG_HIP(hipGetLastError());
    s->launches += 1;
    VG_HIP(hipMemcpyAsync(s->h_out, s->d_out, out * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    VG_HIP(hipMemcpyAsync(s->h_invalid, s->d_invalid, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    if (const int rc = call.finish()) return rc;
    std::memcpy(cov, s->h_out.get(), sizeof(double) * (size_t)n * 36);
    std::memcpy(info, s->h_out.get() + n * 36, sizeof(double) * (size_t)n * 36);
    std::memcpy(invalid, s->h_invalid.get(), sizeof(int32_t) * (size_t)n);
    return VG_OK;
}

int vg_trajectory_gradient_points(int n_params, const double *params, double *points, double *delta)
{
    if (n_params < 1 || n_params > vgt::kP * vgt::kMaxTraj) return fail(VG_ERR_INVALID_ARGUMENT, "1 to 40 parameters expected");
    if (!params || !points) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    gradient_points(n_params, params, points, delta);
    return VG_OK;
}

int vg_trajectory_gradient(vg_trajectory *s, int64_t n, const double *params, double *cost, double *grad, int32_t *invalid)
{
    if (const int rc = check_points(s, n, params, s ? 2 * s->PT + 1 : 1)) return rc;
    if (n > 0 && (!cost || !grad)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n == 0) return VG_OK;
    const int PT = s->PT, per = 2 * PT + 1;
    std::vector<double> points((size_t)n * per * PT), delta((size_t)n * PT);
    for (int64_t k = 0; k < n; k++) gradient_points(PT, params + k * PT, points.data() + (size_t)k * per * PT, delta.data() + k * PT);
    if (const int rc = run_points(s, n * per, points.data())) return rc;
    for (int64_t k = 0; k < n; k++) {
        const bool ok = gradient_of(s, k * per, delta.data() + k * PT, cost + k, grad + k * PT);
        if (invalid) invalid[k] = ok ? 0 : 1;
    }
    return VG_OK;
}

int vg_trajectory_poses(int n_trajectories, const int *steps, const double *params, double *xi, double *cov)
{
    if (const int rc = check_steps(n_trajectories, steps)) return rc;
    if (!params || !xi) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(params, vgt::kP * n_trajectories)) return fail(VG_ERR_INVALID_ARGUMENT, "the parameters must be finite");
    int64_t o = 0;
    for (int t = 0; t < n_trajectories; t++) {
        vgt::TrajectoryWalk w;
        vgt::walk_start(params + vgt::kP * t, w);
        for (int i = 0; i < steps[t]; i++, o++) {
            if (i > 0) vgt::walk_step(w);
            std::memcpy(xi + 6 * o, w.xi, sizeof w.xi);
            if (cov) vgt::walk_cov(w, i == 0, cov + 36 * o);
        }
    }
    return VG_OK;
}

int vg_trajectory_project_board(int model, const double *intrinsics, const vg_trajectory_quality *q, const double *cam_pose, double *uv, int32_t *ok)
{
    if (const int rc = check_scene(model, intrinsics, 1, 1, q)) return rc;
    if (!cam_pose || !uv || !ok) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(cam_pose, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "the camera pose must be finite");
    double xcb[6], R[9];
    vgt::inverse_compose(cam_pose, q->xi_orig_board, xcb);
    vgt::rot_mat(xcb + 3, 1., R);
    for (int k = 0; k < q->board_cols * q->board_rows; k++) {
        const double bx = q->board_step * (k % q->board_cols), by = q->board_step * (k / q->board_cols);
        vg::CornerEval<6> e;
        vg::eval_corner<vg::kEUCM, false, false>(intrinsics, R[0] * bx + R[1] * by + xcb[0], R[3] * bx + R[4] * by + xcb[1], R[6] * bx + R[7] * by + xcb[2], e);
        uv[2 * k] = e.u;
        uv[2 * k + 1] = e.v;
        ok[k] = e.ok ? 1 : 0;
    }
    return VG_OK;
}

int vg_trajectory_optimize(vg_trajectory *s, int64_t n, double *params, const vg_trajectory_options *options, double *cost, int32_t *iterations,
                           int32_t *termination)
{
    if (const int rc = check_points(s, n, params, s ? 2 * s->PT + 1 : 1)) return rc;
    if (n > 0 && !cost) return fail(VG_ERR_INVALID_ARGUMENT, "the cost array is NULL");
    vg_trajectory_options opt;
    vg_trajectory_default_options(&opt);
    if (options) opt = *options;
    if (!(opt.function_tolerance >= 0.) || !(opt.gradient_tolerance >= 0.) || !(opt.parameter_tolerance >= 0.) || opt.max_iterations < 0)
        return fail(VG_ERR_INVALID_ARGUMENT, "the tolerances and max_iterations must not be negative");
    if (n == 0) return VG_OK;
    const int PT = s->PT, per = 2 * PT + 1;
    std::vector<vgb::Bfgs> B((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        B[k].ftol = opt.function_tolerance;
        B[k].gtol = opt.gradient_tolerance;
        B[k].ptol = opt.parameter_tolerance;
        B[k].max_iterations = opt.max_iterations;
        B[k].start(params + k * PT, PT);
    }
    std::vector<int64_t> live;
    std::vector<double> points, delta, g((size_t)PT);
    for (;;) {
        live.clear();
        for (int64_t k = 0; k < n; k++) {
            if (B[k].done) continue;
            if (B[k].trial_finite()) live.push_back(k);
            else B[k].consume(0., g.data(), false);   // nothing to evaluate there: a failed trial
        }
        bool any = false;
        for (int64_t k = 0; k < n; k++) any = any || !B[k].done;
        if (!any) break;
        if (live.empty()) continue;
        const int64_t m = (int64_t)live.size();
        points.resize((size_t)m * per * PT);
        delta.resize((size_t)m * PT);
        for (int64_t j = 0; j < m; j++) gradient_points(PT, B[live[j]].trial(), points.data() + (size_t)j * per * PT, delta.data() + j * PT);
        if (const int rc = run_points(s, m * per, points.data())) return rc;   // one batch per round
        for (int64_t j = 0; j < m; j++) {
            double f;
            const bool ok = gradient_of(s, j * per, delta.data() + j * PT, &f, g.data());
            B[live[j]].consume(f, g.data(), ok);
        }
    }
    for (int64_t k = 0; k < n; k++) {
        std::memcpy(params + k * PT, B[k].x.data(), sizeof(double) * PT);
        cost[k] = B[k].f;
        if (iterations) iterations[k] = B[k].iterations;
        if (termination) termination[k] = B[k].term;
    }
    return VG_OK;
}

}  // extern "C"
