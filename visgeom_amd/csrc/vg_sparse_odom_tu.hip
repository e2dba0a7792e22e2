// vg_sparse_odom_tu.hip -- translation unit of libvisgeom_amd.so: sparse visual odometry (section 13 of the C ABI), the
// reference's SparseOdometry::feedData.  Built with hipcc for gfx950 only; compiled on its own so that an edit of one
// subsystem does not rebuild the others.
//
// A vg_sparse_odom handle owns the scratch of every stage (grown on demand, never shrunk), the previous frame's key points and
// descriptors, and the odometry state.  The stage entries are usable alone; ransac and feed are host orchestration of the
// same launches: every call is synchronous on the handle's stream.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "vg_handle.hpp"
#include "vg_local.hpp"
#include "vg_motion_prior.hpp"
#include "vg_sparse_odom.hpp"
#include "vg_stereo_host.hpp"
#include "vg_pose_host.hpp"

namespace {

using vgi::fail;
using vgsh::blocks_of;

constexpr int64_t kMaxPoints = 1 << 20;   // matches of a ransac / score call, entries of a solve call

}  // namespace

struct vg_sparse_odom : vgi::HandleBase {
    double cam[6], xbc[6];
    int w = 0, h = 0;
    vg_sparse_odom_params prm;
    int64_t cand_cap = 0;   // strict 3 x 3 maxima of the interior: no two are neighbours
    vgi::Grow<double> d_static;   // [81 weights | 6 intrinsics]
    // detect
    vgi::Grow<int32_t> d_grad, d_sums, d_cand_i, d_count;
    vgi::Grow<int64_t> d_resp, d_cand_r;
    vgi::Grow<unsigned int> d_cand_n;
    vgi::GrowPinned<int32_t> h_count;
    // match
    vgi::Grow<double> d_dist;
    vgi::Grow<int32_t> d_nn, d_cnt;
    // solve / score
    vgi::Grow<double> d_consts, d_out, d_frames, d_res;
    vgi::Grow<int64_t> d_offsets;
    vgi::Grow<int32_t> d_index, d_inliers;
    vgi::GrowPinned<double> h_out, h_res;
    vgi::GrowPinned<int32_t> h_inliers;
    // feed: two frame slots, the matches and rays of the current pair
    vgi::Grow<int32_t> d_kp[2], d_matches;
    vgi::Grow<float> d_desc[2];
    vgi::Grow<double> d_distance, d_rays;   // rays: x1 (3) | x2 (3) | p2 (2) | size (1) planes of max_features
    vgi::Grow<uint8_t> d_mask;
    int n_kp[2] = {0, 0}, cur = 0;
    bool has_prev = false;
    double odom_prev[6], xi_local[6], xi_incr[6];
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    std::vector<int32_t> perm;
};

namespace {

int check_handle(const vg_sparse_odom *s)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "sparse odometry handle is NULL");
    return VG_OK;
}

uint64_t next_random(vg_sparse_odom *s)   // xorshift64*
{
    uint64_t x = s->rng;
    x ^= x >> 12;
    x ^= x << 25;
    x ^= x >> 27;
    s->rng = x;
    return x * 0x2545F4914F6CDD1Dull;
}

void draw_samples(vg_sparse_odom *s, int64_t m, int32_t *samples)
{
    const int k = s->prm.num_ransac_points;
    if ((int64_t)s->perm.size() != m) {
        s->perm.resize((size_t)m);
        for (int64_t i = 0; i < m; i++) s->perm[(size_t)i] = (int32_t)i;
    }
    for (int it = 0; it < s->prm.ransac_iterations; it++)
        for (int p = 0; p < k; p++) {   // the head of a Fisher-Yates shuffle of the persistent index vector
            const int64_t j = p + (int64_t)(next_random(s) % (uint64_t)(m - p));
            std::swap(s->perm[(size_t)p], s->perm[(size_t)j]);
            samples[it * k + p] = s->perm[(size_t)p];
        }
}

// the Harris map of n images into resp (DEVICE [n][h][w]); queued, not synchronised
int launch_response(vg_sparse_odom *s, int64_t n, const uint8_t *img, int64_t *resp)
{
    const int64_t P = (int64_t)s->w * s->h;
    if (const int rc = s->d_grad.grow((size_t)(n * P), "the sparse odometry scratch")) return rc;
    if (const int rc = s->d_sums.grow((size_t)(3 * n * P), "the sparse odometry scratch")) return rc;
    const dim3 grid(blocks_of(P, vgso::kThreads), (unsigned)n);
    hipLaunchKernelGGL(vgso::gradient_kernel, grid, dim3(vgso::kThreads), 0, s->stream, img, s->w, s->h, s->d_grad.get());
    hipLaunchKernelGGL(vgso::row_sum_kernel, grid, dim3(vgso::kThreads), 0, s->stream, (const int32_t *)s->d_grad.get(), s->w, s->h, n * P, s->d_sums.get());
    hipLaunchKernelGGL(vgso::response_kernel, grid, dim3(vgso::kThreads), 0, s->stream, (const int32_t *)s->d_sums.get(), s->w, s->h, n * P, resp);
    VG_HIP(hipGetLastError());
    return VG_OK;
}

// detect of n images; count HOST.  Synchronous.
int run_detect(vg_sparse_odom *s, int64_t n, const uint8_t *img, int32_t *count, int32_t *keypoints, float *descriptors)
{
    const int64_t P = (int64_t)s->w * s->h;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (const int rc = s->d_resp.grow((size_t)(n * P), "the sparse odometry scratch")) return rc;
    if (const int rc = s->d_cand_r.grow((size_t)(n * s->cand_cap), "the sparse odometry scratch")) return rc;
    if (const int rc = s->d_cand_i.grow((size_t)(n * s->cand_cap), "the sparse odometry scratch")) return rc;
    if (const int rc = s->d_cand_n.grow((size_t)n, "the sparse odometry scratch")) return rc;
    if (const int rc = s->d_count.grow((size_t)n, "the sparse odometry scratch")) return rc;
    if (const int rc = s->h_count.grow((size_t)n, "the sparse odometry staging")) return rc;
    if (const int rc = launch_response(s, n, img, s->d_resp.get())) return rc;
    VG_HIP(hipMemsetAsync(s->d_cand_n.get(), 0, (size_t)n * sizeof(unsigned int), s->stream));
    const int64_t interior = (int64_t)(s->w - 2 * vgso::kBorder) * (s->h - 2 * vgso::kBorder);
    hipLaunchKernelGGL(vgso::maxima_kernel, dim3(blocks_of(interior, vgso::kThreads), (unsigned)n), dim3(vgso::kThreads), 0, s->stream,
                       (const int64_t *)s->d_resp.get(), s->w, s->h, s->cand_cap, s->d_cand_r.get(), s->d_cand_i.get(), s->d_cand_n.get());
    vgso::SelectArgs a;
    a.img = img;
    a.cand_r = s->d_cand_r.get();
    a.cand_i = s->d_cand_i.get();
    a.cand_n = s->d_cand_n.get();
    a.weights = s->d_static.get();
    a.keypoints = keypoints;
    a.descriptors = descriptors;
    a.count = s->d_count.get();
    a.cap = s->cand_cap;
    a.w = s->w;
    a.h = s->h;
    a.max_features = s->prm.max_features;
    hipLaunchKernelGGL(vgso::select_kernel, dim3((unsigned)n), dim3(vgso::kSelectThreads), 0, s->stream, a);
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(s->h_count.get(), s->d_count.get(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    if (const int rc = call.finish()) return rc;
    std::memcpy(count, s->h_count.get(), (size_t)n * sizeof(int32_t));
    return VG_OK;
}

// match of n pairs; the counts HOST.  Synchronous.
int run_match(vg_sparse_odom *s, int64_t n, const int32_t *count1, const float *desc1, const int32_t *count2, const float *desc2, int32_t *match_count,
              int32_t *matches, double *distance)
{
    const int F = s->prm.max_features;
    int k1 = 0, k2 = 0;
    for (int64_t i = 0; i < n; i++) {
        k1 = std::max(k1, count1[i]);
        k2 = std::max(k2, count2[i]);
    }
    if (k1 == 0 || k2 == 0) {   // an empty side everywhere: nothing to launch
        for (int64_t i = 0; i < n; i++) match_count[i] = 0;
        return VG_OK;
    }
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (const int rc = s->d_dist.grow((size_t)(2 * n) * F * F, "the sparse odometry scratch")) return rc;
    if (const int rc = s->d_nn.grow((size_t)(2 * n) * F, "the sparse odometry scratch")) return rc;
    if (const int rc = s->d_cnt.grow((size_t)(3 * n), "the sparse odometry scratch")) return rc;
    if (const int rc = s->h_count.grow((size_t)(3 * n), "the sparse odometry staging")) return rc;
    std::memcpy(s->h_count.get(), count1, (size_t)n * sizeof(int32_t));
    std::memcpy(s->h_count.get() + n, count2, (size_t)n * sizeof(int32_t));
    VG_HIP(hipMemcpyAsync(s->d_cnt.get(), s->h_count.get(), (size_t)(2 * n) * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    vgso::MatchArgs a;
    a.desc1 = desc1;
    a.desc2 = desc2;
    a.count1 = s->d_cnt.get();
    a.count2 = s->d_cnt.get() + n;
    a.dist = s->d_dist.get();
    a.dist_t = s->d_dist.get() + n * F * F;
    a.nn1 = s->d_nn.get();
    a.nn2 = s->d_nn.get() + n * F;
    a.matches = matches;
    a.distance = distance;
    a.match_count = s->d_cnt.get() + 2 * n;
    a.threshold = s->prm.match_threshold;
    a.max_features = F;
    hipLaunchKernelGGL(vgso::distance_kernel, dim3(blocks_of(k2, vgso::kTile), blocks_of(k1, vgso::kTile), (unsigned)n), dim3(vgso::kTile, vgso::kTile), 0,
                       s->stream, a);
    hipLaunchKernelGGL(vgso::nearest_kernel, dim3(blocks_of(std::max(k1, k2), vgso::kThreads), 2, (unsigned)n), dim3(vgso::kThreads), 0, s->stream, a);
    hipLaunchKernelGGL(vgso::cross_check_kernel, dim3((unsigned)n), dim3(64), 0, s->stream, a);
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(s->h_count.get() + 2 * n, s->d_cnt.get() + 2 * n, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    if (const int rc = call.finish()) return rc;
    std::memcpy(match_count, s->h_count.get() + 2 * n, (size_t)n * sizeof(int32_t));
    return VG_OK;
}

// what every problem of a call shares: the prior's A and J, the camera, xi_base_cam with its constants, the odometry increment
int upload_consts(vg_sparse_odom *s, const double *xi_odom)
{
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (const int rc = s->d_consts.grow(vgso::kConstDoubles, "the sparse odometry scratch")) return rc;
    if (const int rc = s->h_out.grow(vgso::kConstDoubles, "the sparse odometry staging")) return rc;
    const vg_sparse_odom_params &p = s->prm;
    const vgmp::MotionPrior prior = vgmp::make_prior(xi_odom, p.prior_err_v, p.prior_err_w, p.prior_lambda_t, p.prior_lambda_r);
    double *c = s->h_out.get();
    std::memcpy(c + vgso::kConstA, prior.A, sizeof prior.A);
    std::memcpy(c + vgso::kConstJ, prior.J, sizeof prior.J);
    std::memcpy(c + vgso::kConstCam, s->cam, sizeof s->cam);
    std::memcpy(c + vgso::kConstXb, s->xbc, sizeof s->xbc);
    vg::base_const(s->xbc, c + vgso::kConstBase);
    std::memcpy(c + vgso::kConstOdom, xi_odom, sizeof(double) * 6);
    VG_HIP(hipMemcpyAsync(s->d_consts.get(), c, vgso::kConstDoubles * sizeof(double), hipMemcpyHostToDevice, s->stream));
    return call.finish();   // the staging block is reused by the solve's results
}

// n_blocks problems in one launch; offsets HOST, index HOST (may be NULL), the points DEVICE.  Results in h_out
// ([n_blocks][kSolveOut]).  Synchronous.  upload_consts first.
int run_solve(vg_sparse_odom *s, int64_t n_blocks, const int64_t *offsets, const int32_t *index, const double *x1, const double *x2, const double *p2,
              const double *size)
{
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (const int rc = s->d_offsets.grow((size_t)n_blocks + 1, "the sparse odometry scratch")) return rc;
    if (const int rc = s->d_out.grow((size_t)n_blocks * vgso::kSolveOut, "the sparse odometry scratch")) return rc;
    if (const int rc = s->h_out.grow(std::max<size_t>((size_t)n_blocks * vgso::kSolveOut, vgso::kConstDoubles), "the sparse odometry staging")) return rc;
    const int64_t entries = offsets[n_blocks];
    if (index)
        if (const int rc = s->d_index.grow((size_t)std::max<int64_t>(entries, 1), "the sparse odometry scratch")) return rc;
    VG_HIP(hipMemcpyAsync(s->d_offsets.get(), offsets, (size_t)(n_blocks + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s->stream));
    if (index && entries > 0) VG_HIP(hipMemcpyAsync(s->d_index.get(), index, (size_t)entries * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    vgso::SolveArgs a;
    a.consts = s->d_consts.get();
    a.x1 = x1;
    a.x2 = x2;
    a.p2 = p2;
    a.size = size;
    a.index = index ? s->d_index.get() : nullptr;
    a.offsets = s->d_offsets.get();
    a.out = s->d_out.get();
    a.rule = vglm6::ceres_defaults(s->prm.max_lm_iterations);   // computeTransfSparse leaves Ceres' defaults in place but for the cap
    hipLaunchKernelGGL(vgso::solve_kernel, dim3((unsigned)n_blocks), dim3(64), 0, s->stream, a);
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(s->h_out.get(), s->d_out.get(), (size_t)n_blocks * vgso::kSolveOut * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    return call.finish();
}

// the camera motion xi_c = xi_base_cam^-1 o xi o xi_base_cam
void camera_motion(const vg_sparse_odom *s, const double *xi, double *out6)
{
    double rel[6];
    vgth::inverse_compose(s->xbc, xi, rel);
    vgth::compose(rel, s->xbc, out6);
}

// n_hyp poses scored on m matches (index HOST [m] into the point arrays, or NULL); residual DEVICE or NULL; the counts in
// h_inliers.  Synchronous.
int run_score(vg_sparse_odom *s, int64_t n_hyp, const double *xi, int64_t m, const int32_t *index, const double *x1, const double *x2, const double *p2,
              double *residual)
{
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (const int rc = s->d_frames.grow((size_t)n_hyp * vgso::kScoreFrame, "the sparse odometry scratch")) return rc;
    if (const int rc = s->d_inliers.grow((size_t)n_hyp, "the sparse odometry scratch")) return rc;
    if (const int rc = s->h_inliers.grow((size_t)n_hyp, "the sparse odometry staging")) return rc;
    if (const int rc = s->h_res.grow((size_t)n_hyp * vgso::kScoreFrame, "the sparse odometry staging")) return rc;
    if (index)
        if (const int rc = s->d_index.grow((size_t)m, "the sparse odometry scratch")) return rc;
    double *f = s->h_res.get();
    for (int64_t k = 0; k < n_hyp; k++, f += vgso::kScoreFrame) {
        double c[6];   // t | R | Rinv of the camera motion
        camera_motion(s, xi + 6 * k, c);
        vgth::inverse_frame(c, f + 12, f, f + 3);
    }
    VG_HIP(hipMemcpyAsync(s->d_frames.get(), s->h_res.get(), (size_t)n_hyp * vgso::kScoreFrame * sizeof(double), hipMemcpyHostToDevice, s->stream));
    if (index) VG_HIP(hipMemcpyAsync(s->d_index.get(), index, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
    VG_HIP(hipMemsetAsync(s->d_inliers.get(), 0, (size_t)n_hyp * sizeof(int32_t), s->stream));
    vgso::ScoreArgs a;
    a.frames = s->d_frames.get();
    a.cam = s->d_static.get() + vgso::kDesc;
    a.x1 = x1;
    a.x2 = x2;
    a.p2 = p2;
    a.index = index ? s->d_index.get() : nullptr;
    a.residual = residual;
    a.inliers = s->d_inliers.get();
    a.threshold = s->prm.inlier_threshold;
    a.m = (int)m;
    hipLaunchKernelGGL(vgso::score_kernel, dim3(blocks_of(m, vgso::kThreads), (unsigned)n_hyp), dim3(vgso::kThreads), 0, s->stream, a);
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(s->h_inliers.get(), s->d_inliers.get(), (size_t)n_hyp * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    return call.finish();
}

// residual row (DEVICE [m]) to h_res.  Synchronous.
int fetch_residuals(vg_sparse_odom *s, const double *row, int64_t m)
{
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (const int rc = s->h_res.grow((size_t)m, "the sparse odometry staging")) return rc;
    VG_HIP(hipMemcpyAsync(s->h_res.get(), row, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    return call.finish();
}

// ransacNPoints and the two refinements of feedData on m matches (DEVICE); samples HOST [iterations][points], every index in
// [0, m).  report: VG_SPARSE_ODOM_REPORT doubles.
int run_ransac(vg_sparse_odom *s, int64_t m, const double *x1, const double *x2, const double *p2, const double *size, const double *xi_odom,
               const int32_t *samples, double *xi_incr, uint8_t *mask, double *report)
{
    const int iters = s->prm.ransac_iterations, np = s->prm.num_ransac_points;
    double rep[VG_SPARSE_ODOM_REPORT] = {-1., 0., 0., 0., VG_TERM_NO_CONVERGENCE, 0., VG_TERM_NO_CONVERGENCE, VG_SPARSE_ODOM_OK};
    auto finish = [&](int status) {
        rep[7] = status;
        if (report) std::memcpy(report, rep, sizeof rep);
        return VG_OK;
    };
    std::memcpy(xi_incr, xi_odom, sizeof(double) * 6);
    if (mask && m > 0) VG_HIP(hipMemsetAsync(mask, 0, (size_t)m, s->stream));
    if (m < np) {
        VG_HIP(hipStreamSynchronize(s->stream));
        return finish(VG_SPARSE_ODOM_TOO_FEW_MATCHES);
    }
    if (const int rc = upload_consts(s, xi_odom)) return rc;
    // 4. the hypotheses: one launch of `iters` problems of `np` points, one launch that scores them all
    std::vector<int64_t> offsets((size_t)iters + 1);
    for (int k = 0; k <= iters; k++) offsets[(size_t)k] = (int64_t)k * np;
    if (const int rc = run_solve(s, iters, offsets.data(), samples, x1, x2, p2, size)) return rc;
    std::vector<double> xi((size_t)iters * 6);
    for (int k = 0; k < iters; k++) std::memcpy(&xi[(size_t)k * 6], s->h_out.get() + (size_t)k * vgso::kSolveOut, sizeof(double) * 6);
    if (const int rc = s->d_res.grow((size_t)iters * m, "the sparse odometry scratch")) return rc;
    if (const int rc = run_score(s, iters, xi.data(), m, nullptr, x1, x2, p2, s->d_res.get())) return rc;
    int best = -1, count = np;
    for (int k = 0; k < iters; k++)
        if (s->h_inliers.get()[k] > count) {
            count = s->h_inliers.get()[k];
            best = k;
        }
    if (best < 0) return finish(VG_SPARSE_ODOM_NO_HYPOTHESIS);
    rep[0] = best;
    rep[1] = count;
    if (const int rc = fetch_residuals(s, s->d_res.get() + (size_t)best * m, m)) return rc;
    std::vector<int32_t> inl;
    std::vector<uint8_t> hmask((size_t)m);
    for (int64_t i = 0; i < m; i++) {
        hmask[(size_t)i] = s->h_res.get()[i] < s->prm.inlier_threshold ? 1 : 0;
        if (hmask[(size_t)i]) inl.push_back((int32_t)i);
    }
    if (mask) {
        VG_HIP(hipMemcpyAsync(mask, hmask.data(), (size_t)m, hipMemcpyHostToDevice, s->stream));
        VG_HIP(hipStreamSynchronize(s->stream));
    }
    // 5. refinement on the inliers, the sigma gate on their reprojection under the ODOMETRY's camera motion (the reference
    // passes dxi, not the refined pose: sparse_odom.cpp:354-355), and the solve on what passes
    int64_t one[2] = {0, (int64_t)inl.size()};
    if (const int rc = run_solve(s, 1, one, inl.data(), x1, x2, p2, size)) return rc;
    rep[3] = s->h_out.get()[8];
    rep[4] = s->h_out.get()[9];
    if (const int rc = s->d_res.grow((size_t)std::max<int64_t>((int64_t)iters * m, (int64_t)inl.size()), "the sparse odometry scratch")) return rc;
    if (const int rc = run_score(s, 1, xi_odom, (int64_t)inl.size(), inl.data(), x1, x2, p2, s->d_res.get())) return rc;
    if (const int rc = fetch_residuals(s, s->d_res.get(), (int64_t)inl.size())) return rc;
    double acc = 0.;
    std::vector<double> err(inl.size());
    for (size_t i = 0; i < inl.size(); i++) {
        err[i] = s->h_res.get()[i] * s->h_res.get()[i];
        acc += err[i];
    }
    const double sigma_sq = acc / ((double)inl.size() - 2.);   // 2 degrees of freedom
    std::vector<int32_t> kept;
    for (size_t i = 0; i < inl.size(); i++)
        if (err[i] < s->prm.outlier_gate * sigma_sq) kept.push_back(inl[i]);
    rep[2] = (double)kept.size();
    one[1] = (int64_t)kept.size();
    if (const int rc = run_solve(s, 1, one, kept.data(), x1, x2, p2, size)) return rc;
    std::memcpy(xi_incr, s->h_out.get(), sizeof(double) * 6);
    rep[5] = s->h_out.get()[8];
    rep[6] = s->h_out.get()[9];
    return finish(VG_SPARSE_ODOM_OK);
}

int check_samples(const vg_sparse_odom *s, const int32_t *samples, int64_t m)
{
    const int64_t n = (int64_t)s->prm.ransac_iterations * s->prm.num_ransac_points;
    for (int64_t i = 0; i < n; i++)
        if (samples[i] < 0 || samples[i] >= m) return fail(VG_ERR_INVALID_ARGUMENT, "sample index out of range");
    return VG_OK;
}

}  // namespace

extern "C" {

void vg_sparse_odom_params_default(vg_sparse_odom_params *p)
{
    if (!p) return;
    p->max_features = 500;         // NUM_FEATURES (sparse_odom.cpp:194)
    p->match_threshold = 2500.;    // distThresh (sparse_odom.h:110)
    p->num_ransac_points = 2;      // numRansacPoints (sparse_odom.h:47)
    p->ransac_iterations = 200;    // maxIteration (sparse_odom.cpp:517)
    p->inlier_threshold = 1.;      // thresh (:518)
    p->max_lm_iterations = 25;     // :462
    p->prior_err_v = 0.03;         // OdometryPrior(0.03, 0.5, 0.03, 0.05, xiOdom) (:448)
    p->prior_err_w = 0.5;
    p->prior_lambda_t = 0.03;
    p->prior_lambda_r = 0.05;
    p->outlier_gate = 3.6;         // :375
    p->min_stereo_base = 0.;
}

int vg_sparse_odom_create(vg_sparse_odom **out, int device, void *hip_stream, const double *eucm, const double *xi_base_cam, int width, int height,
                          const vg_sparse_odom_params *params)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (!eucm || !xi_base_cam || !params) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    const vg_sparse_odom_params &p = *params;
    if (width < 2 * vgso::kBorder + 1 || height < 2 * vgso::kBorder + 1 || width > 16384 || height > 16384)
        return fail(VG_ERR_INVALID_ARGUMENT, "the image size must be in [15, 16384]");
    if (p.max_features < 1 || p.max_features > vgso::kMaxFeatures) return fail(VG_ERR_INVALID_ARGUMENT, "max_features must be in [1, 1024]");
    if (p.num_ransac_points < 2 || p.num_ransac_points > 16) return fail(VG_ERR_INVALID_ARGUMENT, "num_ransac_points must be in [2, 16]");
    if (p.ransac_iterations < 1 || p.ransac_iterations > vgi::kMaxItems) return fail(VG_ERR_INVALID_ARGUMENT, "ransac_iterations must be in [1, 65535]");
    if (p.max_lm_iterations < 0 || p.max_lm_iterations > 10000) return fail(VG_ERR_INVALID_ARGUMENT, "max_lm_iterations must be in [0, 10000]");
    if (!(p.match_threshold >= 0.) || !(p.inlier_threshold > 0.) || !(p.outlier_gate > 0.) || !(p.min_stereo_base >= 0.) || !std::isfinite(p.match_threshold) ||
        !std::isfinite(p.inlier_threshold) || !std::isfinite(p.outlier_gate) || !std::isfinite(p.min_stereo_base))
        return fail(VG_ERR_INVALID_ARGUMENT, "match_threshold, min_stereo_base must be >= 0, inlier_threshold, outlier_gate > 0, all finite");
    if (!(p.prior_err_v > 0.) || !(p.prior_err_w > 0.) || !(p.prior_lambda_t > 0.) || !(p.prior_lambda_r > 0.) || !std::isfinite(p.prior_err_v) ||
        !std::isfinite(p.prior_err_w) || !std::isfinite(p.prior_lambda_t) || !std::isfinite(p.prior_lambda_r))
        return fail(VG_ERR_INVALID_ARGUMENT, "the prior's four constants must be positive and finite");
    if (!vgsh::finite_n(xi_base_cam, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "xi_base_cam must be finite");
    if (const int rc = vgsh::check_camera(eucm)) return rc;
    std::unique_ptr<vg_sparse_odom> s(new (std::nothrow) vg_sparse_odom());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    for (int i = 0; i < 6; i++) {
        s->cam[i] = eucm[i];
        s->xbc[i] = xi_base_cam[i];
        s->odom_prev[i] = s->xi_local[i] = s->xi_incr[i] = 0.;
    }
    s->w = width;
    s->h = height;
    s->prm = p;
    s->cand_cap = (int64_t)((width - 2 * vgso::kBorder + 1) / 2) * ((height - 2 * vgso::kBorder + 1) / 2);
    if (const int rc = s->open(device, hip_stream, "sparse odometry")) return rc;
    vgi::Call call(s.get());   // a failure below drains the stream before s is freed
    if (const int rc = call.begin()) return rc;
    double st[vgso::kDesc + 6];   // descriptors' kernel (sparse_odom.cpp:211-221): one table of std::exp values
    int q = 0;
    for (int v = -vgso::kPatch; v <= vgso::kPatch; v++) {
        const double y = (2. * v) / vgso::kPatch;
        for (int u = -vgso::kPatch; u <= vgso::kPatch; u++, q++) {
            const double x = (2. * u) / vgso::kPatch;
            st[q] = std::exp(-0.5 * (x * x + y * y));
        }
    }
    for (int i = 0; i < 6; i++) st[vgso::kDesc + i] = eucm[i];
    if (const int rc = s->d_static.grow(vgso::kDesc + 6, "the sparse odometry scratch")) return rc;
    VG_HIP(hipMemcpyAsync(s->d_static.get(), st, sizeof st, hipMemcpyHostToDevice, s->stream));
    if (const int rc = call.finish()) return rc;
    *out = s.release();
    return VG_OK;
}

void vg_sparse_odom_destroy(vg_sparse_odom *s) { vgi::destroy(s); }

int vg_sparse_odom_response(vg_sparse_odom *s, int64_t n, const uint8_t *img, int64_t *response)
{
    if (const int rc = check_handle(s)) return rc;
    if (const int rc = vgi::check_items(n, 1, "image")) return rc;
    if (!img || !response) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (const int rc = launch_response(s, n, img, response)) return rc;
    return call.finish();
}

int vg_sparse_odom_detect(vg_sparse_odom *s, int64_t n, const uint8_t *img, int32_t *count, int32_t *keypoints, float *descriptors)
{
    if (const int rc = check_handle(s)) return rc;
    if (const int rc = vgi::check_items(n, 1, "image")) return rc;
    if (!img || !count || !keypoints || !descriptors) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    return run_detect(s, n, img, count, keypoints, descriptors);
}

int vg_sparse_odom_match(vg_sparse_odom *s, int64_t n, const int32_t *count1, const float *descriptors1, const int32_t *count2,
                         const float *descriptors2, int32_t *match_count, int32_t *matches, double *distance)
{
    if (const int rc = check_handle(s)) return rc;
    if (const int rc = vgi::check_items(n, 1, "pair")) return rc;
    if (!count1 || !descriptors1 || !count2 || !descriptors2 || !match_count || !matches || !distance) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int64_t i = 0; i < n; i++)
        if (count1[i] < 0 || count1[i] > s->prm.max_features || count2[i] < 0 || count2[i] > s->prm.max_features)
            return fail(VG_ERR_INVALID_ARGUMENT, "a feature count must be in [0, max_features]");
    return run_match(s, n, count1, descriptors1, count2, descriptors2, match_count, matches, distance);
}

int vg_sparse_odom_solve(vg_sparse_odom *s, int64_t n_blocks, const int64_t *offsets, const double *x1, const double *x2, const double *p2,
                         const double *size, const double *xi_odom, double *xi_out, double *report)
{
    if (const int rc = check_handle(s)) return rc;
    if (n_blocks < 1 || n_blocks > kMaxPoints) return fail(VG_ERR_INVALID_ARGUMENT, "the block count must be in [1, 2^20]");
    if (!offsets || !xi_odom || !xi_out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (offsets[0] != 0) return fail(VG_ERR_INVALID_ARGUMENT, "offsets[0] must be 0");
    for (int64_t b = 0; b < n_blocks; b++)
        if (offsets[b + 1] < offsets[b]) return fail(VG_ERR_INVALID_ARGUMENT, "offsets must not decrease");
    if (offsets[n_blocks] > kMaxPoints) return fail(VG_ERR_INVALID_ARGUMENT, "at most 2^20 points in one call");
    if (offsets[n_blocks] > 0 && (!x1 || !x2 || !p2 || !size)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi_odom, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "the odometry increment must be finite");
    if (const int rc = upload_consts(s, xi_odom)) return rc;
    if (const int rc = run_solve(s, n_blocks, offsets, nullptr, x1, x2, p2, size)) return rc;
    for (int64_t b = 0; b < n_blocks; b++) {
        const double *o = s->h_out.get() + b * vgso::kSolveOut;
        std::memcpy(xi_out + 6 * b, o, sizeof(double) * 6);
        if (report) std::memcpy(report + 4 * b, o + 6, sizeof(double) * 4);
    }
    return VG_OK;
}

int vg_sparse_odom_score(vg_sparse_odom *s, int64_t n_hyp, const double *xi, int64_t m, const double *x1, const double *x2, const double *p2,
                         double *residual, int32_t *inliers)
{
    if (const int rc = check_handle(s)) return rc;
    if (const int rc = vgi::check_items(n_hyp, 1, "hypothesis")) return rc;
    if (m < 0 || m > kMaxPoints) return fail(VG_ERR_INVALID_ARGUMENT, "the match count must be in [0, 2^20]");
    if (!xi || !inliers || (m > 0 && (!x1 || !x2 || !p2))) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi, 6 * (int)n_hyp)) return fail(VG_ERR_INVALID_ARGUMENT, "the poses must be finite");
    if (m == 0) {
        for (int64_t k = 0; k < n_hyp; k++) inliers[k] = 0;
        return VG_OK;
    }
    if (const int rc = run_score(s, n_hyp, xi, m, nullptr, x1, x2, p2, residual)) return rc;
    std::memcpy(inliers, s->h_inliers.get(), (size_t)n_hyp * sizeof(int32_t));
    return VG_OK;
}

int vg_sparse_odom_draw_samples(vg_sparse_odom *s, int64_t m, int32_t *samples)
{
    if (const int rc = check_handle(s)) return rc;
    if (!samples) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (m < s->prm.num_ransac_points || m > kMaxPoints) return fail(VG_ERR_INVALID_ARGUMENT, "the match count must be in [num_ransac_points, 2^20]");
    draw_samples(s, m, samples);
    return VG_OK;
}

int vg_sparse_odom_ransac(vg_sparse_odom *s, int64_t m, const double *x1, const double *x2, const double *p2, const double *size, const double *xi_odom,
                          const int32_t *samples, double *xi_incr, uint8_t *mask, double *report)
{
    if (const int rc = check_handle(s)) return rc;
    if (m < 0 || m > kMaxPoints) return fail(VG_ERR_INVALID_ARGUMENT, "the match count must be in [0, 2^20]");
    if (!xi_odom || !xi_incr || (m > 0 && (!x1 || !x2 || !p2 || !size))) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi_odom, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "the odometry increment must be finite");
    std::vector<int32_t> drawn;
    if (m >= s->prm.num_ransac_points) {
        if (samples) {
            if (const int rc = check_samples(s, samples, m)) return rc;
        } else {
            drawn.resize((size_t)s->prm.ransac_iterations * s->prm.num_ransac_points);
            draw_samples(s, m, drawn.data());
            samples = drawn.data();
        }
    }
    VG_HIP(hipSetDevice(s->device));
    return run_ransac(s, m, x1, x2, p2, size, xi_odom, samples, xi_incr, mask, report);
}

int vg_sparse_odom_feed(vg_sparse_odom *s, const uint8_t *img, const double *xi_odom_new, const int32_t *samples, double *xi_incr, double *report)
{
    if (const int rc = check_handle(s)) return rc;
    if (!img || !xi_odom_new) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi_odom_new, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "the odometry pose must be finite");
    const int F = s->prm.max_features, iters = s->prm.ransac_iterations, np = s->prm.num_ransac_points;
    for (int64_t i = 0; samples && i < (int64_t)iters * np; i++)
        if (samples[i] < 0) return fail(VG_ERR_INVALID_ARGUMENT, "sample index out of range");
    double rep[VG_SPARSE_ODOM_FEED_REPORT] = {0.};
    auto finish = [&](int state) {
        rep[0] = state;
        if (xi_incr) std::memcpy(xi_incr, s->xi_incr, sizeof s->xi_incr);
        if (report) std::memcpy(report, rep, sizeof rep);
        return VG_OK;
    };
    double odom_incr[6];
    vgth::inverse_compose(s->odom_prev, xi_odom_new, odom_incr);
    if (s->has_prev && s->n_kp[s->cur] > 0) {   // the skip rule (sparse_odom.cpp:242-244)
        double dxi[6];
        camera_motion(s, odom_incr, dxi);
        if (vg::norm3(dxi) < s->prm.min_stereo_base) return finish(VG_SPARSE_ODOM_SKIPPED);
    }
    VG_HIP(hipSetDevice(s->device));
    const int nxt = 1 - s->cur;
    if (const int rc = s->d_kp[nxt].grow((size_t)F * 2, "the sparse odometry scratch")) return rc;
    if (const int rc = s->d_desc[nxt].grow((size_t)F * vgso::kDesc, "the sparse odometry scratch")) return rc;
    int32_t n_new = 0;
    if (const int rc = run_detect(s, 1, img, &n_new, s->d_kp[nxt].get(), s->d_desc[nxt].get())) return rc;
    s->n_kp[nxt] = n_new;
    rep[1] = n_new;
    int state = VG_SPARSE_ODOM_FIRST;
    if (s->has_prev && s->n_kp[s->cur] > 0) {
        state = VG_SPARSE_ODOM_ESTIMATED;
        if (const int rc = s->d_matches.grow((size_t)F * 2, "the sparse odometry scratch")) return rc;
        if (const int rc = s->d_distance.grow((size_t)F, "the sparse odometry scratch")) return rc;
        if (const int rc = s->d_rays.grow((size_t)F * 9, "the sparse odometry scratch")) return rc;
        if (const int rc = s->d_mask.grow((size_t)F, "the sparse odometry scratch")) return rc;
        int32_t m = 0, n_old = s->n_kp[s->cur];
        if (const int rc = run_match(s, 1, &n_old, s->d_desc[s->cur].get(), &n_new, s->d_desc[nxt].get(), &m, s->d_matches.get(), s->d_distance.get()))
            return rc;
        rep[2] = m;
        double *x1 = s->d_rays.get(), *x2 = x1 + 3 * F, *p2 = x2 + 3 * F, *size = p2 + 2 * F;
        if (m > 0) {
            hipLaunchKernelGGL(vgso::rays_kernel, dim3(blocks_of(m, vgso::kThreads)), dim3(vgso::kThreads), 0, s->stream,
                               (const double *)(s->d_static.get() + vgso::kDesc), (const int32_t *)s->d_kp[s->cur].get(), (const int32_t *)s->d_kp[nxt].get(),
                               (const int32_t *)s->d_matches.get(), (int)m, x1, x2, p2, size);
            VG_HIP(hipGetLastError());
        }
        std::vector<int32_t> table;
        if (m >= np) {
            table.resize((size_t)iters * np);
            if (samples)
                for (size_t i = 0; i < table.size(); i++) table[i] = samples[i] % m;   // a given table is folded onto the matches found
            else
                draw_samples(s, m, table.data());
        }
        if (const int rc = run_ransac(s, m, x1, x2, p2, size, odom_incr, table.empty() ? nullptr : table.data(), s->xi_incr, s->d_mask.get(), rep + 4))
            return rc;
        vgth::compose(s->xi_local, s->xi_incr, s->xi_local);   // xiLocal = xiLocal.compose(xiIncr)
    }
    s->cur = nxt;   // refresh state (:432-436)
    s->has_prev = true;
    std::memcpy(s->odom_prev, xi_odom_new, sizeof(double) * 6);
    return finish(state);
}

int vg_sparse_odom_increment(const vg_sparse_odom *s, double *xi6)
{
    if (!s || !xi6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    std::memcpy(xi6, s->xi_incr, sizeof s->xi_incr);
    return VG_OK;
}

int vg_sparse_odom_integrated(const vg_sparse_odom *s, double *xi6)
{
    if (!s || !xi6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    std::memcpy(xi6, s->xi_local, sizeof s->xi_local);
    return VG_OK;
}

}  // extern "C"
