// vg_mono_odom_tu.hip -- translation unit of libvisgeom_amd.so: monocular visual odometry (section 15 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_mono_odom handle is the reference's MonoOdometry.  The four pipelines it owns, its three map triples, the stage steps of
// a frame and the small entries are the frame-loop core it shares with vg_mapping (vg_frame_loop.hpp).  Here: the key image, the
// global pose, the key frame increments and MonoOdometry's state machine -- a new key frame's SGM map is not noise-filtered, the
// photometric key frame is set anew for every solve, xi_local is reset at commit.  A frame works on copies of the poses, writes
// its maps into the scratch triples and commits when its last stage has succeeded.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "vg_frame_loop.hpp"
#include "vg_mono_odom.hpp"

using vgmo::Array6d;

struct vg_mono_odom : vgmo::FrameLoop {
    vg_mono_odom_params prm;
    int state = vgmo::kBegin;
    Array6d xi_global{};
    std::vector<Array6d> transf;   // transfVec
    vgi::Grow<uint8_t> d_key;      // the key image
};

namespace {

using vgi::fail;
using vgmo::load6;
using vgmo::store6;
using vgsh::blocks_of;

int check_thresholds(const vg_mono_odom_params &p)
{
    const double v[5] = {p.min_init_dist, p.max_dist, p.max_angle, p.min_scale_length, p.max_scale_ratio};
    if (!vgsh::finite_n(v, 5)) return fail(VG_ERR_INVALID_ARGUMENT, "the thresholds must be finite");
    if (p.min_init_dist < 0 || p.max_dist < 0 || p.max_angle < 0 || p.min_scale_length < 0)
        return fail(VG_ERR_INVALID_ARGUMENT, "min_init_dist, max_dist, max_angle and min_scale_length must not be negative");
    if (!(p.max_scale_ratio > 0)) return fail(VG_ERR_INVALID_ARGUMENT, "max_scale_ratio must be positive");
    return VG_OK;
}

// what pushKeyFrame leaves behind, committed by feed_image once every stage has succeeded
struct Frame {
    Array6d xi_local, xi_local_old, xi_global;
    int state;
    bool pushed = false;
    double counts[6] = {0, 0, 0, 0, 0, 0};
};

// pushKeyFrame (:175-216) with the pose xi_local of the new image; the maps are written into the scratch triples and
// *new_slot names the triple that becomes the map
int push_keyframe(vg_mono_odom *s, const uint8_t *img, Frame &f, int *new_slot)
{
    const Array6d motion = vgmo::camera_motion(s->xi_base_cam, f.xi_local);
    if (const int rc = vgmo::sgm_map(s, motion, img, s->d_key, false)) return rc;   // computeStereo(imageNew, imageVec.back()), not filtered
    *new_slot = 1;
    if (s->state == vgmo::kReady) {   // the prior map carried into the new frame, the SGM map merged into it
        if (const int rc = vgmo::warp_map(s, motion)) return rc;
        if (const int rc = vgmo::merge_maps(s, f.counts)) return rc;
        *new_slot = 2;
    }
    f.xi_global = vgth::compose(f.xi_global, f.xi_local);
    f.pushed = true;
    return VG_OK;
}

// the new image becomes the key image of the handle and of motion stereo, the triple new_slot the map and the frame's
// poses the handle's.  The two device steps come first: they are the only ones here that can fail.
int commit(vg_mono_odom *s, const uint8_t *img, const Frame &f, int new_slot, bool new_key)
{
    if (new_key) {
        if (const int rc = vgmo::copy_image(s, s->d_key, img)) return rc;
        if (const int rc = vg_motion_stereo_set_base(s->motion, 1, s->d_key)) return rc;
    }
    s->map_slot = (s->map_slot + new_slot) % 3;
    if (f.pushed) {
        s->transf.push_back(f.xi_local);
        s->xi_local = Array6d{};
        s->have_map = true;
    } else {
        s->xi_local = f.xi_local;
    }
    s->xi_local_old = f.xi_local_old;
    s->xi_global = f.xi_global;
    s->state = f.state;
    return VG_OK;
}

}  // namespace

extern "C" {

void vg_mono_odom_params_default(vg_mono_odom_params *p)
{
    if (!p) return;
    p->min_init_dist = 0.25;
    p->max_dist = 0.4;
    p->max_angle = M_PI / 4;
    p->min_scale_length = 1e-2;
    p->max_scale_ratio = 1.2;
    p->num_scales = 5;
    vg_motion_stereo_params_default(&p->motion);
    vg_sparse_odom_params_default(&p->sparse);
}

int vg_mono_odom_create(vg_mono_odom **out, int device, void *hip_stream, const double *eucm, const double *xi_base_cam, int width,
                        int height, const vg_mono_odom_params *params)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (!eucm || !xi_base_cam || !params) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = check_thresholds(*params)) return rc;
    std::unique_ptr<vg_mono_odom> s(new (std::nothrow) vg_mono_odom());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    s->prm = *params;
    if (const int rc = vgmo::open_loop(s.get(), device, hip_stream, eucm, xi_base_cam, width, height, params->motion, params->sparse,
                                       params->num_scales, "monocular odometry"))
        return rc;
    if (const int rc = s->d_key.grow((size_t)s->img, "the key image")) return rc;
    *out = s.release();
    return VG_OK;
}

void vg_mono_odom_destroy(vg_mono_odom *s) { vgi::destroy(s); }

int vg_mono_odom_size(const vg_mono_odom *s, int *width, int *height, int *x_max, int *y_max) { return vgmo::size(s, width, height, x_max, y_max); }

int vg_mono_odom_feed_wheel_odometry(vg_mono_odom *s, const double *xi_odom_new) { return vgmo::feed_odometry(s, xi_odom_new); }

int vg_mono_odom_feed_image(vg_mono_odom *s, const uint8_t *img, const int32_t *samples, double *report)
{
    if (!s || !img) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    Frame f;
    f.xi_local = s->xi_local;
    f.xi_local_old = s->xi_local_old;
    f.xi_global = s->xi_global;
    f.state = s->state;
    int action = vgmo::kWaiting, new_slot = 0;
    double K = 0., length = 0., length_prior = 0., photo[3] = {0., 0., 0.};
    bool new_key = false;
    switch (s->state) {
    case vgmo::kBegin: {   // the starting point, position 0
        const Array6d zero{};
        if (const int rc = vg_sparse_odom_feed(s->sparse, img, zero.data(), samples, nullptr, nullptr)) return rc;
        f.xi_local = f.xi_global = zero;
        f.state = vgmo::kSparseInit;
        action = vgmo::kFirst;
        new_key = true;
        break;
    }
    case vgmo::kSparseInit: {   // wait until the distance is sufficient for the sparse initialisation
        if (!(vgmo::norm3(f.xi_local.data()) >= s->prm.min_init_dist)) break;
        Array6d incr;
        if (const int rc = vg_sparse_odom_feed(s->sparse, img, f.xi_local.data(), samples, incr.data(), nullptr)) return rc;
        f.xi_local = f.xi_local_old = incr;
        if (const int rc = push_keyframe(s, img, f, &new_slot)) return rc;
        f.state = vgmo::kReady;
        action = vgmo::kSparseInitKeyframe;
        new_key = true;
        break;
    }
    default: {
        if (!s->have_map) return fail(VG_ERR_STATE, "READY without a depth map");
        if (const int rc = vg_photometric_set_base(s->photo, s->d_key, s->triple(0))) return rc;   // always: no set_depth shortcut
        Array6d vo;
        if (const int rc = vgmo::solve_photo(s, img, f.xi_local, vo, photo)) return rc;
        const vgmo::Scale sc = vgmo::normalize_scale(s->prm, f.xi_local_old, f.xi_local, vo);
        K = sc.K;
        length = sc.length;
        length_prior = sc.length_prior;
        f.xi_local = sc.xi;
        if (sc.discarded) {   // the reference's break: no refinement, no key frame test, xi_local_old not refreshed
            action = vgmo::kDiscarded;
            break;
        }
        f.xi_local_old = f.xi_local;
        if (vgmo::needs_keyframe(s->prm, f.xi_local)) {
            if (const int rc = push_keyframe(s, img, f, &new_slot)) return rc;
            action = vgmo::kKeyframe;
            new_key = true;
            break;
        }
        action = vgmo::kRefined;
        const Array6d motion = vgmo::camera_motion(s->xi_base_cam, f.xi_local);
        if (!vgsh::has_baseline(motion.data())) break;   // a camera that has not moved refines nothing
        if (const int rc = vgmo::refine_map(s, motion, img, f.counts)) return rc;
        new_slot = 1;   // refined into a scratch triple, which becomes the map when the frame commits
        break;
    }
    }
    const int before = s->state;
    if (const int rc = commit(s, img, f, new_slot, new_key)) return rc;
    if (action == vgmo::kFirst) s->transf.assign(1, Array6d{});   // transfVec.push_back(_xiLocal) of STATE_BEGIN
    if (report) {
        const double r[VG_MONO_ODOM_REPORT] = {(double)before, (double)s->state, (double)action, K, length, length_prior, photo[0], photo[1],
                                              photo[2], f.counts[0], f.counts[1], f.counts[2], f.counts[3], f.counts[4], f.counts[5],
                                              (double)s->transf.size()};
        std::memcpy(report, r, sizeof(r));
    }
    return VG_OK;
}

int vg_mono_odom_set_depth(vg_mono_odom *s, const float *depth_image)
{
    if (!s || !depth_image) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    double *m = s->triple(0);
    const size_t P = (size_t)s->P;
    hipLaunchKernelGGL(vgmo::mono_odom_set_depth_kernel, dim3(blocks_of(s->P, vgmo::kLanes)), dim3(vgmo::kLanes), 0, s->stream, s->view, depth_image, m,
                       m + P, s->have_map ? nullptr : m + 2 * P);
    VG_HIP(hipGetLastError());
    if (const int rc = call.finish()) return rc;
    s->have_map = true;
    return VG_OK;
}

int vg_mono_odom_warp_image(vg_mono_odom *s, const uint8_t *src, const double *xi, const double *depth, uint8_t *dst)
{
    if (!s || !src || !dst) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (xi && !vgsh::finite_n(xi, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "the pose must be finite");
    if (!depth && !s->have_map) return fail(VG_ERR_STATE, "no depth map yet: pass one, or call set_depth or feed images first");
    const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst);
    if (a < b + (size_t)s->img && b < a + (size_t)s->img) return fail(VG_ERR_INVALID_ARGUMENT, "the warp is a gather: dst must not overlap src");
    vgmo::WarpImageArgs args;
    args.v = s->view;
    vgmo::warp_image_pose(s->xi_base_cam, xi ? load6(xi) : s->xi_local, args);
    args.depth = depth ? depth : s->triple(0);
    args.src = src;
    args.dst = dst;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    hipLaunchKernelGGL(vgmo::mono_odom_warp_image_kernel, dim3(blocks_of(s->img, vgmo::kLanes)), dim3(vgmo::kLanes), 0, s->stream, args);
    VG_HIP(hipGetLastError());
    return call.finish();
}

int vg_mono_odom_state(const vg_mono_odom *s, int *state)
{
    if (!s || !state) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *state = s->state;
    return VG_OK;
}

int vg_mono_odom_xi_local(const vg_mono_odom *s, double *xi6) { return vgmo::get_pose(s, &vg_mono_odom::xi_global, xi6, 0); }
int vg_mono_odom_xi_global(const vg_mono_odom *s, double *xi6) { return vgmo::get_pose(s, &vg_mono_odom::xi_global, xi6, 1); }
int vg_mono_odom_xi_composed(const vg_mono_odom *s, double *xi6) { return vgmo::get_pose(s, &vg_mono_odom::xi_global, xi6, 2); }

int vg_mono_odom_num_keyframes(const vg_mono_odom *s, int64_t *count)
{
    if (!s || !count) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *count = (int64_t)s->transf.size();
    return VG_OK;
}

int vg_mono_odom_keyframe_increment(const vg_mono_odom *s, int64_t k, double *xi6)
{
    if (!s || !xi6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (k < 0 || k >= (int64_t)s->transf.size()) return fail(VG_ERR_INVALID_ARGUMENT, "the key frame index is out of range");
    store6(s->transf[(size_t)k], xi6);
    return VG_OK;
}

int vg_mono_odom_get_map(vg_mono_odom *s, double *depth, double *sigma, double *cost) { return vgmo::get_map(s, depth, sigma, cost, "monocular odometry handle is NULL"); }

int vg_mono_odom_map(const vg_mono_odom *s, const double **depth, const double **sigma, const double **cost) { return vgmo::map(s, depth, sigma, cost); }

int vg_mono_odom_integrate(const double *xi_local, const double *xi_odom_old, const double *xi_odom_new, double *out6)
{
    if (!xi_local || !xi_odom_old || !xi_odom_new || !out6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    store6(vgmo::integrate(load6(xi_local), load6(xi_odom_old), load6(xi_odom_new)), out6);
    return VG_OK;
}

int vg_mono_odom_normalize_scale(const vg_mono_odom_params *params, const double *xi_local_old, const double *xi_local_prior,
                                 const double *xi_local_vo, double *out6, double *K, int *discarded)
{
    if (!params || !xi_local_old || !xi_local_prior || !xi_local_vo || !out6 || !discarded) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = check_thresholds(*params)) return rc;
    const vgmo::Scale sc = vgmo::normalize_scale(*params, load6(xi_local_old), load6(xi_local_prior), load6(xi_local_vo));
    store6(sc.xi, out6);
    if (K) *K = sc.K;
    *discarded = sc.discarded ? 1 : 0;
    return VG_OK;
}

int vg_mono_odom_needs_keyframe(const vg_mono_odom_params *params, const double *xi_local, int *needed)
{
    if (!params || !xi_local || !needed) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = check_thresholds(*params)) return rc;
    *needed = vgmo::needs_keyframe(*params, load6(xi_local)) ? 1 : 0;
    return VG_OK;
}

int vg_mono_odom_camera_motion(const double *xi_base_cam, const double *xi, double *out6)
{
    if (!xi_base_cam || !xi || !out6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    store6(vgmo::camera_motion(load6(xi_base_cam), load6(xi)), out6);
    return VG_OK;
}

int vg_mono_odom_compose(const double *a6, const double *b6, double *out6)
{
    if (!a6 || !b6 || !out6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    vgth::compose(a6, b6, out6);
    return VG_OK;
}

}  // extern "C"
