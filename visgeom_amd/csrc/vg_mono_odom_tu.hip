// vg_mono_odom_tu.hip -- translation unit of libvisgeom_amd.so: monocular visual odometry (section 15 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_mono_odom handle is the reference's MonoOdometry: it owns one vg_sparse_odom, vg_motion_stereo, vg_depth_fusion and
// vg_photometric handle (through their C entries, all on the handle's stream), the key image and three map triples of its
// own -- the map, the SGM map of a new key frame and the warp's output -- and builds a vg_stereo object per key frame, whose
// geometry depends on the pose.  Between the stages of a frame only poses, counts and reports cross to the host.  A frame
// works on copies of the poses, writes its maps into the scratch triples and commits when its last stage has succeeded.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "vg_handle.hpp"
#include "vg_mono_odom.hpp"
#include "vg_stereo_host.hpp"

using vgmo::Array6d;

struct vg_mono_odom : vgi::HandleBase {
    vg_mono_odom_params prm;
    double cam[6];
    Array6d xi_base_cam;
    vgmo::View view;
    int64_t P = 0, img = 0;
    vg_sparse_odom *sparse = nullptr;
    vg_motion_stereo *motion = nullptr;
    vg_depth_fusion *fusion = nullptr;
    vg_photometric *photo = nullptr;
    int state = vgmo::kBegin;
    bool have_odom = false, have_map = false;
    Array6d xi_local{}, xi_local_old{}, xi_global{}, xi_odom{};
    std::vector<Array6d> transf;   // transfVec
    vgi::Grow<uint8_t> d_key;      // the key image
    vgi::Grow<double> d_maps;      // [3 triples][3][P]
    int map_slot = 0;              // which triple is the map; the other two are scratch
    double *triple(int k) const { return d_maps.get() + (size_t)((map_slot + k) % 3) * 3 * (size_t)P; }   // 0: the map
    ~vg_mono_odom()
    {
        vg_sparse_odom_destroy(sparse);
        vg_motion_stereo_destroy(motion);
        vg_depth_fusion_destroy(fusion);
        vg_photometric_destroy(photo);
    }
};

namespace {

using vgi::fail;
using vgsh::blocks_of;

constexpr int kMaxPyramid = 8;   // vg_photometric_create refuses more pyramid levels

Array6d load6(const double *p)
{
    Array6d a;
    std::memcpy(a.data(), p, sizeof(double) * 6);
    return a;
}

void store6(const Array6d &a, double *p) { std::memcpy(p, a.data(), sizeof(double) * 6); }

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
    const Array6d motion = vgmo::camera_motion(s->xi_base_cam, f.xi_local), inv = vgth::inverse(motion);
    double *sgm = s->triple(1), *warp = s->triple(2);
    const size_t P = (size_t)s->P;
    vg_stereo *st = nullptr;   // EnhancedSgm(getCameraMotion().inverse(), ...): computeStereo(imageNew, imageVec.back())
    if (const int rc = vg_stereo_create(&st, s->device, s->stream, s->cam, s->cam, inv.data(), &s->prm.motion.stereo)) return rc;
    const int rc = vg_stereo_compute(st, 1, img, s->d_key, sgm, sgm + P, sgm + 2 * P, nullptr);
    vg_stereo_destroy(st);
    if (rc) return rc;
    *new_slot = 1;
    if (s->state == vgmo::kReady) {   // the prior map carried into the new frame, the SGM map merged into it
        const double *map = s->triple(0);
        if (const int rc2 = vg_depth_warp(s->fusion, 1, motion.data(), map, map + P, map + 2 * P, warp, warp + P, warp + 2 * P, nullptr)) return rc2;
        int64_t mc[5];
        if (const int rc2 = vg_depth_merge(s->fusion, 1, warp, warp + P, sgm, sgm + P, mc)) return rc2;
        for (int i = 0; i < 5; i++) f.counts[i] = (double)mc[i];
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
        vgi::Call call(s);
        if (const int rc = call.begin()) return rc;
        VG_HIP(hipMemcpyAsync(s->d_key, img, (size_t)s->img, hipMemcpyDeviceToDevice, s->stream));
        if (const int rc = call.finish()) return rc;
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

int get_pose(const vg_mono_odom *s, double *xi6, int which)
{
    if (!s || !xi6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    store6(which == 0 ? s->xi_local : which == 1 ? s->xi_global : vgth::compose(s->xi_global, s->xi_local), xi6);
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
    const vg_stereo_params &sp = params->motion.stereo;
    if (width != sp.u_max || height != sp.v_max) return fail(VG_ERR_INVALID_ARGUMENT, "the image size must be uMax x vMax of the stereo parameters");
    if (!vgsh::finite_n(xi_base_cam, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "xi_base_cam must be finite");
    std::unique_ptr<vg_mono_odom> s(new (std::nothrow) vg_mono_odom());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    s->prm = *params;
    // every pipeline checks its own arguments before it asks for the device: a missing device is reported only when all
    // four have accepted theirs
    int rcs[4];
    rcs[0] = vg_motion_stereo_create(&s->motion, device, hip_stream, eucm, eucm, &params->motion);
    if (rcs[0] == VG_ERR_INVALID_ARGUMENT) return rcs[0];
    rcs[1] = vg_depth_fusion_create(&s->fusion, device, hip_stream, eucm, &sp);
    if (rcs[1] == VG_ERR_INVALID_ARGUMENT) return rcs[1];
    rcs[2] = vg_photometric_create(&s->photo, device, hip_stream, eucm, &sp, xi_base_cam, width, height, params->num_scales);
    if (rcs[2] == VG_ERR_INVALID_ARGUMENT) return rcs[2];
    rcs[3] = vg_sparse_odom_create(&s->sparse, device, hip_stream, eucm, xi_base_cam, width, height, &params->sparse);
    if (rcs[3] == VG_ERR_INVALID_ARGUMENT) return rcs[3];
    for (int i = 0; i < 4; i++)
        if (rcs[i]) return rcs[i];
    int x_max = 0, y_max = 0;
    if (const int rc = vg_motion_stereo_size(s->motion, &x_max, &y_max)) return rc;
    s->prm.motion.stereo.x_max = x_max;   // equal_margins resolved once, for the per-key-frame SGM objects too
    s->prm.motion.stereo.y_max = y_max;
    s->prm.motion.stereo.equal_margins = 0;
    for (int i = 0; i < 6; i++) s->cam[i] = s->view.cam[i] = eucm[i];
    s->xi_base_cam = load6(xi_base_cam);
    s->view.g = vgmo::Grid{sp.scale, sp.u0, sp.v0, x_max, y_max};
    s->view.width = width;
    s->view.height = height;
    s->P = (int64_t)x_max * y_max;
    s->img = (int64_t)width * height;
    if (const int rc = s->open(device, hip_stream, "monocular odometry")) return rc;
    VG_HIP(hipSetDevice(device));
    if (const int rc = s->d_key.grow((size_t)s->img, "the key image")) return rc;
    if (const int rc = s->d_maps.grow(9 * (size_t)s->P, "the depth maps")) return rc;
    *out = s.release();
    return VG_OK;
}

void vg_mono_odom_destroy(vg_mono_odom *s) { vgi::destroy(s); }

int vg_mono_odom_size(const vg_mono_odom *s, int *width, int *height, int *x_max, int *y_max)
{
    if (!s || !width || !height || !x_max || !y_max) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *width = s->view.width;
    *height = s->view.height;
    *x_max = s->view.g.x_max;
    *y_max = s->view.g.y_max;
    return VG_OK;
}

int vg_mono_odom_feed_wheel_odometry(vg_mono_odom *s, const double *xi_odom_new)
{
    if (!s || !xi_odom_new) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi_odom_new, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "the odometry pose must be finite");
    const Array6d xi_new = load6(xi_odom_new);
    if (s->have_odom) s->xi_local = vgmo::integrate(s->xi_local, s->xi_odom, xi_new);
    s->xi_odom = xi_new;
    s->have_odom = true;
    return VG_OK;
}

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
    const size_t P = (size_t)s->P;
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
        const double *map = s->triple(0);
        if (const int rc = vg_photometric_set_base(s->photo, s->d_key, map)) return rc;
        if (const int rc = vg_photometric_set_targets(s->photo, 1, img)) return rc;
        const int32_t target = 0;
        Array6d vo;
        double rep[4 * kMaxPyramid];
        if (const int rc = vg_photometric_compute_pose(s->photo, 1, f.xi_local.data(), &target, f.xi_local.data(), vo.data(), rep)) return rc;
        for (int i = 0; i < s->prm.num_scales; i++) photo[0] += rep[4 * (size_t)i];
        photo[1] = rep[2];
        photo[2] = rep[3];
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
        double *m = s->triple(1);   // refined into a scratch triple, which becomes the map when the frame commits
        int64_t mc[6];
        if (const int rc = vg_motion_stereo_compute(s->motion, 1, motion.data(), img, map, map + P, map + 2 * P, m, m + P, m + 2 * P, mc)) return rc;
        if (const int rc = vg_depth_filter_noise(s->fusion, 1, m, m + P, m, m + P, nullptr)) return rc;
        for (int i = 0; i < 6; i++) f.counts[i] = (double)mc[i];
        new_slot = 1;
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

int vg_mono_odom_xi_local(const vg_mono_odom *s, double *xi6) { return get_pose(s, xi6, 0); }
int vg_mono_odom_xi_global(const vg_mono_odom *s, double *xi6) { return get_pose(s, xi6, 1); }
int vg_mono_odom_xi_composed(const vg_mono_odom *s, double *xi6) { return get_pose(s, xi6, 2); }

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

int vg_mono_odom_get_map(vg_mono_odom *s, double *depth, double *sigma, double *cost)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "monocular odometry handle is NULL");
    if (!s->have_map) return fail(VG_ERR_STATE, "no depth map yet");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    double *const out[3] = {depth, sigma, cost};
    for (int i = 0; i < 3; i++)
        if (out[i]) VG_HIP(hipMemcpyAsync(out[i], s->triple(0) + (size_t)i * (size_t)s->P, (size_t)s->P * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    return call.finish();
}

int vg_mono_odom_map(const vg_mono_odom *s, const double **depth, const double **sigma, const double **cost)
{
    if (!s || !depth || !sigma || !cost) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!s->have_map) return fail(VG_ERR_STATE, "no depth map yet");
    *depth = s->triple(0);
    *sigma = s->triple(0) + s->P;
    *cost = s->triple(0) + 2 * s->P;
    return VG_OK;
}

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
    store6(vgth::compose(load6(a6), load6(b6)), out6);
    return VG_OK;
}

}  // extern "C"
