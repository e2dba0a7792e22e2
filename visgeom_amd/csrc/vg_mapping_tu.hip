// vg_mapping_tu.hip -- translation unit of libvisgeom_amd.so: photometric mapping (section 16 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_mapping handle is the reference's PhotometricMapping.  The four pipelines it owns, its three map triples, the stage steps
// of a frame and the small entries are the frame-loop core it shares with vg_mono_odom (vg_frame_loop.hpp).  Here: the inter
// frame's image and pose, the frame store, the alignment sums and PhotometricMapping's state machine -- a new inter frame's SGM
// map is noise-filtered, a base below min_stereo_base only warps the map (and fails in INIT), xi_local is reset at push time, the
// photometric key frame keeps the inter image while only the map changes.  A frame works on copies of the poses, writes its maps
// into the scratch triples, keeps a push into the frame store pending, and commits when its last stage has succeeded.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "vg_frame_loop.hpp"
#include "vg_mapping.hpp"

using vgmap::Array6d;

struct vg_mapping : vgmo::FrameLoop {
    vg_mapping_params prm;
    bool photo_has_inter = false;   // the photometric key frame's image is the inter image: set_depth is enough
    int state = vgmap::kBegin, warning = vgmap::kWarnNone, map_idx = -1;
    bool have_inter = false;
    Array6d zeta_odom{}, xi_inter{};
    vgi::Grow<uint8_t> d_inter;    // the inter frame's image
    // the frame store: poses on the host, images in device chunks of kChunk images that are never moved
    static constexpr int64_t kChunk = 16;
    std::vector<Array6d> poses;
    std::vector<std::unique_ptr<vgi::Grow<uint8_t>>> chunks;
    uint8_t *frame(int64_t k) const { return chunks[(size_t)(k / kChunk)]->get() + (size_t)(k % kChunk) * (size_t)img; }
    vgi::Grow<unsigned long long> d_sums;
    vgi::GrowPinned<unsigned long long> h_sums;
};

namespace {

using vgi::fail;
using vgmo::kMaxPyramid;
using vgmo::load6;
using vgmo::store6;
using vgsh::blocks_of;

int check_thresholds(const vg_mapping_params &p)
{
    const double v[8] = {p.new_kf_distance_thresh, p.new_kf_angular_thresh, p.min_init_dist, p.min_stereo_base, p.rotation_tolerance,
                         p.min_scale_length,       p.min_scale_ratio,       p.max_scale_ratio};
    if (!vgsh::finite_n(v, 8) || !std::isfinite(p.dist_thresh)) return fail(VG_ERR_INVALID_ARGUMENT, "the thresholds must be finite");
    for (int i = 0; i < 6; i++)
        if (v[i] < 0) return fail(VG_ERR_INVALID_ARGUMENT, "the distance, angle and length thresholds must not be negative");
    if (!(p.min_scale_ratio > 0) || !(p.max_scale_ratio >= p.min_scale_ratio))
        return fail(VG_ERR_INVALID_ARGUMENT, "the scale ratios must be positive, min_scale_ratio not above max_scale_ratio");
    return VG_OK;
}

// room for frame number `count` (the next one): a new chunk when the last is full
int reserve_frame(vg_mapping *s)
{
    if (s->poses.size() < s->chunks.size() * (size_t)vg_mapping::kChunk) return VG_OK;
    std::unique_ptr<vgi::Grow<uint8_t>> c(new (std::nothrow) vgi::Grow<uint8_t>());
    if (!c) return fail(VG_ERR_ALLOC, "out of host memory");
    if (const int rc = c->grow((size_t)(vg_mapping::kChunk * s->img), "a chunk of the frame store")) return rc;
    s->chunks.push_back(std::move(c));
    return VG_OK;
}

// the unconditional insert; img is a DEVICE image (the caller's or the inter image)
int store_frame(vg_mapping *s, const Array6d &xi, const uint8_t *img)
{
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (const int rc = reserve_frame(s)) return rc;
    VG_HIP(hipMemcpyAsync(s->frame((int64_t)s->poses.size()), img, (size_t)s->img, hipMemcpyDeviceToDevice, s->stream));
    if (const int rc = call.finish()) return rc;
    s->poses.push_back(xi);
    return VG_OK;
}

// what a frame leaves behind, committed by feed_image once every stage has succeeded
struct Frame {
    Array6d xi_local, xi_local_old, xi_inter, zeta_odom;
    int state, map_idx, warning;
    bool pushed = false;       // pushInterFrame ran: img becomes the inter image
    bool to_store = false;     // the old inter frame goes into the frame store (as frame number poses.size())
    Array6d stored_xi{};
    int new_slot = 0;          // the triple that becomes the map
    bool mi_ran = false;
    double scale[4] = {0, 0, 0, 0}, photo[3] = {0, 0, 0}, mi[4] = {0, 0, 0, 0}, sgm = 0, refined = 0, motion[6] = {0, 0, 0, 0, 0, 0},
           merge[5] = {0, 0, 0, 0, 0};
};

// selectMapFrame over the store and the frame's pending push
int select_frame(const vg_mapping *s, const Frame &f, const Array6d &xi, double K)
{
    if (!f.to_store) return vgmap::select_frame(s->prm, (int64_t)s->poses.size(), s->poses.data(), xi, K);
    std::vector<Array6d> all(s->poses);
    all.push_back(f.stored_xi);
    return vgmap::select_frame(s->prm, (int64_t)all.size(), all.data(), xi, K);
}

// pushInterFrame (:190-255) with the pose f.xi_local of the new image; the maps are written into the scratch triples
int push_inter_frame(vg_mapping *s, const uint8_t *img, Frame &f)
{
    if (f.state == vgmap::kSlam) {
        f.to_store = true;
        f.stored_xi = f.xi_inter;
    }
    const Array6d base = vgmo::camera_motion(s->xi_base_cam, f.xi_local);
    if (vgmo::norm3(base.data()) > s->prm.min_stereo_base) {
        if (const int rc = vgmo::sgm_map(s, base, img, s->d_inter, true)) return rc;   // computeStereo(img, interFrame.img), filtered
        f.sgm = 1.;
        f.new_slot = 1;
        if (f.state != vgmap::kInit) {   // the prior map projected forward, the new one merged into it
            if (const int rc = vgmo::warp_map(s, base)) return rc;
            if (const int rc = vgmo::merge_maps(s, f.merge)) return rc;
            f.new_slot = 2;
        }
    } else if (f.state != vgmap::kInit) {   // too short a base for stereo: the map is only carried forward
        if (const int rc = vgmo::warp_map(s, base)) return rc;
        f.new_slot = 2;
    } else {   // the reference's bare throw
        return fail(VG_ERR_STATE, "INIT: the sparse increment moves the camera less than min_stereo_base, no first depth map: call vg_mapping_reinit");
    }
    f.xi_inter = vgth::compose(f.xi_inter, f.xi_local);
    f.zeta_odom = f.xi_local;
    f.xi_local = f.xi_local_old = Array6d{};
    f.pushed = true;
    return VG_OK;
}

// improveStereo (:181-188): the map refined into a scratch triple
int improve_stereo(vg_mapping *s, const uint8_t *img, Frame &f)
{
    const Array6d base = vgmo::camera_motion(s->xi_base_cam, f.xi_local);
    if (vgmo::norm3(base.data()) < s->prm.min_stereo_base || !vgsh::has_baseline(base.data())) return VG_OK;
    if (const int rc = vgmo::refine_map(s, base, img, f.motion)) return rc;
    f.refined = 1.;
    f.new_slot = 1;
    return VG_OK;
}

// localizePhoto (:353-460): img against the inter frame with the map
int localize_photo(vg_mapping *s, const uint8_t *img, Frame &f)
{
    if (!s->have_map || !s->have_inter) return fail(VG_ERR_STATE, "no inter frame with a depth map");
    const double *map = s->triple(0);
    if (s->photo_has_inter) {
        if (const int rc = vg_photo_set_depth(s->photo, map)) {
            s->photo_has_inter = false;
            return rc;
        }
    } else {
        if (const int rc = vg_photometric_set_base(s->photo, s->d_inter, map)) return rc;
        s->photo_has_inter = true;
    }
    Array6d vo;
    if (const int rc = vgmo::solve_photo(s, img, f.xi_local, vo, f.photo)) return rc;
    const vgmap::Scale sc = vgmap::normalize_scale(s->prm, f.xi_local_old, f.xi_local, vo);
    f.xi_local = sc.xi;
    if (s->prm.normalize_scale) {
        f.xi_local_old = f.xi_local;
        f.warning = sc.warning;
    }
    f.scale[0] = sc.K;
    f.scale[1] = sc.length;
    f.scale[2] = sc.length_prior;
    f.scale[3] = sc.rot_diff;
    return VG_OK;
}

// localizeMI (:334-351): the new inter frame (img with the frame's map) against map frame f.map_idx
int localize_mi(vg_mapping *s, const uint8_t *img, Frame &f)
{
    const bool pending = f.map_idx == (int)s->poses.size();   // the frame this call pushes: its image is still the inter image
    const Array6d xi_map = pending ? f.stored_xi : s->poses[(size_t)f.map_idx];
    const uint8_t *target_img = pending ? s->d_inter.get() : s->frame(f.map_idx);
    s->photo_has_inter = false;
    if (const int rc = vg_photometric_set_base(s->photo, img, s->triple(f.new_slot))) return rc;
    if (const int rc = vg_photometric_set_targets(s->photo, 1, target_img)) return rc;
    const Array6d start = vgth::inverse_compose(f.xi_inter, xi_map);
    const int32_t target = 0;
    Array6d out;
    double rep[4 * kMaxPyramid];
    if (const int rc = vg_mi_compute_pose(s->photo, 1, start.data(), &target, f.zeta_odom.data(), nullptr, out.data(), rep)) return rc;
    f.xi_inter = vgth::compose_inverse(xi_map, out);
    for (int i = 0; i < s->prm.num_scales; i++) f.mi[0] += rep[4 * (size_t)i];
    for (int i = 0; i < s->prm.num_scales; i++) {
        int64_t m = 0;
        if (const int rc = vg_photometric_pack(s->photo, i, &m, nullptr, nullptr, nullptr)) return rc;
        if (m == 0) continue;
        for (int k = 1; k < 4; k++) f.mi[k] = rep[4 * (size_t)i + k];
        break;
    }
    f.mi_ran = true;
    return VG_OK;
}

// the device steps first (the only ones that can fail), then the frame's poses and indices become the handle's
int commit(vg_mapping *s, const uint8_t *img, const Frame &f, bool new_inter)
{
    if (f.to_store)
        if (const int rc = store_frame(s, f.stored_xi, s->d_inter)) return rc;
    if (new_inter) {
        if (const int rc = vgmo::copy_image(s, s->d_inter, img)) return rc;
        s->have_inter = true;
        s->photo_has_inter = f.mi_ran;   // localizeMI left img as the photometric key frame
        if (f.pushed)
            if (const int rc = vg_motion_stereo_set_base(s->motion, 1, s->d_inter)) return rc;
    }
    s->map_slot = (s->map_slot + f.new_slot) % 3;
    if (f.new_slot) s->have_map = true;
    s->xi_local = f.xi_local;
    s->xi_local_old = f.xi_local_old;
    s->xi_inter = f.xi_inter;
    s->zeta_odom = f.zeta_odom;
    s->state = f.state;
    s->map_idx = f.map_idx;
    s->warning = f.warning;
    return VG_OK;
}

int check_pose(const double *xi, const char *what)
{
    if (!vgsh::finite_n(xi, 6)) return fail(VG_ERR_INVALID_ARGUMENT, std::string(what) + " must be finite");
    return VG_OK;
}

}  // namespace

extern "C" {

void vg_mapping_params_default(vg_mapping_params *p)
{
    if (!p) return;
    p->new_kf_distance_thresh = 0.03;
    p->new_kf_angular_thresh = 0.25;
    p->min_init_dist = 0.1;
    p->min_stereo_base = 0.07;
    p->dist_thresh = 5.;
    p->normalize_scale = 1;
    p->rotation_tolerance = 0.005;
    p->min_scale_length = 1e-2;
    p->min_scale_ratio = 0.8;
    p->max_scale_ratio = 1.2;
    p->num_scales = 5;
    vg_motion_stereo_params_default(&p->motion);
    vg_sparse_odom_params_default(&p->sparse);
}

int vg_mapping_create(vg_mapping **out, int device, void *hip_stream, const double *eucm, const double *xi_base_cam, int width, int height,
                      const vg_mapping_params *params)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (!eucm || !xi_base_cam || !params) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = check_thresholds(*params)) return rc;
    std::unique_ptr<vg_mapping> s(new (std::nothrow) vg_mapping());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    s->prm = *params;
    if (const int rc = vgmo::open_loop(s.get(), device, hip_stream, eucm, xi_base_cam, width, height, params->motion, params->sparse,
                                       params->num_scales, "photometric mapping"))
        return rc;
    if (const int rc = s->d_inter.grow((size_t)s->img, "the inter image")) return rc;
    if (const int rc = s->d_sums.grow(3, "the alignment sums")) return rc;
    if (const int rc = s->h_sums.grow(3, "the alignment sums' staging")) return rc;
    *out = s.release();
    return VG_OK;
}

void vg_mapping_destroy(vg_mapping *s) { vgi::destroy(s); }

int vg_mapping_size(const vg_mapping *s, int *width, int *height, int *x_max, int *y_max) { return vgmo::size(s, width, height, x_max, y_max); }

int vg_mapping_feed_odometry(vg_mapping *s, const double *xi_odom_new) { return vgmo::feed_odometry(s, xi_odom_new); }

int vg_mapping_reinit(vg_mapping *s, const double *xi)
{
    if (!s || !xi) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = check_pose(xi, "the pose")) return rc;
    if (s->state == vgmap::kSlam)
        if (const int rc = store_frame(s, s->xi_inter, s->d_inter)) return rc;
    s->state = vgmap::kBegin;
    s->xi_local = s->xi_local_old = load6(xi);
    s->have_odom = false;
    return VG_OK;
}

int vg_mapping_feed_image(vg_mapping *s, const uint8_t *img, const int32_t *samples, double *report)
{
    if (!s || !img) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    Frame f;
    f.xi_local = s->xi_local;
    f.xi_local_old = s->xi_local_old;
    f.xi_inter = s->xi_inter;
    f.zeta_odom = s->zeta_odom;
    f.state = s->state;
    f.map_idx = s->map_idx;
    f.warning = s->warning;
    int action = vgmap::kWaiting;
    bool new_inter = false;
    switch (s->state) {
    case vgmap::kBegin: {   // store what the initialisation needs
        f.xi_inter = f.xi_local;
        f.xi_local = Array6d{};
        if (const int rc = vg_sparse_odom_feed(s->sparse, img, f.xi_local.data(), samples, nullptr, nullptr)) return rc;
        f.state = vgmap::kInit;
        action = vgmap::kFirst;
        new_inter = true;
        break;
    }
    case vgmap::kInit: {   // wait until the distance is sufficient
        if (vgmo::norm3(f.xi_local.data()) < s->prm.min_init_dist) break;
        Array6d incr;
        if (const int rc = vg_sparse_odom_feed(s->sparse, img, f.xi_local.data(), samples, incr.data(), nullptr)) return rc;
        f.xi_local = incr;
        if (const int rc = push_inter_frame(s, img, f)) return rc;
        f.map_idx = select_frame(s, f, f.xi_inter, vgmap::kSelectK);
        if (f.map_idx == -1) {
            f.state = vgmap::kSlam;   // the frame will be put into the map
            action = vgmap::kInitSlam;
        } else {
            f.state = vgmap::kLocalize;
            action = vgmap::kInitLocalize;
            if (const int rc = localize_mi(s, img, f)) return rc;
        }
        new_inter = true;
        break;
    }
    case vgmap::kLocalize: {
        if (s->map_idx < 0 || s->map_idx >= (int)s->poses.size()) return fail(VG_ERR_STATE, "LOCALIZE without a map frame");
        if (const int rc = localize_photo(s, img, f)) return rc;
        const bool inter_ok = vgmap::check_distance(s->prm, f.xi_local, 1.);
        const Array6d xi_map_fr = vgth::inverse_compose(s->poses[(size_t)f.map_idx], f.xi_inter);
        const bool map_ok = vgmap::check_distance(s->prm, vgth::compose(xi_map_fr, f.xi_local), 1.);
        if (!map_ok) {   // the map frame has to change
            if (const int rc = push_inter_frame(s, img, f)) return rc;
            const int old_idx = f.map_idx;
            f.map_idx = select_frame(s, f, f.xi_inter, vgmap::kSelectK);
            if (f.map_idx != -1 && f.map_idx != old_idx) {
                action = vgmap::kLocalizeMapFrameChanged;
                if (const int rc = localize_mi(s, img, f)) return rc;
            } else if (f.map_idx == -1) {
                f.state = vgmap::kSlam;
                action = vgmap::kLocalizeLeftMap;
            } else {
                action = vgmap::kLocalizeMapFrameKept;
            }
            new_inter = true;
        } else if (!inter_ok) {
            if (const int rc = push_inter_frame(s, img, f)) return rc;
            action = vgmap::kLocalizeInterFrame;
            if (const int rc = localize_mi(s, img, f)) return rc;
            new_inter = true;
        } else {
            action = vgmap::kLocalizeRefined;
            if (const int rc = improve_stereo(s, img, f)) return rc;
        }
        break;
    }
    default: {   // SLAM: localize with respect to the inter frame
        if (const int rc = localize_photo(s, img, f)) return rc;
        if (!vgmap::check_distance(s->prm, f.xi_local, 1.)) {
            if (const int rc = push_inter_frame(s, img, f)) return rc;
            f.map_idx = select_frame(s, f, f.xi_inter, vgmap::kSelectK);
            action = vgmap::kSlamInterFrame;
            if (f.map_idx != -1) {
                f.state = vgmap::kLocalize;
                action = vgmap::kSlamEnteredMap;
                if (const int rc = localize_mi(s, img, f)) return rc;
            }
            new_inter = true;
        } else {
            action = vgmap::kSlamRefined;
            if (const int rc = improve_stereo(s, img, f)) return rc;
        }
        break;
    }
    }
    const int state_before = s->state, idx_before = s->map_idx;
    if (const int rc = commit(s, img, f, new_inter)) return rc;
    if (report) {
        double r[VG_MAPPING_REPORT] = {(double)state_before, (double)s->state, (double)action, (double)s->warning, (double)idx_before, (double)s->map_idx};
        for (int i = 0; i < 4; i++) r[6 + i] = f.scale[i];
        for (int i = 0; i < 3; i++) r[10 + i] = f.photo[i];
        for (int i = 0; i < 4; i++) r[13 + i] = f.mi[i];
        r[17] = f.sgm;
        r[18] = f.refined;
        for (int i = 0; i < 6; i++) r[19 + i] = f.motion[i];
        for (int i = 0; i < 5; i++) r[25 + i] = f.merge[i];
        r[30] = (double)s->poses.size();
        std::memcpy(report, r, sizeof(r));
    }
    return VG_OK;
}

int vg_mapping_num_frames(const vg_mapping *s, int64_t *count)
{
    if (!s || !count) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *count = (int64_t)s->poses.size();
    return VG_OK;
}

int vg_mapping_get_frame(vg_mapping *s, int64_t k, double *xi6, uint8_t *img)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "mapping handle is NULL");
    if (k < 0 || k >= (int64_t)s->poses.size()) return fail(VG_ERR_INVALID_ARGUMENT, "the frame index is out of range");
    if (xi6) store6(s->poses[(size_t)k], xi6);
    return img ? vgmo::copy_image(s, img, s->frame(k)) : VG_OK;
}

int vg_mapping_add_frame(vg_mapping *s, const double *xi, const uint8_t *img)
{
    if (!s || !xi || !img) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = check_pose(xi, "the pose")) return rc;
    return store_frame(s, load6(xi), img);
}

int vg_mapping_construct_map(vg_mapping *s, const double *xi, const uint8_t *img, int *inserted)
{
    if (!s || !xi || !img || !inserted) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = check_pose(xi, "the pose")) return rc;
    *inserted = 0;
    if (vgmap::select_frame(s->prm, (int64_t)s->poses.size(), s->poses.data(), load6(xi), 1.) != -1) return VG_OK;
    if (const int rc = store_frame(s, load6(xi), img)) return rc;
    *inserted = 1;
    return VG_OK;
}

int vg_mapping_select_frame(const vg_mapping *s, const double *xi, double K, int *idx)
{
    if (!s || !xi || !idx) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = check_pose(xi, "the pose")) return rc;
    if (!std::isfinite(K)) return fail(VG_ERR_INVALID_ARGUMENT, "K must be finite");
    *idx = vgmap::select_frame(s->prm, (int64_t)s->poses.size(), s->poses.data(), load6(xi), K);
    return VG_OK;
}

int vg_mapping_alignment(vg_mapping *s, const uint8_t *base, const uint8_t *img, const double *xi, const double *depth, uint8_t *err, int64_t *sums)
{
    if (!s || !img || !sums) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (xi)
        if (const int rc = check_pose(xi, "the pose")) return rc;
    if (!depth && !s->have_map) return fail(VG_ERR_STATE, "no depth map yet: pass one, or feed images first");
    if (!base && !s->have_inter) return fail(VG_ERR_STATE, "no inter image yet: pass a base image, or feed images first");
    if (err) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(img), b = reinterpret_cast<uintptr_t>(err);
        if (a < b + (size_t)s->img && b < a + (size_t)s->img) return fail(VG_ERR_INVALID_ARGUMENT, "the warp is a gather: err must not overlap img");
    }
    vgmap::AlignArgs args;
    args.w.v = s->view;
    vgmo::warp_image_pose(s->xi_base_cam, xi ? load6(xi) : s->xi_local, args.w);
    args.w.depth = depth ? depth : s->triple(0);
    args.w.src = img;
    args.w.dst = nullptr;
    args.base = base ? base : s->d_inter.get();
    args.err = err;
    args.sums = s->d_sums;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    VG_HIP(hipMemsetAsync(s->d_sums, 0, 3 * sizeof(unsigned long long), s->stream));
    hipLaunchKernelGGL(vgmap::mapping_alignment_kernel, dim3(blocks_of(s->img, vgmap::kLanes)), dim3(vgmap::kLanes), 0, s->stream, args);
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(s->h_sums, s->d_sums, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    if (const int rc = call.finish()) return rc;
    for (int i = 0; i < 3; i++) sums[i] = (int64_t)s->h_sums.get()[i];
    return VG_OK;
}

int vg_mapping_state(const vg_mapping *s, int *state)
{
    if (!s || !state) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *state = s->state;
    return VG_OK;
}

int vg_mapping_map_index(const vg_mapping *s, int *idx)
{
    if (!s || !idx) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *idx = s->map_idx;
    return VG_OK;
}

int vg_mapping_warning(const vg_mapping *s, int *warning)
{
    if (!s || !warning) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *warning = s->warning;
    return VG_OK;
}

int vg_mapping_xi_local(const vg_mapping *s, double *xi6) { return vgmo::get_pose(s, &vg_mapping::xi_inter, xi6, 0); }
int vg_mapping_xi_inter(const vg_mapping *s, double *xi6) { return vgmo::get_pose(s, &vg_mapping::xi_inter, xi6, 1); }
int vg_mapping_xi_composed(const vg_mapping *s, double *xi6) { return vgmo::get_pose(s, &vg_mapping::xi_inter, xi6, 2); }

int vg_mapping_get_map(vg_mapping *s, double *depth, double *sigma, double *cost) { return vgmo::get_map(s, depth, sigma, cost, "mapping handle is NULL"); }

int vg_mapping_map(const vg_mapping *s, const double **depth, const double **sigma, const double **cost) { return vgmo::map(s, depth, sigma, cost); }

int vg_mapping_check_distance(const vg_mapping_params *params, const double *xi, double K, int *ok)
{
    if (!params || !xi || !ok) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = check_thresholds(*params)) return rc;
    if (const int rc = check_pose(xi, "the pose")) return rc;
    if (!std::isfinite(K)) return fail(VG_ERR_INVALID_ARGUMENT, "K must be finite");
    *ok = vgmap::check_distance(*params, load6(xi), K) ? 1 : 0;
    return VG_OK;
}

int vg_mapping_select_frame_host(const vg_mapping_params *params, int64_t n, const double *poses, const double *xi, double K, int *idx)
{
    if (!params || !xi || !idx || (n > 0 && !poses)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n < 0) return fail(VG_ERR_INVALID_ARGUMENT, "the frame count must not be negative");
    if (const int rc = check_thresholds(*params)) return rc;
    if (const int rc = check_pose(xi, "the pose")) return rc;
    if (!std::isfinite(K)) return fail(VG_ERR_INVALID_ARGUMENT, "K must be finite");
    std::vector<Array6d> all((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (const int rc = check_pose(poses + 6 * i, "the map's poses")) return rc;
        all[(size_t)i] = load6(poses + 6 * i);
    }
    *idx = vgmap::select_frame(*params, n, all.data(), load6(xi), K);
    return VG_OK;
}

int vg_mapping_normalize_scale(const vg_mapping_params *params, const double *xi_local_old, const double *xi_local_prior,
                               const double *xi_local_vo, double *out6, double *K, double *length, double *length_prior, double *rot_diff,
                               int *warning)
{
    if (!params || !xi_local_old || !xi_local_prior || !xi_local_vo || !out6 || !warning) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = check_thresholds(*params)) return rc;
    if (!vgsh::finite_n(xi_local_old, 6) || !vgsh::finite_n(xi_local_prior, 6) || !vgsh::finite_n(xi_local_vo, 6))
        return fail(VG_ERR_INVALID_ARGUMENT, "the poses must be finite");
    const vgmap::Scale sc = vgmap::normalize_scale(*params, load6(xi_local_old), load6(xi_local_prior), load6(xi_local_vo));
    store6(sc.xi, out6);
    if (K) *K = sc.K;
    if (length) *length = sc.length;
    if (length_prior) *length_prior = sc.length_prior;
    if (rot_diff) *rot_diff = sc.rot_diff;
    *warning = sc.warning;
    return VG_OK;
}

int vg_mapping_relocalized_pose(const double *xi_map, const double *xi_fr_map, double *out6)
{
    if (!xi_map || !xi_fr_map || !out6) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!vgsh::finite_n(xi_map, 6) || !vgsh::finite_n(xi_fr_map, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "the poses must be finite");
    store6(vgth::compose_inverse(load6(xi_map), load6(xi_fr_map)), out6);
    return VG_OK;
}

}  // extern "C"
