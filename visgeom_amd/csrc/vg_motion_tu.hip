// vg_motion_tu.hip -- translation unit of libvisgeom_amd.so: motion stereo (section 10 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_motion_stereo handle owns the key frames with their masks and, per item of a call, one StereoGeom and one pair of
// curve tables: the pose changes with every call, so setTransformation runs on the host for every item (vg_stereo_host.hpp,
// the code vg_stereo_create uses) and goes up through pinned staging.  Buffers only grow; a call launches one kernel.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <string>

#include "vg_handle.hpp"
#include "vg_motion.hpp"
#include "vg_stereo_host.hpp"

struct vg_motion_stereo : vgi::HandleBase {
    vg_motion_stereo_params prm;
    double c1[6], c2[6];
    int64_t P = 0, img = 0, table_len = 0;   // depth pixels, image pixels, Poly2 entries of one item's two tables
    int64_t n_base = 0;                      // key frames held
    vgi::Grow<uint8_t> d_img1, d_mask;
    vgi::Grow<vgs::StereoGeom> d_geom;       // the per-call buffers: one geometry and table_len table entries per item
    vgi::Grow<vgs::Poly2> d_table;
    vgi::GrowPinned<vgs::StereoGeom> h_geom;
    vgi::GrowPinned<vgs::Poly2> h_table;
    vgi::Counters counters;
};

namespace {

using vgi::fail;
using vgsh::blocks_of;

int ensure_items(vg_motion_stereo *s, int64_t n)
{
    const size_t table = (size_t)(n * s->table_len);
    if (const int rc = s->d_geom.grow((size_t)n, "the motion stereo geometry")) return rc;
    if (const int rc = s->d_table.grow(table, "the motion stereo geometry")) return rc;
    if (const int rc = s->h_geom.grow((size_t)n, "the motion stereo staging")) return rc;
    return s->h_table.grow(table, "the motion stereo staging");
}

// one call of compute / select: setTransformation of every item on the host, upload, one launch, counts back
int run(vg_motion_stereo *s, int64_t n, const double *xi12, const uint8_t *img2, const double *depth_in, const double *sigma_in,
        const double *cost_in, double *depth, double *sigma, double *cost, vgm::Rec *rec, int64_t *counts)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "motion stereo handle is NULL");
    if (const int rc = vgi::check_items(n, 0, "item")) return rc;
    if (n == 0) return VG_OK;
    if (n > s->n_base) return fail(VG_ERR_STATE, "more items than key frames: call vg_motion_stereo_set_base first");
    if (!xi12 || !img2) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if ((depth_in || sigma_in || cost_in) && !(depth_in && sigma_in && cost_in))
        return fail(VG_ERR_INVALID_ARGUMENT, "a prior needs depth_in, sigma_in and cost_in");
    for (int64_t k = 0; k < n; k++) {
        const double *xi = xi12 + 6 * k;
        if (!vgsh::finite_n(xi, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "the transformations must be finite");
        if (!vgsh::has_baseline(xi)) return fail(VG_ERR_INVALID_ARGUMENT, "the baseline of an item must not vanish (|t|^2 > 1e-10)");
    }
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    if (const int rc = ensure_items(s, n)) return rc;
    for (int64_t k = 0; k < n; k++) {
        vgs::StereoGeom &g = s->h_geom.get()[k];
        std::memset(&g, 0, sizeof(g));
        g.x_max = s->prm.stereo.x_max;
        g.y_max = s->prm.stereo.y_max;
        if (const int rc = vgsh::build_geometry(g, s->prm.stereo, s->c1, s->c2, xi12 + 6 * k, s->h_table.get() + k * s->table_len)) return rc;
        g.table = s->d_table.get() + k * s->table_len;
    }
    VG_HIP(hipMemcpyAsync(s->d_geom, s->h_geom, (size_t)n * sizeof(vgs::StereoGeom), hipMemcpyHostToDevice, s->stream));
    VG_HIP(hipMemcpyAsync(s->d_table, s->h_table, (size_t)(n * s->table_len) * sizeof(vgs::Poly2), hipMemcpyHostToDevice, s->stream));
    vgm::MotionArgs a;
    a.geom = s->d_geom;
    a.img1 = s->d_img1;
    a.mask = s->d_mask;
    a.img2 = img2;
    a.depth_in = depth_in;
    a.sigma_in = sigma_in;
    a.cost_in = cost_in;
    a.depth = depth;
    a.sigma = sigma;
    a.cost = cost;
    a.rec = rec;
    if (const int rc = s->counters.begin(call, n, 6, counts, &a.counts)) return rc;
    a.P = s->P;
    a.gradient_thresh = s->prm.gradient_thresh;
    hipLaunchKernelGGL(vgm::motion_stereo_kernel, dim3(blocks_of(s->P, vgs::kMatchLanes), (unsigned)n), dim3(vgs::kMatchLanes), 0, s->stream, a);
    VG_HIP(hipGetLastError());
    return s->counters.end(call, n, 6, counts);
}

}  // namespace

extern "C" {

void vg_motion_stereo_params_default(vg_motion_stereo_params *p)
{
    if (!p) return;
    vg_stereo_params_default(&p->stereo);
    p->gradient_thresh = 2;
}

int vg_motion_stereo_create(vg_motion_stereo **out, int device, void *hip_stream, const double *eucm1, const double *eucm2,
                            const vg_motion_stereo_params *params)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (!eucm1 || !eucm2 || !params) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    int x_max = 0, y_max = 0;
    if (const int rc = vgsh::check_params(params->stereo, x_max, y_max)) return rc;
    if (params->gradient_thresh < 0 || params->gradient_thresh > 255) return fail(VG_ERR_INVALID_ARGUMENT, "gradient_thresh must be in [0, 255]");
    if (!vgsh::finite_n(eucm1, 6) || !vgsh::finite_n(eucm2, 6)) return fail(VG_ERR_INVALID_ARGUMENT, "camera parameters must be finite");
    if (!vgsh::focal_nonzero(eucm1, eucm2)) return fail(VG_ERR_INVALID_ARGUMENT, "fu, fv must be non-zero");
    std::unique_ptr<vg_motion_stereo> s(new (std::nothrow) vg_motion_stereo());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    s->prm = *params;
    s->prm.stereo.x_max = x_max;
    s->prm.stereo.y_max = y_max;
    for (int i = 0; i < 6; i++) {
        s->c1[i] = eucm1[i];
        s->c2[i] = eucm2[i];
    }
    s->P = (int64_t)x_max * y_max;
    s->img = (int64_t)params->stereo.u_max * params->stereo.v_max;
    s->table_len = 2 * (int64_t)(params->stereo.num_epipolar_planes + 1);
    if (const int rc = s->open(device, hip_stream, "motion stereo")) return rc;
    *out = s.release();
    return VG_OK;
}

void vg_motion_stereo_destroy(vg_motion_stereo *s) { vgi::destroy(s); }

int vg_motion_stereo_size(const vg_motion_stereo *s, int *x_max, int *y_max)
{
    if (!s || !x_max || !y_max) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *x_max = s->prm.stereo.x_max;
    *y_max = s->prm.stereo.y_max;
    return VG_OK;
}

int vg_motion_stereo_set_base(vg_motion_stereo *s, int64_t n, const uint8_t *img1)
{
    if (!s || !img1) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n < 1 || n > vgi::kMaxItems) return fail(VG_ERR_INVALID_ARGUMENT, "the number of key frames must be in [1, 65535]");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    s->n_base = 0;
    if (const int rc = s->d_img1.grow((size_t)(n * s->img), "the key frames")) return rc;
    if (const int rc = s->d_mask.grow((size_t)(n * s->img), "the key frames")) return rc;
    VG_HIP(hipMemcpyAsync(s->d_img1, img1, (size_t)(n * s->img), hipMemcpyDeviceToDevice, s->stream));
    const int w = s->prm.stereo.u_max, h = s->prm.stereo.v_max;
    hipLaunchKernelGGL(vgm::motion_mask_kernel, dim3(blocks_of(w, vgm::kMaskW), blocks_of(h, vgm::kMaskH), (unsigned)n),
                       dim3(vgm::kMaskW, vgm::kMaskH), 0, s->stream, s->d_img1.get(), s->d_mask.get(), w, h, s->prm.gradient_thresh);
    VG_HIP(hipGetLastError());
    if (const int rc = call.finish()) return rc;
    s->n_base = n;
    return VG_OK;
}

int vg_motion_stereo_compute(vg_motion_stereo *s, int64_t n, const double *xi12, const uint8_t *img2, const double *depth_in,
                             const double *sigma_in, const double *cost_in, double *depth, double *sigma, double *cost,
                             int64_t *counts)
{
    if (n > 0 && (!depth || !sigma || !cost)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    return run(s, n, xi12, img2, depth_in, sigma_in, cost_in, depth, sigma, cost, nullptr, counts);
}

int vg_motion_stereo_mask(vg_motion_stereo *s, uint8_t *mask)
{
    if (!s || !mask) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (s->n_base < 1) return fail(VG_ERR_STATE, "no key frame: call vg_motion_stereo_set_base first");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    VG_HIP(hipMemcpyAsync(mask, s->d_mask, (size_t)(s->n_base * s->img), hipMemcpyDeviceToDevice, s->stream));
    return call.finish();
}

int vg_motion_stereo_select(vg_motion_stereo *s, int64_t n, const double *xi12, const uint8_t *img2, const double *depth_in,
                            const double *sigma_in, const double *cost_in, int32_t *record)
{
    if (n > 0 && !record) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    return run(s, n, xi12, img2, depth_in, sigma_in, cost_in, nullptr, nullptr, nullptr, reinterpret_cast<vgm::Rec *>(record), nullptr);
}

}  // extern "C"
