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

#include "vg_internal.hpp"
#include "vg_motion.hpp"
#include "vg_stereo_host.hpp"

struct vg_motion_stereo {
    int device = 0;
    hipStream_t stream = nullptr;
    vg_motion_stereo_params prm;
    double c1[6], c2[6];
    int64_t P = 0, img = 0, table_len = 0;   // depth pixels, image pixels, Poly2 entries of one item's two tables
    int64_t n_base = 0, cap_base = 0;        // key frames held / allocated
    vgi::DeviceMem<uint8_t> d_img1, d_mask;
    int64_t cap_items = 0;                   // items the per-call buffers hold
    vgi::DeviceMem<vgs::StereoGeom> d_geom;
    vgi::DeviceMem<vgs::Poly2> d_table;
    vgi::DeviceMem<unsigned long long> d_counts;
    vgi::PinnedMem<vgs::StereoGeom> h_geom;
    vgi::PinnedMem<vgs::Poly2> h_table;
    vgi::PinnedMem<unsigned long long> h_counts;
};

namespace {

using vgi::fail;
constexpr int64_t kMaxItems = 65535;   // items ride on gridDim.y / gridDim.z

using vgsh::blocks_of;

int ensure_items(vg_motion_stereo *s, int64_t n)
{
    if (n <= s->cap_items) return VG_OK;
    s->cap_items = 0;
    const size_t geom = (size_t)n * sizeof(vgs::StereoGeom), table = (size_t)(n * s->table_len) * sizeof(vgs::Poly2);
    const size_t counts = (size_t)n * 6 * sizeof(unsigned long long);
    if (s->d_geom.alloc(geom) != hipSuccess || s->d_table.alloc(table) != hipSuccess || s->d_counts.alloc(counts) != hipSuccess)
        return fail(VG_ERR_ALLOC, "device allocation of the motion stereo geometry failed");
    if (s->h_geom.alloc(geom, hipHostMallocDefault) != hipSuccess || s->h_table.alloc(table, hipHostMallocDefault) != hipSuccess ||
        s->h_counts.alloc(counts, hipHostMallocDefault) != hipSuccess)
        return fail(VG_ERR_ALLOC, "pinned allocation of the motion stereo staging failed");
    s->cap_items = n;
    return VG_OK;
}

// one call of compute / select: setTransformation of every item on the host, upload, one launch, counts back
int run(vg_motion_stereo *s, int64_t n, const double *xi12, const uint8_t *img2, const double *depth_in, const double *sigma_in,
        const double *cost_in, double *depth, double *sigma, double *cost, vgm::Rec *rec, int64_t *counts)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "motion stereo handle is NULL");
    if (n < 0 || n > kMaxItems) return fail(VG_ERR_INVALID_ARGUMENT, "the item count must be in [0, 65535]");
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
    VG_HIP(hipSetDevice(s->device));
    if (const int rc = ensure_items(s, n)) return rc;
    for (int64_t k = 0; k < n; k++) {
        vgs::StereoGeom &g = s->h_geom.get()[k];
        std::memset(&g, 0, sizeof(g));
        g.x_max = s->prm.stereo.x_max;
        g.y_max = s->prm.stereo.y_max;
        if (const int rc = vgsh::build_geometry(g, s->prm.stereo, s->c1, s->c2, xi12 + 6 * k, s->h_table.get() + k * s->table_len)) return rc;
        g.table = s->d_table.get() + k * s->table_len;
    }
    vgi::StreamDrain drain{s->stream};
    VG_HIP(hipMemcpyAsync(s->d_geom, s->h_geom, (size_t)n * sizeof(vgs::StereoGeom), hipMemcpyHostToDevice, s->stream));
    VG_HIP(hipMemcpyAsync(s->d_table, s->h_table, (size_t)(n * s->table_len) * sizeof(vgs::Poly2), hipMemcpyHostToDevice, s->stream));
    if (counts) VG_HIP(hipMemsetAsync(s->d_counts, 0, (size_t)n * 6 * sizeof(unsigned long long), s->stream));
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
    a.counts = counts ? s->d_counts.get() : nullptr;
    a.P = s->P;
    a.gradient_thresh = s->prm.gradient_thresh;
    hipLaunchKernelGGL(vgm::motion_stereo_kernel, dim3(blocks_of(s->P, vgs::kMatchLanes), (unsigned)n), dim3(vgs::kMatchLanes), 0, s->stream, a);
    VG_HIP(hipGetLastError());
    if (counts)
        VG_HIP(hipMemcpyAsync(s->h_counts, s->d_counts, (size_t)n * 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    drain.armed = false;
    VG_HIP(hipStreamSynchronize(s->stream));
    if (counts)
        for (int64_t i = 0; i < n * 6; i++) counts[i] = (int64_t)s->h_counts.get()[i];
    return VG_OK;
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
    if (const int rc = vgi::check_device(device, "motion stereo")) return rc;
    s->device = device;
    s->stream = reinterpret_cast<hipStream_t>(hip_stream);
    *out = s.release();
    return VG_OK;
}

void vg_motion_stereo_destroy(vg_motion_stereo *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    delete s;
}

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
    if (n < 1 || n > kMaxItems) return fail(VG_ERR_INVALID_ARGUMENT, "the number of key frames must be in [1, 65535]");
    VG_HIP(hipSetDevice(s->device));
    s->n_base = 0;
    if (n > s->cap_base) {
        s->cap_base = 0;
        if (s->d_img1.alloc((size_t)(n * s->img)) != hipSuccess || s->d_mask.alloc((size_t)(n * s->img)) != hipSuccess)
            return fail(VG_ERR_ALLOC, "device allocation of the key frames failed");
        s->cap_base = n;
    }
    vgi::StreamDrain drain{s->stream};
    VG_HIP(hipMemcpyAsync(s->d_img1, img1, (size_t)(n * s->img), hipMemcpyDeviceToDevice, s->stream));
    const int w = s->prm.stereo.u_max, h = s->prm.stereo.v_max;
    hipLaunchKernelGGL(vgm::motion_mask_kernel, dim3(blocks_of(w, vgm::kMaskW), blocks_of(h, vgm::kMaskH), (unsigned)n),
                       dim3(vgm::kMaskW, vgm::kMaskH), 0, s->stream, s->d_img1.get(), s->d_mask.get(), w, h, s->prm.gradient_thresh);
    VG_HIP(hipGetLastError());
    drain.armed = false;
    VG_HIP(hipStreamSynchronize(s->stream));
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
    VG_HIP(hipSetDevice(s->device));
    VG_HIP(hipMemcpyAsync(mask, s->d_mask, (size_t)(s->n_base * s->img), hipMemcpyDeviceToDevice, s->stream));
    VG_HIP(hipStreamSynchronize(s->stream));
    return VG_OK;
}

int vg_motion_stereo_select(vg_motion_stereo *s, int64_t n, const double *xi12, const uint8_t *img2, const double *depth_in,
                            const double *sigma_in, const double *cost_in, int32_t *record)
{
    if (n > 0 && !record) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    return run(s, n, xi12, img2, depth_in, sigma_in, cost_in, nullptr, nullptr, nullptr, reinterpret_cast<vgm::Rec *>(record), nullptr);
}

}  // extern "C"
