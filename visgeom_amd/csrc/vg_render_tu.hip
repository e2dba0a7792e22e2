// vg_render_tu.hip -- translation unit of libvisgeom_amd.so: the synthetic scene renderer (section 14 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_render handle owns the world on the device -- the objects, their textures end to end in one block, the 300 doubles of
// the anti-aliasing kernels -- and the scratch of a call: the views' poses, the counters, and the index / u / v buffers the
// image launch reads when the caller asked for none.  Buffers only grow.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "vg_handle.hpp"
#include "vg_pose_host.hpp"
#include "vg_render.hpp"
#include "vg_stereo_host.hpp"

struct vg_render : vgi::HandleBase {
    double cam[6];
    int width = 0, height = 0, n_objects = 0;
    int64_t P = 0;
    vgi::Grow<vgr::Object> d_objects;
    vgi::Grow<uint8_t> d_textures;
    vgi::Grow<double> d_table;
    vgi::Grow<vgr::View> d_views;
    vgi::GrowPinned<vgr::View> h_views;
    vgi::Counters counters;
    vgi::Grow<int16_t> d_index;   // [n][P] each, grown only when the caller passes NULL for it
    vgi::Grow<float> d_u, d_v;
};

namespace {

using vgi::fail;
using vgsh::blocks_of;

const double *filter_table()   // built once, on first use
{
    static const std::vector<double> table = [] {
        std::vector<double> t(vgr::kTableSize);
        vgr::build_filter_table(t.data());
        return t;
    }();
    return table.data();
}

int check_camera(const double *eucm)
{
    if (!eucm) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    return vgsh::check_camera(eucm);
}

}  // namespace

extern "C" {

int vg_render_create(vg_render **out, int device, void *hip_stream, const double *eucm, int width, int height, int n_objects,
                     const vg_render_object *objects)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (const int rc = check_camera(eucm)) return rc;
    if (!objects) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (width < VG_RENDER_MIN_SIDE || width > VG_RENDER_MAX_SIDE || height < VG_RENDER_MIN_SIDE || height > VG_RENDER_MAX_SIDE)
        return fail(VG_ERR_INVALID_ARGUMENT, "the image's width and height must be in [2, 16384]");
    if (n_objects < 1 || n_objects > VG_RENDER_MAX_PLANES + 1) return fail(VG_ERR_INVALID_ARGUMENT, "a background and at most 64 planes expected");
    std::vector<vgr::Object> objs((size_t)n_objects);
    int64_t bytes = 0;
    for (int k = 0; k < n_objects; k++) {
        const vg_render_object &src = objects[k];
        vgr::Object &o = objs[(size_t)k];
        if (k == 0 ? src.kind != VG_RENDER_BACKGROUND : src.kind != VG_RENDER_PLANE)
            return fail(VG_ERR_INVALID_ARGUMENT, "object 0 must be the background and every other object a plane");
        if (!src.texture) return fail(VG_ERR_INVALID_ARGUMENT, "an object has no texture");
        if (src.cols < VG_RENDER_MIN_SIDE || src.cols > VG_RENDER_MAX_SIDE || src.rows < VG_RENDER_MIN_SIDE || src.rows > VG_RENDER_MAX_SIDE)
            return fail(VG_ERR_INVALID_ARGUMENT, "a texture's cols and rows must be in [2, 16384]");
        o.kind = src.kind == VG_RENDER_BACKGROUND ? vgr::kBackground : vgr::kPlane;
        o.cols = src.cols;
        o.rows = src.rows;
        o.texture = bytes;
        bytes += (int64_t)src.cols * src.rows;
        o.u0 = double(src.cols) / 2;
        o.v0 = double(src.rows) / 2;
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        if (o.kind == vgr::kBackground) {   // background.cpp:20-30
            o.fu = src.cols / (2 * M_PI);
            o.fv = src.rows / (2 * M_PI);
            for (int i = 0; i < 3; i++) o.t[i] = 0.;
        } else {   // plane.cpp:20-35
            if (!vgsh::finite_n(src.pose, 6) || !std::isfinite(src.width) || !std::isfinite(src.height))
                return fail(VG_ERR_INVALID_ARGUMENT, "a plane's pose, width and height must be finite");
            if (!(src.width > 0.) || !(src.height > 0.)) return fail(VG_ERR_INVALID_ARGUMENT, "a plane's width and height must be positive");
            o.fu = src.cols / src.width;
            o.fv = src.rows / src.height;
            for (int i = 0; i < 3; i++) o.t[i] = src.pose[i];
            vgth::rotation(src.pose, R);
        }
        for (int i = 0; i < 3; i++) {   // the columns of the rotation
            o.ex[i] = R[3 * i];
            o.ey[i] = R[3 * i + 1];
            o.ez[i] = R[3 * i + 2];
        }
    }
    std::unique_ptr<vg_render> s(new (std::nothrow) vg_render());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    for (int i = 0; i < 6; i++) s->cam[i] = eucm[i];
    s->width = width;
    s->height = height;
    s->n_objects = n_objects;
    s->P = (int64_t)width * height;
    if (const int rc = s->open(device, hip_stream, "rendering")) return rc;
    vgi::Call call(s.get());
    if (const int rc = call.begin()) return rc;
    if (const int rc = s->d_objects.grow((size_t)n_objects, "the objects")) return rc;
    if (const int rc = s->d_textures.grow((size_t)bytes, "the textures")) return rc;
    if (const int rc = s->d_table.grow(vgr::kTableSize, "the filter kernels")) return rc;
    // pageable sources: every copy below has left its source when it returns only after the synchronise, and all of them
    // (the caller's textures, objs, the static table) outlive it
    VG_HIP(hipMemcpyAsync(s->d_objects, objs.data(), objs.size() * sizeof(vgr::Object), hipMemcpyHostToDevice, s->stream));
    for (int k = 0; k < n_objects; k++)
        VG_HIP(hipMemcpyAsync(s->d_textures.get() + objs[(size_t)k].texture, objects[k].texture, (size_t)objects[k].cols * objects[k].rows,
                              hipMemcpyHostToDevice, s->stream));
    VG_HIP(hipMemcpyAsync(s->d_table, filter_table(), vgr::kTableSize * sizeof(double), hipMemcpyHostToDevice, s->stream));
    if (const int rc = call.finish()) return rc;
    *out = s.release();
    return VG_OK;
}

void vg_render_destroy(vg_render *s) { vgi::destroy(s); }

int vg_render_size(const vg_render *s, int *width, int *height)
{
    if (!s || !width || !height) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *width = s->width;
    *height = s->height;
    return VG_OK;
}

int vg_render_set_camera(vg_render *s, const double *eucm)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "render handle is NULL");
    if (const int rc = check_camera(eucm)) return rc;
    for (int i = 0; i < 6; i++) s->cam[i] = eucm[i];
    return VG_OK;
}

int vg_render_views(vg_render *s, int64_t n, const double *xi_cam, uint8_t *image, float *depth, int16_t *index, float *u, float *v,
                    int64_t *counts)
{
    if (const int rc = vgi::check_items(n, 0, "view")) return rc;
    if (n > 0 && !xi_cam) return fail(VG_ERR_INVALID_ARGUMENT, "the camera poses are NULL");
    if (n > 0 && !image) return fail(VG_ERR_INVALID_ARGUMENT, "the image is NULL");
    if (n > 0 && !vgsh::finite_n(xi_cam, 6 * (int)n)) return fail(VG_ERR_INVALID_ARGUMENT, "the camera poses must be finite");
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "render handle is NULL");
    if (n == 0) return VG_OK;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    const size_t np = (size_t)(n * s->P);
    if (const int rc = s->d_views.grow((size_t)n, "the views")) return rc;
    if (const int rc = s->h_views.grow((size_t)n, "the views' staging")) return rc;
    if (!index)
        if (const int rc = s->d_index.grow(np, "the index buffer")) return rc;
    if (!u)
        if (const int rc = s->d_u.grow(np, "the texture coordinate buffer")) return rc;
    if (!v)
        if (const int rc = s->d_v.grow(np, "the texture coordinate buffer")) return rc;
    for (int64_t k = 0; k < n; k++) {
        vgr::View &view = s->h_views.get()[k];
        vgth::rotation(xi_cam + 6 * k, view.R);
        for (int i = 0; i < 3; i++) view.t[i] = xi_cam[6 * k + i];
    }
    VG_HIP(hipMemcpyAsync(s->d_views, s->h_views, (size_t)n * sizeof(vgr::View), hipMemcpyHostToDevice, s->stream));
    vgr::Args a;
    for (int i = 0; i < 6; i++) a.cam[i] = s->cam[i];
    a.width = s->width;
    a.height = s->height;
    a.n_objects = s->n_objects;
    a.P = s->P;
    a.objects = s->d_objects;
    a.textures = s->d_textures;
    a.table = s->d_table;
    a.views = s->d_views;
    a.index = index ? index : s->d_index.get();
    a.u = u ? u : s->d_u.get();
    a.v = v ? v : s->d_v.get();
    a.depth = depth;
    a.image = image;
    if (const int rc = s->counters.begin(call, n, vgr::kCounts, counts, &a.counts)) return rc;
    const dim3 block(vgr::kLanes);
    hipLaunchKernelGGL(vgr::render_buffers_kernel, dim3(blocks_of(s->P, vgr::kLanes), (unsigned)n), block, 0, s->stream, a);
    hipLaunchKernelGGL(vgr::render_image_kernel, dim3(blocks_of(s->P, vgr::kLanes / vgr::kRowLanes), (unsigned)n), block, 0, s->stream, a);
    VG_HIP(hipGetLastError());
    return s->counters.end(call, n, vgr::kCounts, counts);
}

int vg_render_filter_kernel(int length, double *out)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (length < 1 || length > vgr::kMaxKernel) return fail(VG_ERR_INVALID_ARGUMENT, "the kernel length must be in [1, 24]");
    std::memcpy(out, filter_table() + vgr::kernel_offset(length), sizeof(double) * (size_t)length);
    return VG_OK;
}

}  // extern "C"
