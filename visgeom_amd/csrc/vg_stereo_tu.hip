// vg_stereo_tu.hip -- translation unit of libvisgeom_amd.so: dense fisheye stereo (section 9 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_stereo handle owns the curve tables and the per-pixel geometry of one calibrated pair (built at creation) and the
// device scratch of one chunk of pairs (grown on demand, at most max(kStereoBudget, one pair)).  A compute call runs four
// launches per chunk: curve cost, left + right, top + bottom with the winner, depth.  vg_stereo_compute_mh runs the same
// four with the multi-hypothesis variants of the last two: the winner planes take the place of the single winner.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "vg_geometry.hpp"
#include "vg_handle.hpp"
#include "vg_stereo.hpp"
#include "vg_stereo_host.hpp"

namespace {

using vgi::fail;

constexpr int64_t kStereoBudget = int64_t(2) << 30;   // device scratch of one chunk, bytes (one pair more if it is larger)

using namespace vgsh;

}  // namespace

struct vg_stereo : vgi::HandleBase {
    vg_stereo_params prm;
    vgs::StereoGeom g;
    vgi::Grow<vgs::Poly2> d_table;
    vgi::Grow<vgs::GeomEntry> d_geom;
    vgi::Grow<uint8_t> d_scratch;   // bytes
    int64_t P = 0;

    // hyp: winner planes per pixel (1: vg_stereo_compute)
    int64_t per_pair(int hyp = 1) const { return P * (5 * (int64_t)prm.disp_max + 3 + 4 * (int64_t)hyp); }
    int64_t chunk(int hyp = 1) const { return std::max<int64_t>(1, kStereoBudget / per_pair(hyp)); }
};

namespace {

// device pointers of one chunk's scratch (or of the caller's buffers, for the stage entries)
struct Bufs {
    uint8_t *err = nullptr, *step = nullptr, *sal = nullptr, *skip = nullptr;
    int32_t *sum = nullptr, *disp = nullptr;
};

// carve n pairs' err / step / salient / skip / sum / disparity (hyp planes) out of the handle's scratch
int scratch_bufs(vg_stereo *s, int64_t n, Bufs &b, int hyp = 1)
{
    const int64_t P = s->P, D = s->prm.disp_max;
    if (const int rc = s->d_scratch.grow((size_t)(n * s->per_pair(hyp)), "the stereo scratch")) return rc;
    uint8_t *p = s->d_scratch.get();
    b.sum = reinterpret_cast<int32_t *>(p);
    p += n * P * D * 4;
    b.disp = reinterpret_cast<int32_t *>(p);
    p += n * P * hyp * 4;
    b.err = p;
    p += n * P * D;
    b.step = p;
    p += n * P;
    b.sal = p;
    p += n * P;
    b.skip = p;
    return VG_OK;
}

void launch_cost(vg_stereo *s, int64_t n, const uint8_t *img1, const uint8_t *img2, const Bufs &b)
{
    vgs::CurveCostArgs a;
    a.img1 = img1;
    a.img2 = img2;
    a.geom = s->d_geom;
    a.err = b.err;
    a.step = b.step;
    a.salient = b.sal;
    a.skip = b.skip;
    a.n_pairs = n;
    hipLaunchKernelGGL(vgs::stereo_curve_cost_kernel, dim3(blocks_of(n * s->P, vgs::kMatchLanes)), dim3(vgs::kMatchLanes), 0, s->stream,
                       s->g, a);
}

// mh == nullptr: the single winner to b.disp; otherwise the hypothesis planes to mh's arrays
void launch_agg(vg_stereo *s, int64_t n, const Bufs &b, bool write_total, const vgs::MhArgs *mh = nullptr)
{
    vgs::AggArgs a;
    a.err = b.err;
    a.step = b.step;
    a.salient = b.sal;
    a.skip = b.skip;
    a.sum = b.sum;
    a.disparity = b.disp;
    a.n_pairs = n;
    a.write_total = write_total ? 1 : 0;
    hipLaunchKernelGGL(vgs::stereo_agg_rows_kernel, dim3((unsigned)(n * s->g.y_max)), dim3(vgs::kAggLanes), 0, s->stream, s->g, a);
    const dim3 cols((unsigned)(n * s->g.x_max)), lanes(vgs::kAggLanes);
    if (mh) hipLaunchKernelGGL((vgs::stereo_agg_cols_kernel<true>), cols, lanes, 0, s->stream, s->g, a, *mh);
    else hipLaunchKernelGGL((vgs::stereo_agg_cols_kernel<false>), cols, lanes, 0, s->stream, s->g, a, vgs::MhArgs{1, 0, nullptr, nullptr});
}

void launch_depth(vg_stereo *s, int64_t n, const Bufs &b, double *depth, double *sigma, double *cost)
{
    vgs::DepthArgs a;
    a.geom = s->d_geom;
    a.err = b.err;
    a.step = b.step;
    a.salient = b.sal;
    a.skip = b.skip;
    a.disparity = b.disp;
    a.depth = depth;
    a.sigma = sigma;
    a.cost = cost;
    a.n_pairs = n;
    hipLaunchKernelGGL(vgs::stereo_depth_kernel, dim3(blocks_of(n * s->P, 256)), dim3(256), 0, s->stream, s->g, a);
}

// the hypothesis planes: disp and the outputs are [n][hyp][P]
void launch_depth_mh(vg_stereo *s, int64_t n, const Bufs &b, int hyp, const int32_t *disp, double *depth, double *sigma, double *cost)
{
    vgs::DepthArgs a;
    a.geom = s->d_geom;
    a.err = b.err;
    a.step = b.step;
    a.salient = b.sal;
    a.skip = b.skip;
    a.disparity = disp;
    a.depth = depth;
    a.sigma = sigma;
    a.cost = cost;
    a.n_pairs = n;
    hipLaunchKernelGGL(vgs::stereo_depth_mh_kernel, dim3(blocks_of(n * hyp * s->P, 256)), dim3(256), 0, s->stream, s->g, a, hyp);
}

int check_call(vg_stereo *s, int64_t n, const void *img1, const void *img2)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "stereo handle is NULL");
    if (n < 0) return fail(VG_ERR_INVALID_ARGUMENT, "negative pair count");
    if (n > 0 && (!img1 || !img2)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL image");
    return VG_OK;
}

}  // namespace

extern "C" {

void vg_stereo_params_default(vg_stereo_params *p)
{
    if (!p) return;
    *p = vg_stereo_params();
    p->scale = 1;
    p->u0 = p->v0 = 0;
    p->u_max = p->v_max = 1;
    p->x_max = p->y_max = 1;
    p->equal_margins = 0;
    p->num_epipolar_planes = 2000;
    p->epipole_margin = 2500;
    p->disp_max = 48;
    p->error_max = 25;
    p->verbosity = 0;
    p->hypotheses = 1;
    p->hypo_difference = 10;
    p->flaw_cost = 7;
    p->desc_length = 5;
    p->desc_resp_thresh = 5;
    p->n_scales = 4;
    const int sc[4] = {1, 2, 3, 5};
    for (int i = 0; i < 8; i++) p->scales[i] = i < 4 ? sc[i] : 0;
    p->step_cost = 5;
    p->jump_cost = 32;
    p->image_based_cost = 1;
    p->salient_points_only = 1;
    p->use_uv_cache = 1;
}

int vg_stereo_create(vg_stereo **out, int device, void *hip_stream, const double *eucm1, const double *eucm2, const double *xi12,
                     const vg_stereo_params *params)
{
    if (!out) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    *out = nullptr;
    if (!eucm1 || !eucm2 || !xi12 || !params) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    int x_max = 0, y_max = 0;
    if (const int rc = check_params(*params, x_max, y_max)) return rc;
    if (!finite_n(eucm1, 6) || !finite_n(eucm2, 6) || !finite_n(xi12, 6))
        return fail(VG_ERR_INVALID_ARGUMENT, "camera parameters and transformation must be finite");
    if (!focal_nonzero(eucm1, eucm2)) return fail(VG_ERR_INVALID_ARGUMENT, "fu, fv must be non-zero");
    if (!has_baseline(xi12)) return fail(VG_ERR_INVALID_ARGUMENT, "the stereo baseline must not vanish (|t|^2 > 1e-10)");
    std::unique_ptr<vg_stereo> s(new (std::nothrow) vg_stereo());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    s->prm = *params;
    s->prm.x_max = x_max;
    s->prm.y_max = y_max;
    s->g.x_max = x_max;
    s->g.y_max = y_max;
    s->P = (int64_t)x_max * y_max;
    std::vector<vgs::Poly2> table(2 * (size_t)(params->num_epipolar_planes + 1));
    if (const int rc = build_geometry(s->g, s->prm, eucm1, eucm2, xi12, table.data())) return rc;
    if (const int rc = s->open(device, hip_stream, "stereo")) return rc;
    vgi::Call call(s.get());   // a failure below drains the stream before s is freed
    if (call.begin() != VG_OK) return fail(VG_ERR_HIP, "hipSetDevice failed");
    if (const int rc = s->d_table.grow(table.size(), "the stereo geometry")) return rc;
    if (const int rc = s->d_geom.grow((size_t)s->P, "the stereo geometry")) return rc;
    if (hipMemcpyAsync(s->d_table, table.data(), table.size() * sizeof(vgs::Poly2), hipMemcpyHostToDevice, s->stream) != hipSuccess)
        return fail(VG_ERR_HIP, "curve table upload failed");
    s->g.table = s->d_table;
    hipLaunchKernelGGL(vgs::stereo_geometry_kernel, dim3(blocks_of(s->P, 256)), dim3(256), 0, s->stream, s->g, s->d_geom);
    if (hipGetLastError() != hipSuccess || call.finish() != VG_OK) return fail(VG_ERR_HIP, "stereo geometry kernel failed");
    *out = s.release();
    return VG_OK;
}

void vg_stereo_destroy(vg_stereo *s) { vgi::destroy(s); }

int vg_stereo_size(const vg_stereo *s, int *x_max, int *y_max)
{
    if (!s || !x_max || !y_max) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *x_max = s->prm.x_max;
    *y_max = s->prm.y_max;
    return VG_OK;
}

int vg_stereo_chunk(const vg_stereo *s, int64_t *pairs)
{
    if (!s || !pairs) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    *pairs = s->chunk();
    return VG_OK;
}

int vg_stereo_geometry(vg_stereo *s, int32_t *geometry)
{
    if (!s || !geometry) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    VG_HIP(hipMemcpyAsync(geometry, s->d_geom, (size_t)s->P * sizeof(vgs::GeomEntry), hipMemcpyDeviceToDevice, s->stream));
    return call.finish();
}

int vg_stereo_curve_cost(vg_stereo *s, int64_t n_pairs, const uint8_t *img1, const uint8_t *img2, uint8_t *err, uint8_t *step,
                         uint8_t *salient, uint8_t *skip)
{
    if (const int rc = check_call(s, n_pairs, img1, img2)) return rc;
    if (n_pairs > 0 && (!err || !step || !salient || !skip)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    if (n_pairs == 0) return VG_OK;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    Bufs b;
    b.err = err;
    b.step = step;
    b.sal = salient;
    b.skip = skip;
    launch_cost(s, n_pairs, img1, img2, b);
    VG_HIP(hipGetLastError());
    return call.finish();
}

int vg_stereo_aggregate(vg_stereo *s, int64_t n_pairs, const uint8_t *img1, const uint8_t *img2, int32_t *total, int32_t *disparity)
{
    if (const int rc = check_call(s, n_pairs, img1, img2)) return rc;
    if (n_pairs > 0 && !total) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    if (n_pairs == 0) return VG_OK;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    // scratch for what the caller does not supply: the error volume, step / salient / skip, and the winner if disparity is NULL
    const int64_t np = n_pairs * s->P;
    const int64_t bytes = np * (s->prm.disp_max + 3), pad = (4 - bytes % 4) % 4;   // pad: aligns the winner behind the byte buffers
    if (const int rc = s->d_scratch.grow((size_t)(bytes + (disparity ? 0 : pad + np * 4)), "the stereo scratch")) return rc;
    Bufs b;
    b.err = s->d_scratch.get();
    b.step = b.err + np * s->prm.disp_max;
    b.sal = b.step + np;
    b.skip = b.sal + np;
    b.sum = total;
    b.disp = disparity ? disparity : reinterpret_cast<int32_t *>(b.skip + np + pad);
    launch_cost(s, n_pairs, img1, img2, b);
    launch_agg(s, n_pairs, b, true);
    VG_HIP(hipGetLastError());
    return call.finish();
}

int vg_stereo_compute(vg_stereo *s, int64_t n_pairs, const uint8_t *img1, const uint8_t *img2, double *depth, double *sigma,
                      double *cost, int32_t *disparity)
{
    if (const int rc = check_call(s, n_pairs, img1, img2)) return rc;
    if (n_pairs == 0) return VG_OK;
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    const int64_t chunk = std::min<int64_t>(s->chunk(), n_pairs);
    const int64_t P = s->P, img = (int64_t)s->prm.u_max * s->prm.v_max;
    Bufs b;
    if (const int rc = scratch_bufs(s, chunk, b)) return rc;
    for (int64_t first = 0; first < n_pairs; first += chunk) {
        const int64_t n = std::min(chunk, n_pairs - first);
        Bufs c = b;
        if (disparity) c.disp = disparity + first * P;
        launch_cost(s, n, img1 + first * img, img2 + first * img, c);
        launch_agg(s, n, c, false);
        launch_depth(s, n, c, depth ? depth + first * P : nullptr, sigma ? sigma + first * P : nullptr, cost ? cost + first * P : nullptr);
        VG_HIP(hipGetLastError());
    }
    return call.finish();
}

int vg_stereo_compute_mh(vg_stereo *s, int64_t n_pairs, const uint8_t *img1, const uint8_t *img2, int hyp_max, double *depth, double *sigma,
                         double *cost, int32_t *disparity, int32_t *final_cost)
{
    if (!s) return fail(VG_ERR_INVALID_ARGUMENT, "stereo handle is NULL");
    if (n_pairs < 1) return fail(VG_ERR_INVALID_ARGUMENT, "the pair count must be at least 1");
    if (!img1 || !img2) return fail(VG_ERR_INVALID_ARGUMENT, "NULL image");
    if (hyp_max < 2 || hyp_max > vgs::kMaxHyp || hyp_max > s->prm.disp_max)
        return fail(VG_ERR_INVALID_ARGUMENT, "hyp_max must be in [2, 8] and at most disparity_max (1: vg_stereo_compute)");
    vgi::Call call(s);
    if (const int rc = call.begin()) return rc;
    const int64_t chunk = std::min<int64_t>(s->chunk(hyp_max), n_pairs);
    const int64_t HP = hyp_max * s->P, img = (int64_t)s->prm.u_max * s->prm.v_max;
    Bufs b;
    if (const int rc = scratch_bufs(s, chunk, b, hyp_max)) return rc;
    for (int64_t first = 0; first < n_pairs; first += chunk) {
        const int64_t n = std::min(chunk, n_pairs - first);
        vgs::MhArgs mh;
        mh.hyp_max = hyp_max;
        mh.hypo_difference = s->prm.hypo_difference;
        mh.disparity = disparity ? disparity + first * HP : b.disp;
        mh.final_cost = final_cost ? final_cost + first * HP : nullptr;
        launch_cost(s, n, img1 + first * img, img2 + first * img, b);
        launch_agg(s, n, b, false, &mh);
        if (depth || sigma || cost)
            launch_depth_mh(s, n, b, hyp_max, mh.disparity, depth ? depth + first * HP : nullptr, sigma ? sigma + first * HP : nullptr,
                            cost ? cost + first * HP : nullptr);
        VG_HIP(hipGetLastError());
    }
    return call.finish();
}

int vg_stereo_curve_walk(const double *poly6, int u, int v, int eu, int ev, int step_mult, int steps, int32_t *uv)
{
    if (!poly6 || !uv) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (steps < -1000 || steps > 1000) return fail(VG_ERR_INVALID_ARGUMENT, "|steps| must be at most 1000");
    if (step_mult < -16 || step_mult > 16 || step_mult == 0) return fail(VG_ERR_INVALID_ARGUMENT, "step_mult must be in [-16, 16], non-zero");
    if (std::abs(u) > (1 << 24) || std::abs(v) > (1 << 24) || std::abs(eu) > (1 << 24) || std::abs(ev) > (1 << 24))
        return fail(VG_ERR_INVALID_ARGUMENT, "coordinates must be within +-2^24");
    const vgs::Poly2 pl = {poly6[0], poly6[1], poly6[2], poly6[3], poly6[4], poly6[5]};
    vgs::Raster r;
    r.init(u, v, eu, ev, pl);
    r.eps *= step_mult;
    uv[0] = r.u;
    uv[1] = r.v;
    const int n = steps < 0 ? -steps : steps;
    for (int i = 1; i <= n; i++) {
        if (steps > 0) r.step();
        else r.unstep();
        uv[2 * i] = r.u;
        uv[2 * i + 1] = r.v;
    }
    return VG_OK;
}

}  // extern "C"
