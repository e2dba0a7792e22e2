// vg_stereo_tu.hip -- translation unit of libvisgeom_amd.so: dense fisheye stereo (section 9 of the C ABI).
// Built with hipcc for gfx950 only; compiled on its own so that an edit of one subsystem does not rebuild the others.
//
// A vg_stereo handle owns the curve tables and the per-pixel geometry of one calibrated pair (built at creation) and the
// device scratch of one chunk of pairs (grown on demand, at most max(kStereoBudget, one pair)).  A compute call runs four
// launches per chunk: curve cost, left + right, top + bottom with the winner, depth.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "vg_geometry.hpp"
#include "vg_internal.hpp"
#include "vg_stereo.hpp"

namespace {

using vgi::fail;

constexpr int64_t kStereoBudget = int64_t(2) << 30;   // device scratch of one chunk, bytes (one pair more if it is larger)

void limit_vector(double *x)   // limitVector (epipoles.cpp:27-35)
{
    const double M = 1e6;
    for (int i = 0; i < 2; i++) {
        if (x[i] > M) x[i] = M;
        if (x[i] < -M) x[i] = -M;
    }
}

// EnhancedEpipolar::computePolynomial (eucm_epipolar.cpp:129-169) for the camera `p` with epipole `ep`
vgs::Poly2 compute_polynomial(const double *p, const double *ep, const double *plane)
{
    const double alpha = p[0], beta = p[1], fu = p[2], fv = p[3], u0 = p[4], v0 = p[5];
    const double gamma = 1 - alpha, ag = alpha - gamma, a2b = alpha * alpha * beta;
    const double fufv = fu * fv, fufu = fu * fu, fvfv = fv * fv;
    const double A = plane[0], B = plane[1], C = plane[2];
    const double AA = A * A, BB = B * B, CC = C * C;
    const double CCfufv = CC * fufv;
    const double dd = CCfufv / (AA + BB);
    vgs::Poly2 s;
    if ((AA + BB) > 0 && dd < 1.) {
        s.kuu = s.kuv = s.kvv = 0;
        s.ku = A / fu;
        s.kv = B / fv;
        const double normABinv = 1. / std::sqrt(AA + BB);
        const double Cnorm = C / std::sqrt(AA + BB + CC);
        const double du = -A * Cnorm * normABinv * fu;
        const double dv = -B * Cnorm * normABinv * fv;
        s.k1 = -(u0 + du) * A / fu - (v0 + dv) * B / fv;
    } else {
        s.kuu = (AA * ag + CC * a2b) / (CC * fufu);
        s.kuv = 2 * A * B * ag / (CCfufv);
        s.kvv = (BB * ag + CC * a2b) / (CC * fvfv);
        s.ku = 2 * (-(AA * fv * u0 + A * B * fu * v0) * ag - A * C * fufv * gamma - CC * a2b * fv * u0) / (CCfufv * fu);
        s.kv = 2 * (-(BB * fu * v0 + A * B * fv * u0) * ag - B * C * fufv * gamma - CC * a2b * fu * v0) / (CCfufv * fv);
        s.k1 = -(s.kuu * ep[0] * ep[0] + s.kuv * ep[0] * ep[1] + s.kvv * ep[1] * ep[1] + s.ku * ep[0] + s.kv * ep[1]);
    }
    return s;
}

void cross3(const double *a, const double *b, double *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

}  // namespace

struct vg_stereo {
    int device = 0;
    hipStream_t stream = nullptr;
    vg_stereo_params prm;
    vgs::StereoGeom g;
    vgi::DeviceMem<vgs::Poly2> d_table;
    vgi::DeviceMem<vgs::GeomEntry> d_geom;
    vgi::DeviceMem<void> d_scratch;
    int64_t scratch_bytes = 0;
    int64_t P = 0;

    int64_t per_pair() const { return P * (5 * (int64_t)prm.disp_max + 7); }
    int64_t chunk() const { return std::max<int64_t>(1, kStereoBudget / per_pair()); }
};

namespace {

int check_params(const vg_stereo_params &p, int &x_max, int &y_max)
{
    if (p.hypotheses != 1) return fail(VG_ERR_INVALID_ARGUMENT, "hypotheses must be 1 (reconstructDisparityMH is not provided)");
    if (p.disp_max < 4 || p.disp_max > 256 || p.disp_max % 2) return fail(VG_ERR_INVALID_ARGUMENT, "disparity_max must be even in [4, 256]");
    if (p.desc_length < 3 || p.desc_length > vgs::kMaxDesc || p.desc_length % 2 == 0)
        return fail(VG_ERR_INVALID_ARGUMENT, "descriptor_size must be odd in [3, 31]");
    if (p.n_scales < 1 || p.n_scales > vgs::kMaxScales) return fail(VG_ERR_INVALID_ARGUMENT, "1 to 8 descriptor scales");
    for (int i = 0; i < p.n_scales; i++)
        if (p.scales[i] < 1 || p.scales[i] > 16) return fail(VG_ERR_INVALID_ARGUMENT, "every descriptor scale must be in [1, 16]");
    if (p.scale < 1 || p.scale > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "scale must be in [1, 16384]");
    if (p.u_max < 1 || p.u_max > 16384 || p.v_max < 1 || p.v_max > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "uMax / vMax must be in [1, 16384]");
    if (std::abs(p.u0) > 16384 || std::abs(p.v0) > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "|u0|, |v0| must be at most 16384");
    x_max = p.x_max;
    y_max = p.y_max;
    if (p.equal_margins) {   // ScaleParameters::setEqualMargin (scale_parameters.cpp:44-52)
        x_max = (p.u_max - 2 * p.u0) / p.scale + 1;
        y_max = (p.v_max - 2 * p.v0) / p.scale + 1;
    }
    if (x_max < 1 || y_max < 1) return fail(VG_ERR_INVALID_ARGUMENT, "the scaled image is empty: xMax < 1 or yMax < 1");
    if (x_max > 16384 || y_max > 16384) return fail(VG_ERR_INVALID_ARGUMENT, "xMax / yMax must be at most 16384");
    if (p.num_epipolar_planes < 2 || p.num_epipolar_planes > (1 << 20) || p.num_epipolar_planes % 2)
        return fail(VG_ERR_INVALID_ARGUMENT, "num_epipolar_planes must be even in [2, 2^20]");
    if (p.epipole_margin < 0) return fail(VG_ERR_INVALID_ARGUMENT, "epipole_margin must be >= 0");
    if (p.flaw_cost < 0 || p.flaw_cost > 10000 || p.step_cost < 0 || p.step_cost > 10000 || p.jump_cost < 0 || p.jump_cost > 10000)
        return fail(VG_ERR_INVALID_ARGUMENT, "flaw_cost, step_cost and jump_cost must be in [0, 10000]");
    if (std::abs(p.desc_resp_thresh) > 1000000) return fail(VG_ERR_INVALID_ARGUMENT, "descriptor_response_thresh out of range");
    return VG_OK;
}

bool finite_n(const double *v, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// the host half of the handle: transform, epipoles (StereoEpipoles ctor, epipoles.cpp:37-57), curve bases and tables
// (EnhancedEpipolar::initialize, eucm_epipolar.cpp:33-107)
int build_geometry(vg_stereo &s, const double *c1, const double *c2, const double *xi, std::vector<vgs::Poly2> &table)
{
    vgs::StereoGeom &g = s.g;
    const vg_stereo_params &p = s.prm;
    for (int i = 0; i < 6; i++) {
        g.c1[i] = c1[i];
        g.c2[i] = c2[i];
    }
    const vg::RotTrig rt = vg::rot_trig(xi + 3, true, false);
    vg::rotation_matrix(xi + 3, 1., rt, g.R);
    vg::rotation_matrix(xi + 3, -1., rt, g.Rinv);
    for (int i = 0; i < 3; i++) g.t[i] = xi[i];

    double ep[2][2][2];
    const double mt[3] = {-g.t[0], -g.t[1], -g.t[2]};
    double ti[3], mti[3];
    vgs::mat_vec(g.Rinv, g.t, ti);
    for (int i = 0; i < 3; i++) {
        ti[i] = -ti[i];   // transInv = -rotMatInv t
        mti[i] = -ti[i];
    }
    g.epi_ok[0][0] = vgs::eucm_project(c1, g.t, ep[0][0]);
    g.epi_ok[0][1] = vgs::eucm_project(c1, mt, ep[0][1]);
    g.epi_ok[1][0] = vgs::eucm_project(c2, ti, ep[1][0]);
    g.epi_ok[1][1] = vgs::eucm_project(c2, mti, ep[1][1]);
    for (int c = 0; c < 2; c++) {
        if (!g.epi_ok[c][0] && !g.epi_ok[c][1])
            return fail(VG_ERR_INVALID_ARGUMENT, std::string("neither the epipole nor the anti-epipole projects into camera ") +
                                                     (c == 0 ? "1" : "2"));
        for (int k = 0; k < 2; k++) {
            if (!g.epi_ok[c][k]) {
                ep[c][k][0] = ep[c][k][1] = 0.;
                g.epi_px[c][k][0] = g.epi_px[c][k][1] = 0;
                continue;
            }
            limit_vector(ep[c][k]);
            g.epi_px[c][k][0] = (int)std::round(ep[c][k][0]);
            g.epi_px[c][k][1] = (int)std::round(ep[c][k][1]);
        }
    }

    // the epipolar basis
    const int n = p.num_epipolar_planes;
    g.n_planes = n;
    g.plane_step = 4. / n;
    const double tn = std::sqrt(g.t[0] * g.t[0] + g.t[1] * g.t[1] + g.t[2] * g.t[2]);
    double z[3];
    for (int i = 0; i < 3; i++) z[i] = -(g.t[i] / tn);
    const int axis = (z[2] * z[2] > z[0] * z[0] + z[1] * z[1]) ? 0 : 2;
    double xb[3];
    for (int i = 0; i < 3; i++) xb[i] = (i == axis ? 1. : 0.) - z[i] * z[axis];
    const double xn = std::sqrt(xb[0] * xb[0] + xb[1] * xb[1] + xb[2] * xb[2]);
    for (int i = 0; i < 3; i++) g.xBase[i] = xb[i] / xn;
    cross3(z, g.xBase, g.yBase);

    table.resize(2 * (size_t)(n + 1));
    double z2[3];
    vgs::mat_vec(g.Rinv, z, z2);   // t21n
    for (int c = 0; c < 2; c++) {
        const double *cam = c == 0 ? c1 : c2;
        const int k = g.epi_ok[c][0] ? 0 : 1;   // StereoEpipoles::get(idx)
        for (int idx = 0; idx < n; idx++) {
            double dir[3];
            if (idx < n / 2) {
                const double sv = g.plane_step * idx - 1;
                for (int i = 0; i < 3; i++) dir[i] = g.xBase[i] + sv * g.yBase[i];
            } else {
                const double cv = g.plane_step * (-idx + n / 2) + 1;
                for (int i = 0; i < 3; i++) dir[i] = cv * g.xBase[i] + g.yBase[i];
            }
            double plane[3];
            if (c == 0) {
                cross3(dir, z, plane);
            } else {
                double dir2[3];
                vgs::mat_vec(g.Rinv, dir, dir2);
                cross3(dir2, z2, plane);
            }
            table[(size_t)c * (n + 1) + idx] = compute_polynomial(cam, ep[c][k], plane);
        }
        table[(size_t)c * (n + 1) + n] = table[(size_t)c * (n + 1)];
    }

    g.scale = p.scale;
    g.u0 = p.u0;
    g.v0 = p.v0;
    g.u_max = p.u_max;
    g.v_max = p.v_max;
    g.epipole_margin = p.epipole_margin;
    g.disp_max = p.disp_max;
    g.error_max = p.error_max;
    g.flaw_cost = p.flaw_cost;
    g.desc_length = p.desc_length;
    g.n_scales = p.n_scales;
    for (int i = 0; i < vgs::kMaxScales; i++) g.scales[i] = i < p.n_scales ? p.scales[i] : 1;
    g.desc_resp_thresh = p.desc_resp_thresh;
    g.step_cost = p.step_cost;
    g.jump_cost = p.jump_cost;
    g.image_based_cost = p.image_based_cost != 0;
    g.salient_points_only = p.salient_points_only != 0;
    g.use_uv_cache = p.use_uv_cache != 0;
    return VG_OK;
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// device pointers of one chunk's scratch (or of the caller's buffers, for the stage entries)
struct Bufs {
    uint8_t *err = nullptr, *step = nullptr, *sal = nullptr, *skip = nullptr;
    int32_t *sum = nullptr, *disp = nullptr;
};

int ensure_scratch(vg_stereo *s, int64_t bytes)
{
    if (bytes <= s->scratch_bytes) return VG_OK;
    s->scratch_bytes = 0;
    VG_HIP(s->d_scratch.release());
    VG_HIP(s->d_scratch.alloc((size_t)bytes));
    s->scratch_bytes = bytes;
    return VG_OK;
}

// carve n pairs' err / step / salient / skip / sum / disparity out of the handle's scratch
int scratch_bufs(vg_stereo *s, int64_t n, Bufs &b)
{
    const int64_t P = s->P, D = s->prm.disp_max;
    if (const int rc = ensure_scratch(s, n * s->per_pair())) return rc;
    char *p = static_cast<char *>(s->d_scratch.get());
    b.sum = reinterpret_cast<int32_t *>(p);
    p += n * P * D * 4;
    b.disp = reinterpret_cast<int32_t *>(p);
    p += n * P * 4;
    b.err = reinterpret_cast<uint8_t *>(p);
    p += n * P * D;
    b.step = reinterpret_cast<uint8_t *>(p);
    p += n * P;
    b.sal = reinterpret_cast<uint8_t *>(p);
    p += n * P;
    b.skip = reinterpret_cast<uint8_t *>(p);
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
    hipLaunchKernelGGL(vgs::stereo_curve_cost_kernel, dim3(blocks_of(n * s->P, vgs::kCostLanes)), dim3(vgs::kCostLanes), 0, s->stream,
                       s->g, a);
}

void launch_agg(vg_stereo *s, int64_t n, const Bufs &b, bool write_total)
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
    hipLaunchKernelGGL(vgs::stereo_agg_cols_kernel, dim3((unsigned)(n * s->g.x_max)), dim3(vgs::kAggLanes), 0, s->stream, s->g, a);
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
    if (eucm1[2] == 0. || eucm1[3] == 0. || eucm2[2] == 0. || eucm2[3] == 0.) return fail(VG_ERR_INVALID_ARGUMENT, "fu, fv must be non-zero");
    if (!(xi12[0] * xi12[0] + xi12[1] * xi12[1] + xi12[2] * xi12[2] > 1e-10))
        return fail(VG_ERR_INVALID_ARGUMENT, "the stereo baseline must not vanish (|t|^2 > 1e-10)");
    std::unique_ptr<vg_stereo> s(new (std::nothrow) vg_stereo());
    if (!s) return fail(VG_ERR_ALLOC, "out of host memory");
    s->prm = *params;
    s->prm.x_max = x_max;
    s->prm.y_max = y_max;
    s->g.x_max = x_max;
    s->g.y_max = y_max;
    s->P = (int64_t)x_max * y_max;
    std::vector<vgs::Poly2> table;
    if (const int rc = build_geometry(*s, eucm1, eucm2, xi12, table)) return rc;
    if (const int rc = vgi::check_device(device, "stereo")) return rc;
    s->device = device;
    s->stream = reinterpret_cast<hipStream_t>(hip_stream);
    if (hipSetDevice(device) != hipSuccess) return fail(VG_ERR_HIP, "hipSetDevice failed");
    vgi::StreamDrain drain{s->stream};   // a failure below drains the stream before s is freed
    if (s->d_table.alloc(table.size() * sizeof(vgs::Poly2)) != hipSuccess || s->d_geom.alloc((size_t)s->P * sizeof(vgs::GeomEntry)) != hipSuccess)
        return fail(VG_ERR_ALLOC, "device allocation of the stereo geometry failed");
    if (hipMemcpyAsync(s->d_table, table.data(), table.size() * sizeof(vgs::Poly2), hipMemcpyHostToDevice, s->stream) != hipSuccess)
        return fail(VG_ERR_HIP, "curve table upload failed");
    s->g.table = s->d_table;
    hipLaunchKernelGGL(vgs::stereo_geometry_kernel, dim3(blocks_of(s->P, 256)), dim3(256), 0, s->stream, s->g, s->d_geom);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) return fail(VG_ERR_HIP, "stereo geometry kernel failed");
    drain.armed = false;
    *out = s.release();
    return VG_OK;
}

void vg_stereo_destroy(vg_stereo *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    delete s;
}

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
    VG_HIP(hipSetDevice(s->device));
    VG_HIP(hipMemcpyAsync(geometry, s->d_geom, (size_t)s->P * sizeof(vgs::GeomEntry), hipMemcpyDeviceToDevice, s->stream));
    VG_HIP(hipStreamSynchronize(s->stream));
    return VG_OK;
}

int vg_stereo_curve_cost(vg_stereo *s, int64_t n_pairs, const uint8_t *img1, const uint8_t *img2, uint8_t *err, uint8_t *step,
                         uint8_t *salient, uint8_t *skip)
{
    if (const int rc = check_call(s, n_pairs, img1, img2)) return rc;
    if (n_pairs > 0 && (!err || !step || !salient || !skip)) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    if (n_pairs == 0) return VG_OK;
    VG_HIP(hipSetDevice(s->device));
    Bufs b;
    b.err = err;
    b.step = step;
    b.sal = salient;
    b.skip = skip;
    launch_cost(s, n_pairs, img1, img2, b);
    VG_HIP(hipGetLastError());
    VG_HIP(hipStreamSynchronize(s->stream));
    return VG_OK;
}

int vg_stereo_aggregate(vg_stereo *s, int64_t n_pairs, const uint8_t *img1, const uint8_t *img2, int32_t *total, int32_t *disparity)
{
    if (const int rc = check_call(s, n_pairs, img1, img2)) return rc;
    if (n_pairs > 0 && !total) return fail(VG_ERR_INVALID_ARGUMENT, "NULL output");
    if (n_pairs == 0) return VG_OK;
    VG_HIP(hipSetDevice(s->device));
    // scratch for what the caller does not supply: the error volume, step / salient / skip, and the winner if disparity is NULL
    const int64_t np = n_pairs * s->P;
    if (const int rc = ensure_scratch(s, np * (s->prm.disp_max + 3) + (disparity ? 0 : np * 4))) return rc;
    Bufs b;
    b.err = static_cast<uint8_t *>(s->d_scratch.get());
    b.step = b.err + np * s->prm.disp_max;
    b.sal = b.step + np;
    b.skip = b.sal + np;
    b.sum = total;
    b.disp = disparity ? disparity : reinterpret_cast<int32_t *>(b.skip + np + (4 - (np * (s->prm.disp_max + 3)) % 4) % 4);
    launch_cost(s, n_pairs, img1, img2, b);
    launch_agg(s, n_pairs, b, true);
    VG_HIP(hipGetLastError());
    VG_HIP(hipStreamSynchronize(s->stream));
    return VG_OK;
}

int vg_stereo_compute(vg_stereo *s, int64_t n_pairs, const uint8_t *img1, const uint8_t *img2, double *depth, double *sigma,
                      double *cost, int32_t *disparity)
{
    if (const int rc = check_call(s, n_pairs, img1, img2)) return rc;
    if (n_pairs == 0) return VG_OK;
    VG_HIP(hipSetDevice(s->device));
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
    VG_HIP(hipStreamSynchronize(s->stream));
    return VG_OK;
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
