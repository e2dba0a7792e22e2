// vg_convert_tu.hip -- translation unit of libvisgeom_amd.so: conversion between camera models (vg_unproject, vg_convert_map,
// vg_convert_start, vg_convert_fit; include/visgeom_amd.h section 20).  Built with hipcc for gfx950 only; compiled on its own so
// that an edit of one subsystem does not rebuild the others.  vg_unproject and vg_convert_map are stateless and asynchronous on the
// caller's stream: no allocation, no synchronisation, no host round trip (a caller may capture them in a graph).  vg_convert_fit
// owns its device blocks for the duration of the call and is synchronous.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "vg_convert.hpp"
#include "vg_internal.hpp"
#include "vg_lmn.hpp"

namespace {

using vgi::fail;

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

bool valid_dim(int d) { return d >= 1 && d <= vg::kRectMaxDim; }

void copy_intrinsics(int model, const double *src, double *dst)
{
    const int K = vg::num_intrinsics(model);
    for (int k = 0; k < vg::kConvertMaxK; k++) dst[k] = k < K ? src[k] : 0.;
}

template <int DST, int SRC>
void launch_map(const vg::ConvertMapArgs &a, bool vec, hipStream_t st)
{
    const dim3 grid((unsigned)((a.width + vg::kTileW - 1) / vg::kTileW), (unsigned)((a.height + vg::kTileH - 1) / vg::kTileH));
    const dim3 blk(vg::kRectLanesX, vg::kRectLanesY);
    if (vec) hipLaunchKernelGGL((vg::vg_convert_map_kernel<DST, SRC, true>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((vg::vg_convert_map_kernel<DST, SRC, false>), grid, blk, 0, st, a);
}

int launch_unproject(int model, const vg::UnprojectArgs &a, hipStream_t st)
{
    const dim3 grid((unsigned)((a.n + vg::kConvertLanes - 1) / vg::kConvertLanes)), blk(vg::kConvertLanes);
    if (!vg::dispatch_model(model, vg::AllModels{},
                            [&](auto m) { hipLaunchKernelGGL((vg::vg_unproject_kernel<decltype(m)::value>), grid, blk, 0, st, a); }))
        return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
    VG_HIP(hipGetLastError());
    return VG_OK;
}

// paraxial focal lengths: what the model's (fu, fv) are worth next to the optical axis
void paraxial_focal(int model, const double *p, double *f0)
{
    const int K = vg::num_intrinsics(model);
    const double s = (model == VG_MODEL_UCM || model == VG_MODEL_MEI || model == VG_MODEL_DS) ? 1. + p[0] : 1.;
    f0[0] = p[K - 4] / s;
    f0[1] = p[K - 3] / s;
}

// ---------------------------------------------------------------------------------------------- the fit
struct Fit {
    int dst_model = 0, K = 0, S = 0, n = 0, blocks = 0;
    hipStream_t st = nullptr;
    vgi::DeviceMem<double> d_rays, d_uv, d_out, d_res;   // d_out: [blocks][S] partial rows | the lowest failed sample (8 bytes)
    std::vector<double> h_out;

    // sums [S] at x; *bad = the lowest sample that does not project, or -1
    int evaluate(const double *x, double *sums, int *bad, double *d_residuals)
    {
        vg::ConvertEvalArgs a;
        copy_intrinsics(dst_model, x, a.intr);
        a.n = n;
        a.rays = d_rays;
        a.uv = d_uv;
        a.partials = d_out;
        a.first_bad = reinterpret_cast<int *>(d_out.get() + (size_t)blocks * S);
        a.residuals = d_residuals;
        VG_HIP(hipMemsetAsync(a.first_bad, 0x7f, sizeof(double), st));   // 0x7f7f7f7f: above every sample index
        const dim3 grid((unsigned)blocks), blk(vg::kConvertLanes);
        if (!vg::dispatch_model(dst_model, vg::AllModels{},
                                [&](auto m) { hipLaunchKernelGGL((vg::vg_convert_eval_kernel<decltype(m)::value>), grid, blk, 0, st, a); }))
            return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
        VG_HIP(hipGetLastError());
        VG_HIP(hipMemcpyAsync(h_out.data(), d_out.get(), sizeof(double) * h_out.size(), hipMemcpyDeviceToHost, st));
        VG_HIP(hipStreamSynchronize(st));
        for (int q = 0; q < S; q++) {   // the partial rows in index order
            double v = 0.;
            for (int b = 0; b < blocks; b++) v += h_out[(size_t)b * S + q];
            sums[q] = v;
        }
        int fb;
        std::memcpy(&fb, &h_out[(size_t)blocks * S], sizeof fb);
        *bad = fb < n ? fb : -1;
        return VG_OK;
    }
};

bool valid_tolerance(double t) { return t >= 0.; }   // false for NaN

}  // namespace

extern "C" {

int vg_unproject(int device, void *hip_stream, int model, const double *intrinsics, int64_t n, const double *uv, double *rays,
                 uint8_t *ok)
{
    if (vg::num_intrinsics(model) < 0) return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
    if (n < 0 || n > (int64_t)INT32_MAX) return fail(VG_ERR_INVALID_ARGUMENT, "the pixel count must be in [0, 2^31)");
    if (!intrinsics || (n > 0 && (!uv || !rays || !ok))) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (const int rc = vgi::check_device(device, "unprojection")) return rc;
    if (n == 0) return VG_OK;
    vg::UnprojectArgs a;
    copy_intrinsics(model, intrinsics, a.intr);
    a.n = n;
    a.uv = uv;
    a.rays = rays;
    a.ok = ok;
    VG_HIP(hipSetDevice(device));
    return launch_unproject(model, a, reinterpret_cast<hipStream_t>(hip_stream));
}

int vg_convert_map(int device, void *hip_stream, int dst_model, const double *dst_intrinsics, int src_model, const double *src_intrinsics,
                   const double *rotvec3, int width, int height, float *map_x, float *map_y)
{
    if (vg::num_intrinsics(dst_model) < 0 || vg::num_intrinsics(src_model) < 0) return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
    if (!dst_intrinsics || !src_intrinsics || !map_x || !map_y) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!valid_dim(width) || !valid_dim(height)) return fail(VG_ERR_INVALID_ARGUMENT, "map sides must be in [1, 16384]");
    if (rotvec3 && !(std::isfinite(rotvec3[0]) && std::isfinite(rotvec3[1]) && std::isfinite(rotvec3[2])))
        return fail(VG_ERR_INVALID_ARGUMENT, "the rotation vector must be finite");
    if (const int rc = vgi::check_device(device, "camera model conversion")) return rc;
    vg::ConvertMapArgs a;
    copy_intrinsics(dst_model, dst_intrinsics, a.dst_intr);
    copy_intrinsics(src_model, src_intrinsics, a.src_intr);
    const double zero[3] = {0., 0., 0.}, *rot = rotvec3 ? rotvec3 : zero;
    const vg::RotTrig g = vg::rot_trig(rot, true, false);
    vg::rotation_matrix(rot, 1., g, a.R);
    a.width = width;
    a.height = height;
    a.map_x = map_x;
    a.map_y = map_y;
    const bool vec = width % vg::kRectPix == 0 && aligned16(map_x) && aligned16(map_y);
    VG_HIP(hipSetDevice(device));
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    const bool known = vg::dispatch_model(dst_model, vg::AllModels{}, [&](auto d) {
        vg::dispatch_model(src_model, vg::AllModels{}, [&](auto s) { launch_map<decltype(d)::value, decltype(s)::value>(a, vec, st); });
    });
    if (!known) return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
    VG_HIP(hipGetLastError());
    return VG_OK;
}

int vg_convert_start(int src_model, const double *src_intrinsics, int dst_model, double *dst_intrinsics)
{
    const int Ks = vg::num_intrinsics(src_model), Kd = vg::num_intrinsics(dst_model);
    if (Ks < 0 || Kd < 0) return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
    if (!src_intrinsics || !dst_intrinsics) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    double f0[2];
    paraxial_focal(src_model, src_intrinsics, f0);
    double *o = dst_intrinsics;
    for (int k = 0; k < Kd; k++) o[k] = 0.;
    const double twice = (dst_model == VG_MODEL_UCM || dst_model == VG_MODEL_MEI) ? 2. : 1.;   // xi = 1: f = (1 + xi) f0
    if (dst_model == VG_MODEL_EUCM) {
        o[0] = 0.5;
        o[1] = 1.;
    } else if (dst_model == VG_MODEL_UCM || dst_model == VG_MODEL_MEI) {
        o[0] = 1.;
    } else if (dst_model == VG_MODEL_DS) {
        o[1] = 0.5;
    }   // Kannala-Brandt: k1 = ... = k4 = 0
    o[Kd - 4] = twice * f0[0];
    o[Kd - 3] = twice * f0[1];
    o[Kd - 2] = src_intrinsics[Ks - 2];
    o[Kd - 1] = src_intrinsics[Ks - 1];
    return VG_OK;
}

void vg_convert_fit_default_options(vg_convert_fit_options *o)
{
    if (!o) return;
    o->grid_w = 64;
    o->grid_h = 40;
    o->max_angle = vg::kUnprojectPi;
    o->max_iterations = 100;
    o->function_tolerance = 1e-6;   // Ceres' defaults
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->use_bounds = 1;
}

int vg_convert_fit(int device, void *hip_stream, int src_model, const double *src_intrinsics, int width, int height, int dst_model,
                   double *dst_intrinsics, const vg_convert_fit_options *options, vg_convert_fit_summary *summary)
{
    const int Ks = vg::num_intrinsics(src_model), K = vg::num_intrinsics(dst_model);
    if (Ks < 0 || K < 0) return fail(VG_ERR_INVALID_ARGUMENT, "unknown camera model");
    if (!src_intrinsics || !dst_intrinsics) return fail(VG_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!valid_dim(width) || !valid_dim(height)) return fail(VG_ERR_INVALID_ARGUMENT, "image sides must be in [1, 16384]");
    vg_convert_fit_options opt;
    vg_convert_fit_default_options(&opt);
    if (options) opt = *options;
    if (opt.grid_w < 1 || opt.grid_h < 1 || (int64_t)opt.grid_w * (int64_t)opt.grid_h > (int64_t)vg::kConvertMaxGrid)
        return fail(VG_ERR_INVALID_ARGUMENT, "grid_w and grid_h must be at least 1 and their product at most 2^20");
    if (!(opt.max_angle > 0.)) return fail(VG_ERR_INVALID_ARGUMENT, "max_angle must be positive");
    if (opt.max_iterations < 0) return fail(VG_ERR_INVALID_ARGUMENT, "max_iterations must not be negative");
    if (!valid_tolerance(opt.function_tolerance) || !valid_tolerance(opt.gradient_tolerance) || !valid_tolerance(opt.parameter_tolerance))
        return fail(VG_ERR_INVALID_ARGUMENT, "tolerances must not be negative");
    if (const int rc = vgi::check_device(device, "camera model conversion")) return rc;
    VG_HIP(hipSetDevice(device));
    int rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);

    // ---- the samples: pixel centres of a grid_w x grid_h grid, unprojected once by the source camera
    const int G = opt.grid_w * opt.grid_h;
    std::vector<double> uv((size_t)G * 2), rays((size_t)G * 3), res;
    std::vector<uint8_t> ok((size_t)G);
    Fit f;
    vgi::DeviceMem<uint8_t> d_ok;
    vgi::StreamDrain drain{st};   // declared last: a failure path waits for the queued copies before their arrays go
    for (int b = 0; b < opt.grid_h; b++)
        for (int a = 0; a < opt.grid_w; a++) {
            uv[2 * ((size_t)b * opt.grid_w + a)] = (a + 0.5) * width / opt.grid_w - 0.5;
            uv[2 * ((size_t)b * opt.grid_w + a) + 1] = (b + 0.5) * height / opt.grid_h - 0.5;
        }
    f.st = st;
    f.dst_model = dst_model;
    f.K = K;
    f.S = K * (K + 1) / 2 + K + 1;
    VG_HIP(f.d_uv.alloc(sizeof(double) * uv.size()));
    VG_HIP(f.d_rays.alloc(sizeof(double) * rays.size()));
    VG_HIP(d_ok.alloc(ok.size()));
    VG_HIP(hipMemcpyAsync(f.d_uv.get(), uv.data(), sizeof(double) * uv.size(), hipMemcpyHostToDevice, st));
    {
        vg::UnprojectArgs a;
        copy_intrinsics(src_model, src_intrinsics, a.intr);
        a.n = G;
        a.uv = f.d_uv;
        a.rays = f.d_rays;
        a.ok = d_ok;
        if ((rc = launch_unproject(src_model, a, st)) != VG_OK) return rc;
    }
    VG_HIP(hipMemcpyAsync(rays.data(), f.d_rays.get(), sizeof(double) * rays.size(), hipMemcpyDeviceToHost, st));
    VG_HIP(hipMemcpyAsync(ok.data(), d_ok.get(), ok.size(), hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    // kept: unprojected and no further than max_angle from the axis; compacted in raster order
    int kept = 0;
    for (int i = 0; i < G; i++) {
        if (!ok[(size_t)i]) continue;
        const double z = rays[3 * (size_t)i + 2];
        const double angle = std::acos(z < -1. ? -1. : (z > 1. ? 1. : z));
        if (!(angle <= opt.max_angle)) continue;
        for (int k = 0; k < 3; k++) rays[3 * (size_t)kept + k] = rays[3 * (size_t)i + k];
        for (int k = 0; k < 2; k++) uv[2 * (size_t)kept + k] = uv[2 * (size_t)i + k];
        kept++;
    }
    if (summary) {
        std::memset(summary, 0, sizeof *summary);
        summary->kept = kept;
        summary->dropped = G - kept;
        summary->termination = VG_TERM_FAILURE;
    }
    if (2 * kept < K) {
        char msg[160];
        std::snprintf(msg, sizeof msg, "%d of %d samples kept: %d residuals cannot determine %d intrinsics", kept, G, 2 * kept, K);
        return fail(VG_ERR_INVALID_ARGUMENT, msg);
    }
    f.n = kept;
    f.blocks = (kept + vg::kConvertLanes - 1) / vg::kConvertLanes;
    f.h_out.assign((size_t)f.blocks * f.S + 1, 0.);
    VG_HIP(f.d_out.alloc(sizeof(double) * f.h_out.size()));
    VG_HIP(f.d_res.alloc(sizeof(double) * 2 * (size_t)kept));
    VG_HIP(hipMemcpyAsync(f.d_rays.get(), rays.data(), sizeof(double) * 3 * (size_t)kept, hipMemcpyHostToDevice, st));
    VG_HIP(hipMemcpyAsync(f.d_uv.get(), uv.data(), sizeof(double) * 2 * (size_t)kept, hipMemcpyHostToDevice, st));

    // ---- the start
    double x[vg::kConvertMaxK], xc[vg::kConvertMaxK], lo[vg::kConvertMaxK], hi[vg::kConvertMaxK];
    if (std::isnan(dst_intrinsics[0])) {
        if ((rc = vg_convert_start(src_model, src_intrinsics, dst_model, x)) != VG_OK) return rc;
    } else {
        for (int k = 0; k < K; k++) x[k] = dst_intrinsics[k];
    }
    for (int k = 0; k < K; k++) {
        if (!std::isfinite(x[k])) return fail(VG_ERR_INVALID_ARGUMENT, "the start of the fit is not finite");
        if ((rc = vg_intrinsic_bounds(dst_model, k, &lo[k], &hi[k])) != VG_OK) return rc;
    }
    const int S = f.S;
    double sums[vg::kConvertMaxSums], sums_c[vg::kConvertMaxSums];
    int bad;
    if ((rc = f.evaluate(x, sums, &bad, nullptr)) != VG_OK) return rc;
    if (bad >= 0) {
        char msg[200];
        std::snprintf(msg, sizeof msg, "the start of the fit cannot project kept sample %d (pixel %.6g, %.6g)", bad, uv[2 * (size_t)bad],
                      uv[2 * (size_t)bad + 1]);
        return fail(VG_ERR_NUMERIC, msg);
    }
    if (!std::isfinite(sums[S - 1])) return fail(VG_ERR_NUMERIC, "the cost at the start of the fit is not finite");

    // ---- the trust-region rule of vg_lmn.hpp with no eliminated block; candidates on the vg_intrinsic_bounds box with the
    // active set of the calibration's host loop (vg_lm_host_loop.hpp: a parameter on a bound whose step points outwards is held)
    const vglmn::Rule rule{opt.max_iterations, opt.function_tolerance, opt.gradient_tolerance, opt.parameter_tolerance,
                           1e4, 1e16, 1e-32, 1e-3, 1e-6, 1e32};
    vglmn::State s;
    vglmn::start(rule, s, sums[S - 1]);
    const double initial_cost = s.cost;
    const int T = K * (K + 1) / 2;
    while (!s.done) {
        double A[vg::kConvertMaxK * vg::kConvertMaxK], Sw[vg::kConvertMaxK * vg::kConvertMaxK], rw[vg::kConvertMaxK], D[vg::kConvertMaxK];
        const double *g = sums + T;
        int q = 0;
        for (int r = 0; r < K; r++)
            for (int c = r; c < K; c++, q++) A[r * K + c] = A[c * K + r] = sums[q];
        const double mu = 1. / s.radius;
        for (int k = 0; k < K; k++) {
            D[k] = vglmn::clamp_diag(rule, A[k * K + k]);
            A[k * K + k] += mu * D[k];
        }
        vglmn::Step step;
        bool held[vg::kConvertMaxK] = {false};
        for (int pass = 0; pass <= K; pass++) {
            for (int k = 0; k < K * K; k++) Sw[k] = A[k];
            for (int k = 0; k < K; k++) rw[k] = g[k];
            for (int k = 0; k < K; k++)
                if (held[k]) {
                    for (int j = 0; j < K; j++) Sw[k * K + j] = Sw[j * K + k] = 0.;
                    Sw[k * K + k] = 1.;
                    rw[k] = 0.;
                }
            vglmn::dense_step(K, Sw, rw, mu, step);
            bool changed = false;
            if (step.ok && opt.use_bounds)
                for (int k = 0; k < K; k++) {
                    if (held[k]) continue;
                    if ((x[k] <= lo[k] && step.dx[k] < 0.) || (x[k] >= hi[k] && step.dx[k] > 0.)) {
                        held[k] = true;
                        changed = true;
                    }
                }
            if (!changed) break;
        }
        vglmn::head_sums(K, x, g, D, step, xc);
        if (opt.use_bounds) {
            step.gmax = 0.;   // the projected gradient |Project(x - g) - x|, as the host loop measures a bounded parameter's
            for (int k = 0; k < K; k++) {
                xc[k] = xc[k] < lo[k] ? lo[k] : (xc[k] > hi[k] ? hi[k] : xc[k]);
                double xg = x[k] - g[k];
                xg = xg < lo[k] ? lo[k] : (xg > hi[k] ? hi[k] : xg);
                step.gmax = std::fmax(step.gmax, std::fabs(xg - x[k]));
            }
        }
        double cost_c = 0.;
        if (step.ok) {
            if ((rc = f.evaluate(xc, sums_c, &bad, nullptr)) != VG_OK) return rc;
            cost_c = bad >= 0 ? INFINITY : sums_c[S - 1];   // a candidate that loses a sample is rejected
        }
        if (vglmn::accept(rule, s, step, cost_c)) {
            for (int k = 0; k < K; k++) x[k] = xc[k];
            for (int k = 0; k < S; k++) sums[k] = sums_c[k];
        }
    }

    // ---- the last evaluation: the residuals of the returned point
    if ((rc = f.evaluate(x, sums, &bad, f.d_res)) != VG_OK) return rc;
    res.resize(2 * (size_t)kept);
    VG_HIP(hipMemcpyAsync(res.data(), f.d_res.get(), sizeof(double) * res.size(), hipMemcpyDeviceToHost, st));
    VG_HIP(hipStreamSynchronize(st));
    drain.armed = false;
    double sum2 = 0., max2 = 0.;
    for (int i = 0; i < kept; i++) {
        const double r2 = res[2 * (size_t)i] * res[2 * (size_t)i] + res[2 * (size_t)i + 1] * res[2 * (size_t)i + 1];
        sum2 += r2;
        max2 = r2 > max2 ? r2 : max2;
    }
    for (int k = 0; k < K; k++) dst_intrinsics[k] = x[k];
    if (summary) {
        summary->iterations = s.iterations;
        summary->termination = s.term;
        summary->initial_cost = initial_cost;
        summary->final_cost = sums[S - 1];
        summary->rms = std::sqrt(sum2 / kept);
        summary->max_residual = std::sqrt(max2);
    }
    return VG_OK;
}

}  // extern "C"
