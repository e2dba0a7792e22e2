// vg_render.hpp -- the synthetic scene renderer: RenderDevice::fillBuffers and fillImage (src/render/render.cpp:86-193) with
// Plane::intersection (plane.cpp:39-60), Background::intersection (background.cpp:34-56), Texture::sample (texture.cpp:28-70),
// bilinear (include/ocv.h:64-84) and the LookupFilter table (aa_filter_lt.cpp) on the EUCM device functions of
// vg_stereo_device.hpp.  Two launches over all views: the hit buffers (one lane per pixel, every object tested in order), then
// the image.  In the image launch four lanes share a pixel: each takes every fourth row of the nv x nu tap grid, sums it left
// to right and leaves row sum * vKernel in LDS; the pixel's first lane adds the up to 24 products top to bottom, which is the
// reference's summation order.  Four lanes were the fastest of 1, 4, 8 and 16 on the MI355X.
// Evaluated in the order written (-ffp-contract=off); tests/render_ref.py restates the same order.  DESIGN.md section 5.16.
#pragma once

#include "vg_bicubic.hpp"
#include "vg_image_device.hpp"

namespace vgr {

using namespace vgs;

constexpr int kLanes = 256;
constexpr int kRowLanes = 4;                     // lanes per pixel of the image launch; divides the wave
constexpr int kMaxKernel = 24;                   // MAX_SIZE - 1 (aa_filter_lt.h:45)
constexpr int kTableSize = kMaxKernel * (kMaxKernel + 1) / 2;   // kernels 1 .. 24 end to end: 300 doubles
constexpr double kSigma = 0.55;                  // SIGMA (:46)
constexpr int kSampleCount = 600;                // SAMPLE_COUNT (aa_filter_lt.cpp:55)
constexpr double kBackgroundDepth = 150.;        // background.cpp:47
constexpr double kPlaneGate = 0.01;              // plane.cpp:48
constexpr float kDepthInit = 1e6f;               // _depthMat.setTo(1e6)
constexpr int kCounts = 5;                       // not reconstructed, covered by nothing, background, plane, single bicubic tap

VGS_HD int kernel_offset(int length) { return length * (length - 1) / 2; }   // of kernel `length` in the table
VGS_HD double filter_origin(int length) { return 3 * kSigma * (-1 + 1. / length); }   // LookupFilter::computeOrigin
VGS_HD double filter_step(int length) { return 6 * kSigma / length; }                 // computeStep
VGS_HD double filter_radius() { return 5 * kSigma; }                                  // getRadius

// LookupFilter::LookupFilter (aa_filter_lt.cpp:52-103), its loops as written; table: kTableSize doubles.  Host only.
inline void build_filter_table(double *table)
{
    double kernel_data[kSampleCount + 1], integral[kSampleCount + 1];
    integral[0] = 0;
    const double step = filter_step(kSampleCount);
    double x = filter_origin(kSampleCount);
    for (int i = 0; i < kSampleCount; i++, x += step) {
        kernel_data[i] = exp(-x * x / (2 * kSigma * kSigma)) - 0.35 * exp(-x * x / (1.3 * kSigma * kSigma));   // computeKernel
        integral[i + 1] = integral[i] + kernel_data[i];
    }
    kernel_data[kSampleCount] = 0;
    const double normalizer = 1. / integral[kSampleCount];
    integral[kSampleCount] = 1;
    for (int i = 0; i < kSampleCount; i++) {
        integral[i] *= normalizer;
        kernel_data[i] *= normalizer;
    }
    table[0] = 1;
    table[1] = 0.5;
    table[2] = 0.5;
    for (int length = 3; length <= kMaxKernel; length++) {
        const double frac_samples = double(kSampleCount) / length;
        double prev = 0;
        for (int i = 0; i < length; i++) {
            const double frac_idx = frac_samples * (i + 1);
            const int idx = int(frac_idx);
            const double surplus = frac_idx - idx;
            const double cur = integral[idx] + surplus * kernel_data[idx];
            table[kernel_offset(length) + i] = cur - prev;
            prev = cur;
        }
    }
}

enum : int { kBackground = 0, kPlane = 1 };

// one object of the world as the kernels read it: Background / Plane after their constructors
struct Object {
    int kind, cols, rows;
    int64_t texture;           // offset of its [rows][cols] samples in the handle's texture block
    double u0, v0, fu, fv;
    double t[3], ex[3], ey[3], ez[3];
};

struct View {   // _xiCam: rotMat row-major, trans
    double R[9], t[3];
};

struct Args {
    double cam[6];
    int width, height, n_objects;
    int64_t P;
    const Object *objects;     // DEVICE [n_objects]
    const uint8_t *textures;
    const double *table;       // DEVICE [kTableSize]
    const View *views;         // DEVICE [n]
    int16_t *index;            // [n][P], like u and v: the caller's arrays or the handle's
    float *u, *v;
    float *depth;              // [n][P] or NULL
    uint8_t *image;            // [n][P]
    unsigned long long *counts;   // [n][kCounts] or NULL
};

// the bounds test both objects end with.  Written so that a NaN coordinate is outside (the reference's four comparisons let it
// through; finite inputs give none: DESIGN.md section 9)
VGS_HD bool in_texture(const Object &o, const double *uv) { return uv[0] >= 0 && uv[0] <= o.cols - 1 && uv[1] >= 0 && uv[1] <= o.rows - 1; }

// Plane::intersection (plane.cpp:39-60)
VGS_HD bool plane_hit(const Object &o, const double *pos, const double *dir, double *uv, double &depth)
{
    const double d[3] = {o.t[0] - pos[0], o.t[1] - pos[1], o.t[2] - pos[2]};
    const double num = dot3(o.ez, d), den = dot3(o.ez, dir);
    if (den * num < kPlaneGate) return false;
    const double lambda = num / den;
    depth = lambda * sqrt(dot3(dir, dir));
    double pt[3];
    for (int i = 0; i < 3; i++) pt[i] = dir[i] * lambda + pos[i] - o.t[i];
    uv[0] = o.u0 + o.fu * dot3(o.ex, pt);
    uv[1] = o.v0 + o.fv * dot3(o.ey, pt);
    return in_texture(o, uv);
}

// Background::intersection (background.cpp:34-56): _ex, _ey, _ez are the world axes, their dot products written out
VGS_HD bool background_hit(const Object &o, const double *dir, double *uv, double &depth)
{
    const double sphi = o.ex[0] * dir[0] + o.ex[1] * dir[1] + o.ex[2] * dir[2];
    const double cphi = o.ez[0] * dir[0] + o.ez[1] * dir[1] + o.ez[2] * dir[2];
    const double cth = sqrt(sphi * sphi + cphi * cphi);
    const double sth = o.ey[0] * dir[0] + o.ey[1] * dir[1] + o.ey[2] * dir[2];
    depth = kBackgroundDepth;
    const double phi = atan2(sphi, cphi), th = atan2(sth, cth);
    uv[0] = o.u0 + o.fu * phi;
    uv[1] = o.v0 + o.fv * th;
    return in_texture(o, uv);
}

// fillBuffers (render.cpp:86-114): one lane per pixel, views on gridDim.y
__global__ __launch_bounds__(kLanes) void render_buffers_kernel(Args a)
{
    const int64_t item = blockIdx.y, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    int st = -1;   // 0 not reconstructed, 1 nothing, 2 background, 3 plane
    if (pix < a.P) {
        const View &view = a.views[item];
        const int u = (int)(pix % a.width), v = (int)(pix / a.width);
        float best = kDepthInit, bu = 0.f, bv = 0.f;
        int16_t bi = -1;
        double X[3], dir[3];
        st = 0;
        if (eucm_reconstruct(a.cam, (double)u, (double)v, X)) {
            mat_vec(view.R, X, dir);
            for (int k = 0; k < a.n_objects; k++) {
                const Object &o = a.objects[k];
                double uv[2], depth;
                if (!(o.kind == kBackground ? background_hit(o, dir, uv, depth) : plane_hit(o, view.t, dir, uv, depth))) continue;
                if ((double)best > depth) {   // the buffers are float: the stored depth is what the next object meets
                    best = (float)depth;
                    bi = (int16_t)k;
                    bu = (float)uv[0];
                    bv = (float)uv[1];
                }
            }
            st = bi < 0 ? 1 : (a.objects[bi].kind == kBackground ? 2 : 3);
        }
        const int64_t gi = item * a.P + pix;
        a.index[gi] = bi;
        a.u[gi] = bu;
        a.v[gi] = bv;
        if (a.depth) a.depth[gi] = best;
    }
    if (a.counts)
        for (int k = 0; k < 4; k++) count_wave(a.counts + item * kCounts + k, st == k);
}

// bilinear<double>(Mat8u, x, y) (ocv.h:64-84) with its quirks: int() truncates towards zero, so a coordinate in (-1, 0) keeps
// cell 0 and extrapolates; `fail` carries over from u to v, so a u outside [0, cols - 2] also sends v to row 0
VGS_HD double bilinear(const uint8_t *src, int cols, int rows, double x, double y)
{
    int u = (int)x, v = (int)y;
    const double dx = x - u, dy = y - v, dx2 = 1 - dx;
    bool fail = false;
    if (u < 0) {
        fail = true;
        u = 0;
    } else if (u > cols - 2) {
        fail = true;
        u = cols - 1;
    }
    if (fail || v < 0) {
        fail = true;
        v = 0;
    } else if (v > rows - 2) {
        fail = true;
        v = rows - 1;
    }
    if (fail) return (double)src[(int64_t)v * cols + u];
    const uint8_t *r0 = src + (int64_t)v * cols + u, *r1 = r0 + cols;
    const double i00 = r0[0], i01 = r0[1], i10 = r1[0], i11 = r1[1];
    return (i11 * dx + i10 * dx2) * dy + (i01 * dx + i00 * dx2) * (1 - dy);
}

// one row of Texture::sample's tap grid (texture.cpp:55-64): nu taps from pt0 + vidx * vstep, summed left to right
VGS_HD double sample_row(const uint8_t *tex, int cols, int rows, const double *pt0, const double *ustep, const double *vstep, int vidx, int nu,
                         const double *u_kernel)
{
    double pc[2] = {pt0[0] + vidx * vstep[0], pt0[1] + vidx * vstep[1]};
    double ures = 0;
    for (int uidx = 0; uidx < nu; uidx++) {
        ures += bilinear(tex, cols, rows, pc[0], pc[1]) * u_kernel[uidx];
        pc[0] += ustep[0];
        pc[1] += ustep[1];
    }
    return ures;
}

VGS_HD int kernel_length(double e0, double e1)   // min(max(round(|e| * radius), 1.), 24.)
{
    const double r = round(sqrt(e0 * e0 + e1 * e1) * filter_radius());
    return (int)(r < 1. ? 1. : (r > 24. ? 24. : r));
}

// fillImage (render.cpp:116-193) and Texture::sample: kRowLanes lanes per pixel, kLanes / kRowLanes pixels per block
__global__ __launch_bounds__(kLanes) void render_image_kernel(Args a)
{
    constexpr int kPixels = kLanes / kRowLanes;
    __shared__ double s_table[kTableSize];
    __shared__ double s_rows[kPixels][kMaxKernel + 1];   // + 1: rows of neighbouring pixels on other banks
    for (int i = threadIdx.x; i < kTableSize; i += kLanes) s_table[i] = a.table[i];
    __syncthreads();
    const int sub = threadIdx.x % kRowLanes, slot = threadIdx.x / kRowLanes;
    const int64_t item = blockIdx.y, pix = (int64_t)blockIdx.x * kPixels + slot;
    const int16_t *index = a.index + item * a.P;
    const float *um = a.u + item * a.P, *vm = a.v + item * a.P;
    const int idx = pix < a.P ? index[pix] : -1;
    int nu = 1, nv = 1;
    double res = 0;
    const uint8_t *tex = nullptr;
    int cols = 0, rows = 0;
    if (idx >= 0) {
        const Object &o = a.objects[idx];
        tex = a.textures + o.texture;
        cols = o.cols;
        rows = o.rows;
        const int u = (int)(pix % a.width), v = (int)(pix / a.width);
        const double pt[2] = {(double)um[pix], (double)vm[pix]};
        // the local basis: differences to the neighbours that hold the same object, over their number
        double eu[2] = {0, 0}, ev[2] = {0, 0};
        int count = 0;
        double u_min = pt[0], u_max = pt[0], v_min = pt[1], v_max = pt[1];
        if (u > 0 && index[pix - 1] == idx) {
            count++;
            u_min = um[pix - 1];
            v_min = vm[pix - 1];
        }
        if (u < a.width - 1 && index[pix + 1] == idx) {
            count++;
            u_max = um[pix + 1];
            v_max = vm[pix + 1];
        }
        if (count != 0) {
            eu[0] = (u_max - u_min) / count;
            eu[1] = (v_max - v_min) / count;
        }
        count = 0;
        u_min = pt[0], u_max = pt[0], v_min = pt[1], v_max = pt[1];
        if (v > 0 && index[pix - a.width] == idx) {
            count++;
            u_min = um[pix - a.width];
            v_min = vm[pix - a.width];
        }
        if (v < a.height - 1 && index[pix + a.width] == idx) {
            count++;
            u_max = um[pix + a.width];
            v_max = vm[pix + a.width];
        }
        if (count != 0) {
            ev[0] = (u_max - u_min) / count;
            ev[1] = (v_max - v_min) / count;
        }
        nu = kernel_length(eu[0], eu[1]);
        nv = kernel_length(ev[0], ev[1]);
        if (nu == 1 && nv == 1) {
            if (sub == 0) {
                double dr, dc;
                bicubic(tex, cols, rows, pt[1], pt[0], res, dr, dc);
            }
        } else {
            const double su = filter_step(nu), sv = filter_step(nv), ou = filter_origin(nu), ov = filter_origin(nv);
            const double ustep[2] = {eu[0] * su, eu[1] * su}, vstep[2] = {ev[0] * sv, ev[1] * sv};
            const double pt0[2] = {pt[0] + eu[0] * ou + ev[0] * ov, pt[1] + eu[1] * ou + ev[1] * ov};
            const double *u_kernel = s_table + kernel_offset(nu), *v_kernel = s_table + kernel_offset(nv);
            for (int vidx = sub; vidx < nv; vidx += kRowLanes)
                s_rows[slot][vidx] = sample_row(tex, cols, rows, pt0, ustep, vstep, vidx, nu, u_kernel) * v_kernel[vidx];
        }
    }
    __syncthreads();
    if (sub == 0 && idx >= 0 && !(nu == 1 && nv == 1))
        for (int vidx = 0; vidx < nv; vidx++) res += s_rows[slot][vidx];
    if (sub == 0 && pix < a.P) {
        // uchar(min(255., max(res, 0.))): truncated, not rounded; std::max / std::min send a NaN to 255.  Uncovered: 0
        const double hi = res < 0. ? 0. : res, lo = hi < 255. ? hi : 255.;
        a.image[item * a.P + pix] = idx >= 0 ? (uint8_t)lo : (uint8_t)0;
    }
    if (a.counts) count_wave(a.counts + item * kCounts + 4, sub == 0 && idx >= 0 && nu == 1 && nv == 1);
}

}  // namespace vgr
