// vg_hough.hpp -- fisheye line detection: the reference's hough_test (test/reconstruction/hough_test.cpp) on the EUCM device
// functions of vg_stereo_device.hpp.
//   hough_vote_kernel     Sobel from a row tile with halo, the threshold on the exact integer gradient, the FP64 chain from the
//                         pixel to its plane's normal (.cpp:380-420) and an integer atomicAdd into the image's accumulator
//   hough_blur_kernel     one pass of the separable Gaussian under the float rule of the corner detector:
//                         weights rounded to float, taps summed in order, no FMA, BORDER_REFLECT_101; row pass, then column pass
//   hough_maxima_kernel   the (2 s + 1)^2 test, the 3 x 3 centroid and the accumulator camera's reconstruction per kept bin
//                         (.cpp:458-482), compacted in raster order (count / scan / place, vg_compact.hpp): no atomics
// and, on the host, computePolynomial, findTerminalPoints and the trace (.cpp:31-91, 100-283, 499-536).  Integer adds commute,
// so the accumulator is the same on every run; everything else is evaluated in the order written (-ffp-contract=off), so
// tests/hough_ref.py agrees bit for bit.
#pragma once

#include <cmath>
#include <limits>

#include "vg_compact.hpp"
#include "vg_image_device.hpp"

namespace vgh {

using namespace vgs;

constexpr int kLanes = 256;
constexpr int kTileW = 64, kTileH = 16;   // one wave per image row of the tile, four rows per lane
constexpr int kCounts = 6;
constexpr int kMaxBlur = 15;
enum : int { kSelected = 0, kNotReconstructed = 1, kFirstCast = 2, kAntipodeCast = 3, kFailed = 4, kOutside = 5 };
enum : int { kVoteCast = 0, kVoteFailed = 1, kVoteOutside = 2 };

struct BlurWeights {
    float w[kMaxBlur];
    int n;
};

// what every kernel reads about one handle (host-built, passed by value)
struct Geom {
    double cam[6], acc_cam[6];
    int width, height, acc_w, acc_h;
    int margin, search_size;
    double grad_thresh, acc_thresh, acc_delta_thresh, horizon_ratio;
};

// one vote: the bin of the normal's projection through the accumulator camera.  A failed projection casts nothing (the
// reference votes at a stale point); so does a point outside the accumulator (the reference writes out of bounds), NaN included.
VGS_HD int vote_bin(const Geom &g, const double *ABC, int &bin)
{
    double q[2];
    if (!eucm_project(g.acc_cam, ABC, q)) return kVoteFailed;
    const double cu = round(q[0]), cv = round(q[1]);   // C round: half away from zero
    if (!(cu >= 0. && cu < (double)g.acc_w && cv >= 0. && cv < (double)g.acc_h)) return kVoteOutside;
    bin = (int)cv * g.acc_w + (int)cu;
    return kVoteCast;
}

// .cpp:386-406: the normal of the plane through the projection centre that contains the edge at (u, v); kx, ky: the integer
// Sobel sums, the gradient is k / 2048 (exact in float and in double)
VGS_HD bool edge_plane(const Geom &g, int u, int v, int kx, int ky, double *ABC)
{
    double X[3];
    if (!eucm_reconstruct(g.cam, (double)u, (double)v, X)) return false;
    const double alpha = g.cam[0], beta = g.cam[1], gamma = 1. - alpha;
    const double x = X[0], y = X[1], z = X[2];
    const double Kx = 2 * alpha * alpha * beta * x;
    const double Ky = 2 * alpha * alpha * beta * y;
    const double P = 2 * (alpha - gamma);
    const double Q = 2 * gamma;
    const double fx = (double)kx / 2048., fy = (double)ky / 2048.;
    const double Y[3] = {-fy * (P * z + Q), fx * (P * z + Q), fy * Kx - fx * Ky};
    ABC[0] = X[1] * Y[2] - X[2] * Y[1];
    ABC[1] = X[2] * Y[0] - X[0] * Y[2];
    ABC[2] = X[0] * Y[1] - X[1] * Y[0];
    if (ABC[2] < 0)
        for (int i = 0; i < 3; i++) ABC[i] *= -1;
    return true;
}

struct VoteArgs {
    Geom g;
    int tiles_x;
    const uint8_t *images;        // [n][height][width]
    int32_t *acc;                 // [n][acc_h][acc_w], zero on entry
    unsigned long long *counts;   // [n][kCounts], or nullptr
};

// the votes of one wave, bin < 0 for none.  Equal bins are added inside the wave first: the wave loops over its distinct bins and
// the first lane of each issues one atomic with the number of its lanes (the pixels of one edge vote into a handful of bins).
// Against one atomic per vote the kernel is 4-5 x faster on a single long edge and 1.2-1.5 x slower where every lane has a bin of
// its own.  Every lane of the wave calls this.
__device__ __forceinline__ void cast_votes(int32_t *acc, int bin)
{
    unsigned long long todo = __ballot(bin >= 0);
    while (todo) {   // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const int b = __shfl(bin, leader);
        const unsigned long long same = __ballot(bin == b);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(acc + b, (int)__popcll(same));
        todo &= ~same;
    }
}

// One workgroup: a 64 x 16 tile of one image, its one-pixel halo in LDS.  Wave w takes rows 4 w .. 4 w + 3, one row at a time.
__global__ __launch_bounds__(kLanes) void hough_vote_kernel(VoteArgs a)
{
    __shared__ uint8_t in[kTileH + 2][kTileW + 4];
    const Geom &g = a.g;
    const int64_t item = blockIdx.y;
    const int t = threadIdx.x, W = g.width, H = g.height;
    const int tx0 = ((int)blockIdx.x % a.tiles_x) * kTileW, ty0 = ((int)blockIdx.x / a.tiles_x) * kTileH;
    const uint8_t *src = a.images + item * ((int64_t)W * H);
    for (int k = t; k < (kTileH + 2) * (kTileW + 2); k += kLanes) {
        const int r = k / (kTileW + 2), c = k % (kTileW + 2);
        // clamped into the image so that every load is unconditional: margin >= 1, so no visited pixel reads a clamped one
        const int y = min(max(ty0 - 1 + r, 0), H - 1), x = min(max(tx0 - 1 + c, 0), W - 1);
        in[r][c] = src[(int64_t)y * W + x];
    }
    __syncthreads();
    int32_t *acc = a.acc + item * ((int64_t)g.acc_w * g.acc_h);
    const int col = t % kTileW, row0 = (t / kTileW) * 4;
    int cnt[kCounts] = {0, 0, 0, 0, 0, 0};
    for (int q = 0; q < 4; q++) {
        const int u = tx0 + col, v = ty0 + row0 + q, r = row0 + q + 1, c = col + 1;
        int bin1 = -1, bin2 = -1;
        if (u >= g.margin && u < W - g.margin && v >= g.margin && v < H - g.margin) {
            // Sobel 3 x 3 (.cpp:363-364), |k| <= 1020
            const int kx = ((int)in[r - 1][c + 1] - (int)in[r - 1][c - 1]) + 2 * ((int)in[r][c + 1] - (int)in[r][c - 1]) +
                           ((int)in[r + 1][c + 1] - (int)in[r + 1][c - 1]);
            const int ky = ((int)in[r + 1][c - 1] - (int)in[r - 1][c - 1]) + 2 * ((int)in[r + 1][c] - (int)in[r - 1][c]) +
                           ((int)in[r + 1][c + 1] - (int)in[r - 1][c + 1]);
            // gnorm = (kx^2 + ky^2) / 2^22 is exact in float (the sum is below 2^24), and so is the comparison in double
            if (!((double)(kx * kx + ky * ky) / 4194304. < g.grad_thresh)) {
                cnt[kSelected]++;
                double ABC[3];
                if (!edge_plane(g, u, v, kx, ky, ABC)) {
                    cnt[kNotReconstructed]++;
                } else {
                    const int s1 = vote_bin(g, ABC, bin1);
                    cnt[kFirstCast] += s1 == kVoteCast;
                    cnt[kFailed] += s1 == kVoteFailed;
                    cnt[kOutside] += s1 == kVoteOutside;
                    // 0 / 0 for a zero normal: NaN compares false and no antipode vote is cast
                    if (ABC[2] * ABC[2] / (ABC[0] * ABC[0] + ABC[1] * ABC[1]) < g.horizon_ratio) {
                        const double anti[3] = {-ABC[0], -ABC[1], -ABC[2]};
                        const int s2 = vote_bin(g, anti, bin2);
                        cnt[kAntipodeCast] += s2 == kVoteCast;
                        cnt[kFailed] += s2 == kVoteFailed;
                        cnt[kOutside] += s2 == kVoteOutside;
                    }
                }
            }
        }
        cast_votes(acc, bin1);
        cast_votes(acc, bin2);
    }
    if (a.counts)
        for (int k = 0; k < kCounts; k++) count_wave(a.counts + item * kCounts + k, cnt[k]);
}

// one pass over all items: along the rows (COLUMN = false, from the int32 accumulator) or along the columns (from the row pass).
// The handle refuses an accumulator side below the blur's radius r + 1, so the overhang r stays below the side and reflect101's
// clamp never acts.
template <bool COLUMN, class T>
__global__ __launch_bounds__(kLanes) void hough_blur_kernel(const T *in, float *out, int w, int h, BlurWeights bw)
{
    const int64_t bins = (int64_t)w * h, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (pix >= bins) return;
    const int x = (int)(pix % w), y = (int)(pix / w), r = bw.n / 2;
    const T *src = in + (int64_t)blockIdx.y * bins;
    float acc = 0.f;
    for (int i = 0; i < bw.n; i++) {
        const int64_t o = COLUMN ? (int64_t)reflect101(y - r + i, h) * w + x : (int64_t)y * w + reflect101(x - r + i, w);
        const float tap = bw.w[i] * (float)src[o];
        acc = i == 0 ? tap : acc + tap;
    }
    out[(int64_t)blockIdx.y * bins + pix] = acc;
}

struct LineRec {
    double u, v, val, n[3];   // the centroid, the blurred value, accCam.reconstructPoint(centroid), not normalised
};

struct MaximaArgs {
    Geom g;
    const float *blur;              // [n][acc_h][acc_w]
    unsigned *block_counts;         // [n][blocks]
    const unsigned *block_offsets;  // [n][blocks], scanned per item
    int max_lines;
    LineRec *recs;                  // [n][max_lines]
};

// .cpp:462-482 at one bin of the blurred accumulator
VGS_HD bool maximum_at(const Geom &g, const float *acc, int u, int v, LineRec &rec)
{
    const int s = g.search_size, w = g.acc_w;
    if (u < s || u >= g.acc_w - s || v < s || v >= g.acc_h - s) return false;
    const double val = acc[(int64_t)v * w + u];
    if (val < g.acc_thresh) return false;
    for (int du = -s; du <= s; du++)
        for (int dv = -s; dv <= s; dv++) {
            if (du == 0 && dv == 0) continue;
            if (val <= (double)acc[(int64_t)(v + dv) * w + (u + du)] + g.acc_delta_thresh) return false;
        }
    double uAcc = 0, vAcc = 0, numAcc = 0;   // subpixel (.cpp:286-311)
    for (int du = -1; du <= 1; du++)
        for (int dv = -1; dv <= 1; dv++) {
            const double x = acc[(int64_t)(v + dv) * w + (u + du)];
            numAcc += x;
            uAcc += du * x;
            vAcc += dv * x;
        }
    rec.u = u + uAcc / numAcc;
    rec.v = v + vAcc / numAcc;
    rec.val = val;
    if (!eucm_reconstruct(g.acc_cam, rec.u, rec.v, rec.n)) return false;   // the reference goes on with an unset vector
    return !(rec.n[2] < 0);
}

// Pass 1 (WRITE = false): the kept bins of every block of 256; pass 2: their raster-ordered places from the per-item scan, the
// first max_lines of an item written.
template <bool WRITE>
__global__ __launch_bounds__(kLanes) void hough_maxima_kernel(MaximaArgs a)
{
    const Geom &g = a.g;
    const int64_t item = blockIdx.y, bins = (int64_t)g.acc_w * g.acc_h, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    LineRec rec;
    const bool keep = pix < bins && maximum_at(g, a.blur + item * bins, (int)(pix % g.acc_w), (int)(pix / g.acc_w), rec);
    const unsigned pos = vgc::block_place<WRITE, kLanes>(keep, item * gridDim.x + blockIdx.x, a.block_counts, a.block_offsets);
    if (!WRITE || !keep) return;
    if (pos < (unsigned)a.max_lines) a.recs[item * a.max_lines + pos] = rec;
}

// ---- host: the geometry of one detected line

// computePolynomial (.cpp:31-91): the conic of the plane's image, k1 in closed form
inline Poly2 polynomial(const double *p, const double *plane)
{
    const double alpha = p[0], beta = p[1], fu = p[2], fv = p[3], u0 = p[4], v0 = p[5];
    const double gamma = 1 - alpha, ag = alpha - gamma, a2b = alpha * alpha * beta;
    const double fufv = fu * fv, fufu = fu * fu, fvfv = fv * fv;
    const double A = plane[0], B = plane[1], C = plane[2];
    const double AA = A * A, BB = B * B, CC = C * C;
    const double CCfufv = CC * fufv;
    const double dd = CCfufv / (AA + BB);   // squared distance to the projection centre in pixels
    Poly2 s;
    if ((AA + BB) > 0 && dd < 1.) {   // the curve passes through the projection centre
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
        s.k1 = (A * A * fv * fv * u0 * u0 * (alpha - gamma) + 2 * A * B * fu * fv * u0 * v0 * (alpha - gamma) +
                2 * A * C * fu * fv * fv * gamma * u0 + B * B * fu * fu * v0 * v0 * (alpha - gamma) + 2 * B * C * fu * fu * fv * gamma * v0 +
                C * C * alpha * alpha * beta * fu * fu * v0 * v0 + C * C * alpha * alpha * beta * fv * fv * u0 * u0 - C * C * fu * fu * fv * fv) /
               (C * C * fu * fu * fv * fv);
    }
    return s;
}

constexpr double kNotValid = -1, kBothValid = -2;

inline bool solve_quadratic(double A, double B, double C, double &x1, double &x2)
{
    if (std::fabs(A) < 1e-8) {
        x1 = -C / B;
        x2 = -std::numeric_limits<double>::max();
        return true;
    }
    const double Delta = B * B - 4 * A * C;
    if (Delta < 0) return false;
    const double Ainv = 0.5 / A;
    const double sqrtDelta = std::sqrt(Delta);
    x1 = (-B + sqrtDelta) * Ainv;
    x2 = (-B - sqrtDelta) * Ainv;
    return true;
}

inline double choose_valid_solution(double valMax, double x1, double x2)
{
    x1 = std::round(x1);
    x2 = std::round(x2);
    const bool valid1 = x1 >= 0 && x1 < valMax, valid2 = x2 >= 0 && x2 < valMax;
    if (valid1 && valid2) return kBothValid;
    if (valid1) return x1;
    if (valid2) return x2;
    return kNotValid;
}

inline double midpoint_check(double x0, double x1, double x2) { return std::fabs(x1 - x0) < std::fabs(x2 - x0) ? x1 : x2; }

inline bool distance_check(const double *cam, double pu, double pv)
{
    const double r2 = cam[2] * cam[3] / (cam[0] * cam[0] * cam[1]);
    pu -= cam[4];
    pv -= cam[5];
    return pu * pu + pv * pv < r2;
}

// one border of findPoint (.cpp:212-242): the curve's crossing of the line "coordinate `fixed_v ? v : u` = c".  A candidate
// exists only when chooseValidSolution yields a root or BOTH_VALID (the reference reads an unset one otherwise).
inline bool border_point(const double *cam, const Poly2 &poly, bool fixed_v, double c, double other_max, double *pt)
{
    const double k2 = fixed_v ? poly.kuu : poly.kvv, k2c = fixed_v ? poly.kvv : poly.kuu;
    const double kl = fixed_v ? poly.ku : poly.kv, klc = fixed_v ? poly.kv : poly.ku;
    const double B = poly.kuv * c + kl;
    const double C = k2c * c * c + klc * c + poly.k1;
    double x1, x2;
    if (!solve_quadratic(k2, B, C, x1, x2)) return false;
    const double res = choose_valid_solution(other_max, x1, x2);
    double x;
    if (res >= 0) x = res;
    else if (res == kBothValid) x = midpoint_check(fixed_v ? cam[4] : cam[5], x1, x2);
    else return false;
    const double cand[2] = {fixed_v ? x : c, fixed_v ? c : x};
    if (!distance_check(cam, cand[0], cand[1])) return false;
    pt[0] = cand[0];
    pt[1] = cand[1];
    return true;
}

// bringToBorder (.cpp:244-272); false: neither border of the point's corner gives a point inside the projection circle
inline bool bring_to_border(const double *cam, int width, int height, const Poly2 &poly, double *pt)
{
    pt[0] = std::round(pt[0]);
    pt[1] = std::round(pt[1]);
    if (pt[0] < width && pt[0] >= 0 && pt[1] < height && pt[1] >= 0) return true;
    const double cu = pt[0] < width / 2 ? 0 : width - 1, cv = pt[1] < height / 2 ? 0 : height - 1;   // integer halves, as there
    return border_point(cam, poly, false, cu, height, pt) || border_point(cam, poly, true, cv, width, pt);
}

// findTerminalPoints (.cpp:100-122, 275-283)
inline bool end_points(const double *cam, int width, int height, const double *n, const Poly2 &poly, double *pt4)
{
    const double r = 1. / (cam[0] * std::sqrt(cam[1]));
    double *p1 = pt4, *p2 = pt4 + 2;
    if (std::fabs(n[0]) + std::fabs(n[1]) < 1e-4) {
        p1[0] = r;
        p1[1] = 0;
        p2[0] = 0;
        p2[1] = r;
    } else {
        const double nrm = std::sqrt(n[0] * n[0] + n[1] * n[1]);
        const double pn[2] = {n[0] / nrm * r, n[1] / nrm * r};
        p1[0] = pn[1] * cam[2] + cam[4];
        p1[1] = -pn[0] * cam[3] + cam[5];
        p2[0] = -pn[1] * cam[2] + cam[4];
        p2[1] = pn[0] * cam[3] + cam[5];
    }
    return bring_to_border(cam, width, height, poly, p1) && bring_to_border(cam, width, height, poly, p2);
}

// .cpp:499-536: the pixels the rasteriser visits from round(pt1) until it is within 2 px (L1) of pt2
inline int trace(const Poly2 &poly, const double *pt4, int max_steps, int32_t *uv)
{
    Raster r;
    r.init((int)std::round(pt4[0]), (int)std::round(pt4[1]), (int)std::round(pt4[2]), (int)std::round(pt4[3]), poly);
    int n = 0;
    for (; n < max_steps && std::fabs(r.u - pt4[2]) + std::fabs(r.v - pt4[3]) > 2; n++) {
        uv[2 * n] = r.u;
        uv[2 * n + 1] = r.v;
        r.step();
    }
    return n;
}

}  // namespace vgh
