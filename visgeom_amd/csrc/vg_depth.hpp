// vg_depth.hpp -- depth map propagation and fusion: DepthMap::wrapDepth, merge and filterNoise of the reference
// (src/reconstruction/depth_map.cpp:723-760, 917-958, 868-914) on the EUCM device functions of vg_stereo_device.hpp.
// The warp is a forward splat in three launches over all items: every source min-reduces the bit pattern of its range into a
// 64-bit z-buffer entry of its target, every source whose range won min-reduces its index into a 32-bit winner entry, and
// every target gathers the winner's sigma and cost.  Integer min is commutative, so the map is the one the reference's ascending
// loop with a strict "<" leaves, bit for bit and from run to run.  Merge and the noise filter are one elementwise launch each.
// Evaluated in the order written (-ffp-contract=off), so tests/depth_ref.py agrees bit for bit.
#pragma once

#include "vg_compact.hpp"
#include "vg_image_device.hpp"

namespace vgd {

using namespace vgs;

constexpr double kDefaultSigma = 30.;   // DEFAULT_SIGMA_DEPTH (stereo_misc.h)
constexpr double kDefaultCost = 5.;     // DEFAULT_COST_DEPTH
constexpr int kLanes = 256;
constexpr unsigned long long kZEmpty = ~0ull;
constexpr unsigned kNoWinner = ~0u;

// one item of a warp call, as it goes up and comes back: the pose and the counters (zero on the way up)
struct WarpItem {
    double Rinv[9], t[3];
    unsigned long long counts[6];   // sources, dropped by reconstruct, dropped by project, outside the map, reached a target, targets written
};

struct WarpArgs {
    WarpItem *item;   // DEVICE [n]
    double cam[6];
    Grid g;
    int64_t P;
    const double *depth_in, *sigma_in, *cost_in;   // [n][P]
    unsigned long long *zbuf;                      // [n][P], all ones between calls
    unsigned *winner;                              // [n][P], all ones between calls
    double *depth, *sigma, *cost;                  // [n][P]
    bool count;
#ifdef VG_DEPTH_WARP_STORE
    int *src_target;    // [n][P]: what (a) found per source, -1 for none
    double *src_dist;
#endif
};

enum : int { kNotSource = 0, kDropReconstruct = 1, kDropProject = 2, kOutside = 3, kReached = 4 };

// one source pixel of wrapDepth: its target index and its range in the new frame
VGS_HD int warp_source(const double *cam, const Grid &g, const WarpItem &it, int64_t pix, double d, int64_t &target, double &dist)
{
    if (!(d >= kMinDepth)) return kNotSource;   // getIdxVec (depth_map.cpp:525); false for NaN
    const int x = (int)(pix % g.x_max), y = (int)(pix / g.x_max);
    double X[3], X1[3], X2[3], q[2];
    if (!eucm_reconstruct(cam, (double)(x * g.scale + g.u0), (double)(y * g.scale + g.v0), X)) return kDropReconstruct;
    const double nrm = sqrt(dot3(X, X));
    for (int i = 0; i < 3; i++) X1[i] = X[i] / nrm * d - it.t[i];   // normalized() * depth, then inverseTransform
    mat_vec(it.Rinv, X1, X2);
    if (!eucm_project(cam, X2, q)) return kDropProject;
    dist = sqrt(dot3(X2, X2));
    if (!(dist > 0.)) return kDropProject;   // a point at the new origin: project refuses it already (denom < 1e-3)
    if (!coord_ok(q)) return kOutside;       // NaN or beyond +-2^24, before any conversion to int
    const int xd = round_int((q[0] - g.u0) / g.scale), yd = round_int((q[1] - g.v0) / g.scale);   // xConv, yConv
    if (xd < 0 || xd >= g.x_max || yd < 0 || yd >= g.y_max) return kOutside;
    target = (int64_t)yd * g.x_max + xd;
    return kReached;
}

// (a) the z-buffer: min over the sources of a target of the bits of dist (monotone for positive doubles)
__global__ __launch_bounds__(kLanes) void depth_warp_zbuf_kernel(WarpArgs a)
{
    const int64_t item = blockIdx.y, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    int st = kNotSource;
    if (pix < a.P) {
        int64_t target = 0;
        double dist = 0.;
        st = warp_source(a.cam, a.g, a.item[item], pix, a.depth_in[item * a.P + pix], target, dist);
        if (st == kReached) atomicMin(a.zbuf + item * a.P + target, (unsigned long long)__double_as_longlong(dist));
#ifdef VG_DEPTH_WARP_STORE
        a.src_target[item * a.P + pix] = st == kReached ? (int)target : -1;
        a.src_dist[item * a.P + pix] = dist;
#endif
    }
    if (a.count) {
        unsigned long long *c = a.item[item].counts;
        count_wave(c + 0, st != kNotSource);
        for (int k = kDropReconstruct; k <= kReached; k++) count_wave(c + k, st == k);
    }
}

// (b) the winner: among the sources whose range is the target's minimum, the smallest index.  The source is recomputed
// (8 bytes read again and the arithmetic of (a)); -DVG_DEPTH_WARP_STORE builds the other shape, in which (a) stores the
// target and the range (12 bytes per source) and (b) loads them: DESIGN.md section 5.12.
__global__ __launch_bounds__(kLanes) void depth_warp_winner_kernel(WarpArgs a)
{
    const int64_t item = blockIdx.y, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (pix >= a.P) return;
    int64_t target = 0;
    double dist = 0.;
#ifdef VG_DEPTH_WARP_STORE
    target = a.src_target[item * a.P + pix];
    if (target < 0) return;
    dist = a.src_dist[item * a.P + pix];
#else
    if (warp_source(a.cam, a.g, a.item[item], pix, a.depth_in[item * a.P + pix], target, dist) != kReached) return;
#endif
    if (a.zbuf[item * a.P + target] == (unsigned long long)__double_as_longlong(dist)) atomicMin(a.winner + item * a.P + target, (unsigned)pix);
}

// (c) one lane per target: gather the winner, write the three maps, leave the scratch all ones for the next call
__global__ __launch_bounds__(kLanes) void depth_warp_gather_kernel(WarpArgs a)
{
    const int64_t item = blockIdx.y, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    bool written = false;
    if (pix < a.P) {
        const int64_t gi = item * a.P + pix;
        const unsigned w = a.winner[gi];
        double d = 0., s = kDefaultSigma, c = kDefaultCost;   // DepthMap's initial values
        if (w != kNoWinner) {
            d = __longlong_as_double((long long)a.zbuf[gi]);
            s = a.sigma_in[item * a.P + w] + 0.005 * d;
            c = a.cost_in[item * a.P + w];
            a.zbuf[gi] = kZEmpty;
            a.winner[gi] = kNoWinner;
            written = true;
        }
        a.depth[gi] = d;
        a.sigma[gi] = s;
        a.cost[gi] = c;
    }
    if (a.count) count_wave(a.item[item].counts + 5, written);
}

// DepthMap::merge (depth_map.cpp:917-958), in place on map 1; counts [n][5]: skipped, copied, fused, replaced, kept
__global__ __launch_bounds__(kLanes) void depth_merge_kernel(double *depth, double *sigma, const double *depth2, const double *sigma2,
                                                            int64_t P, unsigned long long *counts)
{
    const int64_t item = blockIdx.y, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    int st = -1;
    if (pix < P) {
        const int64_t gi = item * P + pix;
        const double d2 = depth2[gi];
        st = 0;
        if (!(d2 < kMinDepth || d2 == 0.)) {
            const double s2 = sigma2[gi];
            double d = depth[gi], s = sigma[gi];
            if (d == 0.) {
                d = d2;
                s = s2;
                st = 1;
            } else if (fabs(d - d2) < 2 * (s + s2)) {
                fuse(d, s, d2, s2);
                st = 2;
            } else if (d2 < d) {
                d = d2;
                s = s2;
                st = 3;
            } else {
                st = 4;
            }
            if (st != 4) {
                depth[gi] = d;
                sigma[gi] = s;
            }
        }
    }
    if (counts)
        for (int k = 0; k < 5; k++) count_wave(counts + item * 5 + k, st == k);
}

// DepthMap::filterNoise (depth_map.cpp:868-914): reads (depth_in, sigma_in) only, writes every pixel of (depth, sigma);
// counts [n][3]: interior pixels with a depth, cleared, smoothed
__global__ __launch_bounds__(kLanes) void depth_filter_noise_kernel(const double *depth_in, const double *sigma_in, double *depth, double *sigma,
                                                                   Grid g, int64_t P, unsigned long long *counts)
{
    const int dx[8] = {-1, 0, 1, 1, 1, 0, -1, -1}, dy[8] = {1, 1, 1, 0, -1, -1, -1, 0};
    const int64_t item = blockIdx.y, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    int st = 0;   // 1 cleared, 2 smoothed
    if (pix < P) {
        const double *din = depth_in + item * P, *sin = sigma_in + item * P;
        const int x = (int)(pix % g.x_max), y = (int)(pix / g.x_max);
        double d = din[pix], s = sin[pix];
        if (x >= 1 && x < g.x_max - 1 && y >= 1 && y < g.y_max - 1 && d != 0.) {
            int filled = 0, matches = 0;
            double acc = d * 5;   // CENTRAL_WEIGHT
            for (int i = 0; i < 8; i++) {
                const int64_t j = (int64_t)(y + dy[i]) * g.x_max + (x + dx[i]);
                const double nd = din[j];
                if (nd == 0.) continue;
                filled++;
                const double err = fabs(d - nd);
                if (err > s || err > 3 * sin[j]) continue;
                matches++;
                acc += nd;
            }
            if ((matches < 2 && matches < filled) || filled < 2) {
                d = 0.;
                s = 0.;
                st = 1;
            } else {
                d = acc / (matches + 5);
                st = 2;
            }
        }
        depth[item * P + pix] = d;
        sigma[item * P + pix] = s;
    }
    if (counts) {
        count_wave(counts + item * 3 + 0, st != 0);
        count_wave(counts + item * 3 + 1, st == 1);
        count_wave(counts + item * 3 + 2, st == 2);
    }
}

constexpr int kMaxHyp = 8;   // hypothesis planes of a map: [n][hyp_max][P]

// DepthMap::regularize (depth_map.cpp:960-983), in place: one lane per (item, pixel) walks its planes in ascending order.  A
// plane below MIN_DEPTH takes (depth, sigma, cost) of the first filled plane above it, whose depth is then cleared; its sigma
// and cost stay.  The pixels are independent, so the reference's plane-major loop leaves the same maps.
__global__ __launch_bounds__(kLanes) void depth_regularize_kernel(double *depth, double *sigma, double *cost, int hyp_max, int64_t P)
{
    const int64_t item = blockIdx.y, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (pix >= P) return;
    const int64_t base = item * hyp_max * P + pix;
    for (int h = 0; h < hyp_max - 1; h++) {
        if (!(depth[base + h * P] < kMinDepth)) continue;
        int h2 = h + 1;
        while (h2 < hyp_max && depth[base + h2 * P] < kMinDepth) h2++;
        if (h2 == hyp_max) continue;
        depth[base + h * P] = depth[base + h2 * P];
        sigma[base + h * P] = sigma[base + h2 * P];
        cost[base + h * P] = cost[base + h2 * P];
        depth[base + h2 * P] = 0.;
    }
}

struct PackMhArgs {
    double cam[6];
    Grid g;
    int hyp_max;
    const double *depth, *sigma;    // [hyp_max][P]; sigma may be NULL when sigma_out is
    unsigned *block_counts;         // [blocks]
    const unsigned *block_offsets;
    int32_t *indices, *hyp;         // the pack, each may be NULL
    double *cloud, *sigma_out;
};

// DepthMap::reconstruct(pack, ALL_HYPOTHESES | SIGMA_VALUE) (depth_map.cpp:532-635) of one map, compacted in the reference's
// order: the pixels whose plane 0 holds a depth (getIdxVec) in raster order, and of each its filled planes in ascending order.
// Pass 1 (WRITE = false) counts the entries of every block of 256 pixels; pass 2 places them from the scanned block counts,
// one wave ballot per plane and the lanes below -- the ordered compaction of the photometric data pack (vg_compact.hpp) with
// up to hyp_max entries per lane.
template <bool WRITE>
__global__ __launch_bounds__(kLanes) void depth_pack_mh_kernel(PackMhArgs a)
{
    const int64_t P = (int64_t)a.g.x_max * a.g.y_max, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    const bool query = pix < P && a.depth[pix] >= kMinDepth;
    double d[kMaxHyp];
    unsigned below = 0, total = 0;   // entries of the wave's lower lanes, of the whole wave
#pragma unroll
    for (int h = 0; h < kMaxHyp; h++) {
        d[h] = (query && h < a.hyp_max) ? a.depth[h * P + pix] : 0.;
        const unsigned long long ball = __ballot(d[h] >= kMinDepth);
        below += vgc::lanes_below(ball);
        total += (unsigned)__popcll(ball);
    }
    int64_t pos = vgc::block_place<WRITE, kLanes>(below, total, blockIdx.x, a.block_counts, a.block_offsets);
    if (!WRITE || !query) return;
    const int x = (int)(pix % a.g.x_max), y = (int)(pix / a.g.x_max);
    double X[3], dir[3] = {0., 0., 0.};
    const bool seen = a.cloud && eucm_reconstruct(a.cam, (double)(x * a.g.scale + a.g.u0), (double)(y * a.g.scale + a.g.v0), X);
    if (seen) {
        const double nrm = sqrt(dot3(X, X));
        for (int i = 0; i < 3; i++) dir[i] = X[i] / nrm;   // normalized()
    }
#pragma unroll
    for (int h = 0; h < kMaxHyp; h++) {   // d[h] is 0 from hyp_max on
        if (!(d[h] >= kMinDepth)) continue;
        if (a.indices) a.indices[pos] = (int32_t)pix;
        if (a.hyp) a.hyp[pos] = h;
        if (a.sigma_out) a.sigma_out[pos] = a.sigma[h * P + pix];
        if (a.cloud)
            for (int i = 0; i < 3; i++) a.cloud[3 * pos + i] = seen ? dir[i] * d[h] : 0.;   // a pixel the camera refuses: (0, 0, 0)
        pos++;
    }
}

// ---- point clouds, the plane prior and the accuracy score ------------------------------------------

constexpr double kDefaultDepth = 5.;   // DEFAULT_DEPTH (stereo_misc.h)
constexpr int kMaxPolygon = 16;

enum : unsigned {   // DepthMap's reconstruct flags (depth_map.h:39-49), the values of VG_RECON_*
    kQueryPoints = 1, kImageValues = 2, kMinMax = 4, kAllHypotheses = 8, kDefaultValues = 16, kSigmaValue = 32, kQueryIndices = 64, kIndexMapping = 128
};

struct ReconArgs {
    double cam[6];
    Grid g;
    int64_t P, units;               // pixels of a plane; lanes per item: P, or the queries
    int hyp_max, num_hyps;          // planes of a map, planes read
    unsigned flags;
    const double *depth, *sigma;    // [n][hyp_max][P]; sigma may be NULL when no flag reads it
    const int32_t *query_idx;       // [units] or NULL
    const double *query_pts;        // [units][2] or NULL
    const double *pose;             // [n][12]: rotMat row-major, trans; or NULL
    const unsigned *item_first;     // [n]: the entries of the items in front; NULL for one item
    unsigned *block_counts;         // [n][blocks]
    const unsigned *block_offsets;
    int nb;
    int32_t *indices, *hyp, *index_map, *item;   // the entries, each may be NULL
    double *points, *sigma_out, *cloud;
    uint8_t *valid;
};

// DepthMap::reconstruct(pack, flags) (depth_map.cpp:532-635) of gridDim.y maps, compacted in the reference's order: item after
// item, the queries (or the pixels with a depth in plane 0) in order, of each its planes in ascending order.  One lane per query
// and item holds up to kMaxHyp entries; pass 1 counts, pass 2 places (vg_compact.hpp).  No lane leaves in front of block_place.
template <bool WRITE>
__global__ __launch_bounds__(kLanes) void depth_reconstruct_kernel(ReconArgs a)
{
    const int64_t item = blockIdx.y, unit = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    const double *dep = a.depth + item * a.hyp_max * a.P;
    int64_t pix = -1;
    double pu = 0., pv = 0.;   // the image point the ray goes through
    if (unit < a.units) {
        if (a.flags & kQueryIndices) {
            const int32_t q = a.query_idx[unit];
            if (q >= 0 && q < a.P) pix = q;
        } else if (a.flags & kQueryPoints) {
            pu = a.query_pts[2 * unit];
            pv = a.query_pts[2 * unit + 1];
            const double fx = round((pu - a.g.u0) / a.g.scale), fy = round((pv - a.g.v0) / a.g.scale);   // xConv, yConv; in double
            if (fx >= 0. && fx < (double)a.g.x_max && fy >= 0. && fy < (double)a.g.y_max) pix = (int64_t)fy * a.g.x_max + (int64_t)fx;
        } else if (dep[unit] >= kMinDepth) {   // getIdxVec()
            pix = unit;
        }
    }
    if (pix >= 0 && !((a.flags & kQueryPoints) && !(a.flags & kQueryIndices))) {
        pu = (double)((int)(pix % a.g.x_max) * a.g.scale + a.g.u0);
        pv = (double)((int)(pix / a.g.x_max) * a.g.scale + a.g.v0);
    }
    double d[kMaxHyp];
    unsigned below = 0, total = 0, filled = 0;   // filled: the planes that hold a depth of their own
#pragma unroll
    for (int h = 0; h < kMaxHyp; h++) {
        d[h] = (pix >= 0 && h < a.num_hyps) ? dep[h * a.P + pix] : 0.;
        if (d[h] >= kMinDepth) {
            filled |= 1u << h;
        } else {
            d[h] = (h == 0 && pix >= 0 && (a.flags & kDefaultValues)) ? kDefaultDepth : 0.;
        }
        const unsigned long long ball = __ballot(d[h] >= kMinDepth);
        below += vgc::lanes_below(ball);
        total += (unsigned)__popcll(ball);
    }
    int64_t pos = vgc::block_place<WRITE, kLanes>(below, total, item * a.nb + blockIdx.x, a.block_counts, a.block_offsets);
    if (!WRITE || pix < 0) return;
    if (a.item_first) pos += a.item_first[item];
    const bool minmax = (a.flags & kMinMax) != 0;
    double X[3], dir[3] = {0., 0., 0.};
    const bool seen = eucm_reconstruct(a.cam, pu, pv, X);
    if (seen && a.cloud) {
        const double nrm = sqrt(dot3(X, X));
        for (int i = 0; i < 3; i++) dir[i] = X[i] / nrm;   // normalized()
    }
    const double *R = a.pose ? a.pose + 12 * item : nullptr;
    const double *sig = a.sigma ? a.sigma + item * a.hyp_max * a.P : nullptr;
#pragma unroll
    for (int h = 0; h < kMaxHyp; h++) {
        if (!(d[h] >= kMinDepth)) continue;
        const double s = !sig ? 0. : (filled >> h & 1u) ? sig[h * a.P + pix] : kDefaultSigma;
        if (a.indices) a.indices[pos] = (int32_t)pix;
        if (a.hyp) a.hyp[pos] = h;
        if (a.index_map) a.index_map[pos] = (int32_t)unit;
        if (a.item) a.item[pos] = (int32_t)item;
        if (a.valid) a.valid[pos] = seen ? 1 : 0;
        if (a.sigma_out) a.sigma_out[pos] = s;
        if (a.points) {
            a.points[2 * pos] = pu;
            a.points[2 * pos + 1] = pv;
        }
        if (a.cloud) {
            const int m = minmax ? 2 : 1;
            for (int e = 0; e < m; e++) {
                const double range = !minmax ? d[h] : e == 0 ? dmax(d[h] - 3 * s, kMinDepth) : d[h] + 3 * s;
                double c[3] = {0., 0., 0.}, w[3];
                if (seen) {
                    for (int i = 0; i < 3; i++) c[i] = dir[i] * range;
                    if (R) {   // Transformation::transform
                        mat_vec(R, c, w);
                        for (int i = 0; i < 3; i++) c[i] = w[i] + R[9 + i];
                    }
                }
                for (int i = 0; i < 3; i++) a.cloud[(pos * m + e) * 3 + i] = c[i];
            }
        }
        pos++;
    }
}

struct PlaneArgs {
    double cam[6];
    Grid g;
    double t[3], z[3];                // the plane's origin and z axis in the camera frame
    double poly[kMaxPolygon][3];      // the polygon in the camera frame
    int k;
    double *depth, *sigma, *cost;     // [P]; cost may be NULL
};

// DepthMap::generatePlane (depth_map.cpp:762-803): one lane per pixel
__global__ __launch_bounds__(kLanes) void depth_generate_plane_kernel(PlaneArgs a)
{
    const int64_t P = (int64_t)a.g.x_max * a.g.y_max, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    if (pix >= P) return;
    const int x = (int)(pix % a.g.x_max), y = (int)(pix / a.g.x_max);
    double vec[3], d = 0., s = 0.;
    if (eucm_reconstruct(a.cam, (double)(x * a.g.scale + a.g.u0), (double)(y * a.g.scale + a.g.v0), vec)) {
        const double zvec = dot3(a.z, vec);
        if (!(zvec < 1e-3)) {
            bool inside = true;
            for (int i = 0; i < a.k && inside; i++) {
                const double *p = a.poly[i], *q = a.poly[i + 1 == a.k ? 0 : i + 1];
                const double nrm[3] = {p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]};
                if (dot3(vec, nrm) < 0) inside = false;
            }
            if (inside) {
                const double alpha = dot3(a.t, a.z) / zvec;
                for (int i = 0; i < 3; i++) vec[i] *= alpha;
                d = sqrt(dot3(vec, vec));
                s = 1.;
            }
        }
    }
    a.depth[pix] = d;
    a.sigma[pix] = s;
    if (a.cost) a.cost[pix] = kDefaultCost;
}

struct CompareArgs {
    Grid g;
    int u_max, v_max;
    int64_t P;
    int nb;
    double sigma_max;
    const double *depth, *sigma;    // [n][P]
    const float *truth;             // [n][v_max][u_max]
    double *partial;                // [n][nb][kCompareSums] of every workgroup
    uint8_t *inliers;               // [n][P] or NULL
};

constexpr int kCompareSums = 6;   // err, err2, dist, then Ngt, Nmax, N: counts of at most 2^28 pixels are exact in FP64

// analyzeError (stereo_test.cpp:32-84) per pixel; the sums and the counts of a workgroup leave through block_sums' fixed tree: no
// atomics (three counters of one item would take 12 same-address atomics per workgroup)
__global__ __launch_bounds__(kLanes) void depth_compare_kernel(CompareArgs a)
{
    const int64_t item = blockIdx.y, pix = (int64_t)blockIdx.x * kLanes + threadIdx.x;
    double sums[kCompareSums] = {0., 0., 0., 0., 0., 0.};
    if (pix < a.P) {
        const int x = (int)(pix % a.g.x_max), y = (int)(pix / a.g.x_max);
        const float truth = a.truth[(item * a.v_max + (y * a.g.scale + a.g.v0)) * a.u_max + (x * a.g.scale + a.g.u0)];
        const float d = (float)a.depth[item * a.P + pix], s = (float)a.sigma[item * a.P + pix];   // toMat, sigmaToMat
        bool inlier = false;
        if (truth != 0.f) sums[3] = 1.;
        if (!(truth == 0.f || d == 0.f) && !(truth != truth || d != d)) {
            sums[4] = 1.;
            sums[2] = (double)truth;
            const float diff = truth - d;
            if (!((double)s > a.sigma_max || fabsf(diff) > s)) {
                inlier = true;
                sums[5] = 1.;
                sums[0] = (double)diff;
                sums[1] = (double)diff * (double)diff;
            }
        }
        if (a.inliers) a.inliers[item * a.P + pix] = inlier ? 255 : 0;
    }
    block_sums<kCompareSums, kLanes>(sums, a.partial + (item * a.nb + blockIdx.x) * kCompareSums);
}

// the partials of an item added in block order: workgroup `item` stages kLanes blocks at a time in LDS with coalesced loads, and
// lane k < kCompareSums walks column k of the stage, eight loads ahead of its chain of dependent adds
__global__ __launch_bounds__(kLanes) void depth_compare_sum_kernel(const double *partial, int nb, double *sums)
{
    __shared__ double stage[kLanes * kCompareSums];
    const double *p = partial + (int64_t)blockIdx.x * nb * kCompareSums;
    double s = 0.;
    for (int first = 0; first < nb; first += kLanes) {
        const int m = min(kLanes, nb - first);
        for (int i = threadIdx.x; i < kCompareSums * m; i += kLanes) stage[i] = p[kCompareSums * (int64_t)first + i];
        __syncthreads();
        if (threadIdx.x < kCompareSums) {
#pragma unroll 8
            for (int b = 0; b < m; b++) s += stage[kCompareSums * b + threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x < kCompareSums) sums[blockIdx.x * kCompareSums + threadIdx.x] = s;
}

}  // namespace vgd
