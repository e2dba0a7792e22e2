// vg_corners_graph.hpp -- the host stages of the corner detector (src/calibration/corner_detector.cpp): the circle rasteriser
// (CurveRasterizer, include/utils/curve_rasterizer.h) that builds the kernels' circle tables, the graph construction
// (constructGraph .cpp:612-780), the chain extraction and pattern selection (.cpp:850-1077) and initPoin (.cpp:1261-1300).
// One image per call; the caller runs images side by side on host threads.  Host only, no device code.
#pragma once

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <queue>
#include <stdexcept>
#include <unordered_map>
#include <utility>
#include <vector>

#include "vg_corners.hpp"

namespace vgcorner {

inline int sign(double x) { return 2 * int(x > 0) - 1; }   // std.h:74: sign(0) = -1

// getCircle (.cpp:1079-1108) around (0, 0): radius 1 is the fixed 8-neighbourhood, larger radii the CurveRasterizer walk
// (curve_rasterizer.h:170-259) of Polynomial2::Circle from (r, 0) towards (0, r) until it is back next to its start
inline std::vector<std::array<int, 2>> raster_circle(int radius)
{
    std::vector<std::array<int, 2>> res;
    if (radius == 1) {
        const int du[8] = {1, 1, 0, -1, -1, -1, 0, 1}, dv[8] = {0, 1, 1, 1, 0, -1, -1, -1};
        for (int i = 0; i < 8; i++) res.push_back({du[i], dv[i]});
        return res;
    }
    // Polynomial2::Circle(0, 0, r): u^2 + v^2 - r^2
    const double k1 = -(double)radius * radius;
    auto surf = [&](int u, int v) { return (1. * u + 0. * v + 0.) * u + (1. * v + 0.) * v + k1; };
    auto gradu = [](int u, int v) { return 2. * u + 0. * v + 0.; };
    auto gradv = [](int u, int v) { return 0. * u + 2. * v + 0.; };
    int u = radius, v = 0;
    double fu = gradu(u, v), fv = gradv(u, v), delta = surf(u, v);
    const int eps = fu * (radius - v) - fv * (0 - u) > 0 ? 1 : -1;
    auto moveU = [&](int du) {
        if (du == 0) return;
        u += du;
        const double fu2 = gradu(u, v);
        delta += 0.5 * du * (fu + fu2);
        fu = fu2;
        fv = gradv(u, v);
    };
    auto moveV = [&](int dv) {
        if (dv == 0) return;
        v += dv;
        const double fv2 = gradv(u, v);
        delta += 0.5 * dv * (fv + fv2);
        fv = fv2;
        fu = gradu(u, v);
    };
    for (int i = 0;; i++) {
        res.push_back({u, v});
        if (i > 5 && std::abs(u - radius) <= 1 && std::abs(v) <= 1) break;
        if (res.size() > 1000) throw std::logic_error("circle rasteriser did not close");
        if (std::abs(fu) > std::abs(fv)) {
            moveV(eps * sign(fu));
            moveU((int)-std::round(delta / fu));
        } else {
            moveU(-eps * sign(fv));
            moveV((int)-std::round(delta / fv));
        }
    }
    return res;
}

inline vg::CircleTable circle_table()
{
    vg::CircleTable t{};
    int pos = 0;
    for (int r = 1; r <= vg::kCircMaxR; r++) {
        const auto c = raster_circle(r);
        if ((int)c.size() > vg::kCircMaxLen || pos + (int)c.size() > vg::kCircTableLen) throw std::logic_error("circle table overflow");
        t.start[r] = pos;
        t.len[r] = (int)c.size();
        for (auto &p : c) {
            t.du[pos] = (int8_t)p[0];
            t.dv[pos] = (int8_t)p[1];
            pos++;
        }
    }
    return t;
}

// one image's inputs to the graph stages: the maps that stay on the host side and the accepted candidates
struct ImageView {
    int W = 0, H = 0, init_radius = 0;
    const uint8_t *src2 = nullptr;
    const float *gradx = nullptr, *grady = nullptr;
    int n_hyp = 0;
    const int *trans = nullptr;          // [n_hyp][9] (vg_corner_transitions_kernel)
    const double *grad_thresh = nullptr; // [n_hyp]
};

struct Pt {
    int u, v;
};

// bilinear<double> (include/ocv.h:63-84) on the u8 map, with its border rule
inline double bilinear(const ImageView &im, double x, double y)
{
    int u = (int)x, v = (int)y;
    const double dx = x - u, dy = y - v, dx2 = 1 - dx;
    bool fail = false;
    if ((fail |= u < 0)) u = 0;
    else if ((fail |= u > im.W - 2)) u = im.W - 1;
    if ((fail |= v < 0)) v = 0;
    else if ((fail |= v > im.H - 2)) v = im.H - 1;
    auto at = [&](int vv, int uu) { return (double)im.src2[(size_t)vv * im.W + uu]; };
    if (fail) return at(v, u);
    const double i00 = at(v, u), i01 = at(v, u + 1), i10 = at(v + 1, u), i11 = at(v + 1, u + 1);
    return (i11 * dx + i10 * dx2) * dy + (i01 * dx + i00 * dx2) * (1 - dy);
}

inline int inorm(int x, int y) { return (int)std::sqrt((double)(x * x + y * y)); }   // Vector2i::norm() is an int (truncated)

class Graph {
public:
    Graph(const ImageView &im, int Nx, int Ny) : im_(im), Nx_(Nx), Ny_(Ny) {}

    // constructGraph (.cpp:612-780).  The hypotheses leave _hypHeap in std::pop_heap order of -(u + v) (.cpp:597, :620-623): the
    // same heap calls on the same sequence as the reference, so equal sums come out in the reference's order.
    void construct()
    {
        std::vector<std::pair<double, int>> heap;
        for (int h = 0; h < im_.n_hyp; h++) heap.emplace_back(-(double)im_.trans[9 * h] - im_.trans[9 * h + 1], h);
        auto comp = [](const std::pair<double, int> &a, const std::pair<double, int> &b) { return a.first < b.first; };
        std::make_heap(heap.begin(), heap.end(), comp);
        struct TimePoint {
            int t, idx, u, v;
        };
        std::queue<TimePoint> fringe;
        idxMap_.assign((size_t)im_.W * im_.H, -1);
        for (int i = 0; !heap.empty(); i++) {
            std::pop_heap(heap.begin(), heap.end(), comp);
            const int h = heap.back().second;
            heap.pop_back();
            const int *tr = im_.trans + 9 * h;
            gradThresh_.push_back(im_.grad_thresh[h]);
            if (tr[2] == 4)
                for (int q = 0; q < 4; q++) fringe.push({0, i, tr[3 + q] & 0xFFFF, tr[3 + q] >> 16});
            arcVec_.emplace_back();
            ptVec_.push_back({tr[0], tr[1]});
            hypOf_.push_back(h);
        }
        const int duVec[8] = {-1, 0, 1, 1, 1, 0, -1, -1};
        const int dvVec[8] = {-1, -1, -1, 0, 1, 1, 1, 0};
        const int SEARCH_REACH = 140;
        const int W = im_.W, H = im_.H, R = im_.init_radius;
        while (!fringe.empty() && fringe.front().t < SEARCH_REACH) {
            const TimePoint e = fringe.front();
            fringe.pop();
            int &slot = idxMap_[(size_t)e.v * W + e.u];
            if (slot != -1) continue;
            slot = e.idx;
            bool connected = false;
            for (int i = 0; i < 8; i++) {
                const int u2 = e.u + duVec[i], v2 = e.v + dvVec[i];
                if (u2 < 0 || u2 >= W || v2 < 0 || v2 >= H) continue;
                const int idx2 = idxMap_[(size_t)v2 * W + u2];
                if (idx2 == -1 || idx2 == e.idx) continue;
                connected = true;
                auto &arcs = arcVec_[e.idx];
                if (std::find(arcs.begin(), arcs.end(), idx2) != arcs.end()) continue;
                // the arc sign (.cpp:672-693): which side of the arc is darker in the sigma_2 image
                const double ax = ptVec_[idx2].u - ptVec_[e.idx].u, ay = ptVec_[idx2].v - ptVec_[e.idx].v;
                const double an = std::sqrt(ax * ax + ay * ay);
                const double nx = ax / an, ny = ay / an;
                int signAcc = 0;
                for (int base = 1; base <= R; base++) {
                    const double sx = nx * base, sy = ny * base;
                    for (int lambda = 1; lambda < 5; lambda++) {
                        const double mx = ptVec_[e.idx].u + ax * (double(lambda) / 5), my = ptVec_[e.idx].v + ay * (double(lambda) / 5);
                        const double sample1 = bilinear(im_, mx - sy, my + sx);
                        const double sample2 = bilinear(im_, mx + sy, my - sx);
                        signAcc += sign(sample1 - sample2);
                    }
                }
                signAcc = sign(signAcc);
                arcVec_[e.idx].push_back(idx2);
                arcVec_[idx2].push_back(e.idx);
                arcSign_[key(e.idx, idx2)] = signAcc;
                arcSign_[key(idx2, e.idx)] = -signAcc;
            }
            if (connected) continue;
            for (int i = 0; i < 8; i++) {   // proliferate (.cpp:705-745)
                const int u2 = e.u + duVec[i], v2 = e.v + dvVec[i];
                if (u2 < 0 || u2 >= W || v2 < 0 || v2 >= H) continue;
                if (idxMap_[(size_t)v2 * W + u2] != -1) continue;
                const double x1 = u2 - ptVec_[e.idx].u, y1 = v2 - ptVec_[e.idx].v;
                const double t = std::sqrt(x1 * x1 + y1 * y1);
                const double xg = im_.gradx[(size_t)v2 * W + u2], yg = im_.grady[(size_t)v2 * W + u2];
                const double gradProj = std::abs(xg * y1 - yg * x1);
                if (t > 0 && gradProj / t < gradThresh_[e.idx]) continue;
                if (t > 0) {
                    const double c = x1 * xg + y1 * yg, s = x1 * yg - y1 * xg;
                    const double angle = std::abs(std::atan2(s, c));
                    const double thresh = std::min(M_PI / 5, t / 150. + 1 / t);
                    if (angle < M_PI / 2 - thresh || angle > M_PI / 2 + thresh) continue;
                }
                fringe.push({e.t + 1, e.idx, u2, v2});
            }
        }
    }

    // selectPattern (.cpp:957-1031): indices into ptVec, row by row (Nx per row), or empty
    std::vector<int> select_pattern()
    {
        std::vector<int> res;
        for (int idx0 = 0; idx0 < (int)ptVec_.size(); idx0++) {
            if (arcVec_[idx0].size() < 2) continue;
            std::vector<int> chainY, chainX;
            for (int n : arcVec_[idx0]) {
                std::vector<int> chain = extract_sequence(idx0, n);
                if ((int)chain.size() >= Ny_) {
                    chain.resize(Ny_);
                    chainX = best_orthogonal_chain(idx0, n, -1, Nx_);
                    if ((int)chainX.size() == Nx_) {
                        chainY = chain;
                        break;
                    }
                }
            }
            if (chainY.empty() || chainX.empty()) continue;
            res = chainX;
            for (size_t i = 1; i < chainY.size(); i++) {
                std::vector<int> bestChain = best_orthogonal_chain(chainY[i], chainY[i - 1], 1, Nx_);
                if ((int)bestChain.size() >= Nx_) res.insert(res.end(), bestChain.begin(), bestChain.begin() + Nx_);
                else break;
            }
            if ((int)res.size() == Nx_ * Ny_ && verify(res)) return res;
            res.clear();
        }
        return res;
    }

    Pt point(int idx) const { return ptVec_[idx]; }
    int hyp_of(int idx) const { return hypOf_[idx]; }

private:
    static int64_t key(int a, int b) { return ((int64_t)a << 32) | (uint32_t)b; }
    int arc_sign(int a, int b) const
    {
        auto it = arcSign_.find(key(a, b));
        return it == arcSign_.end() ? 0 : it->second;   // std::map::operator[] would insert 0 (never reached for an arc)
    }
    double compare(Pt d1, Pt d2) const   // compareVectors (.cpp:838-848), integer norms
    {
        return inorm(d1.u - d2.u, d1.v - d2.v) / double(inorm(d1.u, d1.v));
    }
    Pt diff(int a, int b) const { return {ptVec_[a].u - ptVec_[b].u, ptVec_[a].v - ptVec_[b].v}; }

    // extractSequence (.cpp:850-914).  The walk is bounded by the number of points plus one (the reference has no bound; a
    // walk that long would have to revisit points, where the reference loops forever).
    std::vector<int> extract_sequence(int idx0, int idx1) const
    {
        std::vector<int> chain;
        const Pt d1 = diff(idx1, idx0);
        int idx2 = -1;
        double bestNormDiff = 1;
        for (int n2 : arcVec_[idx1]) {
            const double normDiff = compare(d1, diff(n2, idx1));
            if (arc_sign(idx1, n2) == arc_sign(idx0, idx1)) continue;
            if (normDiff < bestNormDiff) {
                bestNormDiff = normDiff;
                idx2 = n2;
            }
        }
        if (idx2 == -1) return chain;
        chain = {idx0, idx1, idx2};
        const size_t limit = ptVec_.size() + 1;
        while (chain.size() <= limit) {
            const int i1 = chain[chain.size() - 1], i0 = chain[chain.size() - 2];
            const Pt d0 = diff(i1, i0);
            int best = -1;
            double bnd = 1;
            for (int n2 : arcVec_[i1]) {
                if (n2 == i0) continue;
                if (arc_sign(i1, n2) == arc_sign(i0, i1)) continue;
                const double normDiff = compare(d0, diff(n2, i1));
                if (normDiff < bnd) {
                    bnd = normDiff;
                    best = n2;
                }
            }
            if (best == -1) break;
            chain.push_back(best);
        }
        return chain;
    }

    // selectBestOrthogonalChain (.cpp:922-954)
    std::vector<int> best_orthogonal_chain(int idx0, int idx1, int EPS, int LENGTH) const
    {
        double bestCost = 0.3;
        std::vector<int> bestChain;
        const int baseSign = arc_sign(idx0, idx1);
        for (int nx : arcVec_[idx0]) {
            if (nx == idx1) continue;
            if (arc_sign(idx0, nx) == baseSign) continue;
            const Pt d1 = diff(idx1, idx0), d2 = diff(nx, idx0);
            std::vector<int> chain = extract_sequence(idx0, nx);
            const double cost = EPS * (d1.u * d2.v - d1.v * d2.u) / double(inorm(d1.u, d1.v) * inorm(d2.u, d2.v));
            if (cost < bestCost) continue;
            if ((int)chain.size() >= LENGTH) {
                bestCost = cost;
                bestChain = chain;
            }
        }
        if ((int)bestChain.size() > LENGTH) bestChain.resize(LENGTH);
        return bestChain;
    }

    // verifyDetection (.cpp:1033-1050)
    bool verify(const std::vector<int> &idxVec) const
    {
        if ((int)idxVec.size() != Nx_ * Ny_) return false;
        for (int i = 1; i < Nx_; i++) {
            const auto &arcs = arcVec_[idxVec[i]];
            if (std::find(arcs.begin(), arcs.end(), idxVec[Nx_ + i]) == arcs.end()) return false;
            const std::vector<int> chain = extract_sequence(idxVec[i], idxVec[Nx_ + i]);
            if ((int)chain.size() < Ny_) return false;
            for (int j = 2; j < Ny_; j++)
                if (chain[j] != idxVec[j * Nx_ + i]) return false;
        }
        return true;
    }

    const ImageView &im_;
    const int Nx_, Ny_;
    std::vector<int> idxMap_;
    std::vector<std::vector<int>> arcVec_;
    std::vector<double> gradThresh_;
    std::unordered_map<int64_t, int> arcSign_;
    std::vector<Pt> ptVec_;
    std::vector<int> hypOf_;
};

// initPoin (.cpp:1261-1300) from a candidate's transitions [max1, max2, min1, min2] = A, C, B, D: the intersection of AC and BD
// (Eigen's 2 x 2 inverse) and the two line angles; false when there are no transitions or the lines are parallel (the
// reference reads past an empty vector or divides by zero there; the corner is then left where the detector put it)
inline bool init_point(const int *tr, double *data)
{
    if (tr[2] != 4) return false;
    const double A0 = tr[3] & 0xFFFF, A1 = tr[3] >> 16, C0 = tr[4] & 0xFFFF, C1 = tr[4] >> 16;
    const double B0 = tr[5] & 0xFFFF, B1 = tr[5] >> 16, D0 = tr[6] & 0xFFFF, D1 = tr[6] >> 16;
    const double m00 = A1 - C1, m01 = C0 - A0, m10 = B1 - D1, m11 = D0 - B0;
    const double b0 = A1 * m01 + A0 * m00, b1 = B1 * m11 + B0 * m10;
    const double det = m00 * m11 - m10 * m01;
    if (det == 0.) return false;
    const double invdet = 1. / det;
    const double i00 = m11 * invdet, i10 = -m10 * invdet, i01 = -m01 * invdet, i11 = m00 * invdet;
    data[0] = i00 * b0 + i01 * b1;
    data[1] = i10 * b0 + i11 * b1;
    data[2] = std::atan2(A1 - C1, A0 - C0);
    data[3] = std::atan2(B1 - D1, B0 - D0);
    data[4] = 0;
    return std::isfinite(data[0]) && std::isfinite(data[1]);
}

// improveCorners' radii (.cpp:164-175), including its `i > _Nx` test
inline void refine_radii(const std::vector<double> &pts, int Nx, std::vector<double> &rad)
{
    const int n = (int)pts.size() / 2;
    rad.resize(n);
    auto dist = [&](int a, int b) {   // Vector2d::norm()
        const double dx = pts[2 * a] - pts[2 * b], dy = pts[2 * a + 1] - pts[2 * b + 1];
        return std::sqrt(dx * dx + dy * dy);
    };
    for (int i = 0; i < n; i++) {
        double radMax = 7;
        if (i > Nx) radMax = std::min(radMax, dist(i, i - Nx) * 0.7);
        else radMax = std::min(radMax, dist(i, i + Nx) * 0.7);
        if (i > 0) radMax = std::min(radMax, dist(i, i - 1) * 0.7);
        else radMax = std::min(radMax, dist(i, i + 1) * 0.7);
        rad[i] = radMax;
    }
}

}  // namespace vgcorner
