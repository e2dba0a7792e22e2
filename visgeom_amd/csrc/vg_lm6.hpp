// vg_lm6.hpp -- the trust-region rule of the 6-parameter pose solves, once, for the host loop of the photometric solve
// (vg_photometric_tu.hip) and the kernel of the sparse odometry solve (vg_sparse_odom.hpp): the damped 6 x 6 Cholesky step from
// the 28 sums [J^T J (21, upper triangle row-major) | J^T r (6) | cost] of a pose, and Ceres' acceptance of its candidate (gain
// ratio, the three tolerances tested BEFORE the step is taken, radius update, decrease_factor doubling).  The caller evaluates
// the sums; nothing here knows what the cost is.  (vg_pose_lm.hpp, the calibration's per-image refinement, is a different
// rule: loss weight, function tolerance after acceptance.)
//
// Self-contained: <cmath> and the termination codes of the C ABI, so a plain host compiler takes it (tests/host/lm6_check.cpp).
// Every statement keeps one shape for both users: the device build must not reassociate what the host build computes.
#pragma once

#include <cmath>

#include "../../include/visgeom_amd.h"

#if defined(__HIPCC__)
#define VG_LM6_FN __host__ __device__ __forceinline__
#else
#define VG_LM6_FN inline
#endif

namespace vglm6 {

struct Rule {
    int max_iter;
    double ftol, gtol, ptol, radius0, max_radius, min_radius, min_rel_decrease, dmin, dmax;
};

// Ceres' defaults, which the reference's pose solves leave in place but for the iteration cap
constexpr Rule ceres_defaults(int max_iter) { return Rule{max_iter, 1e-6, 1e-10, 1e-8, 1e4, 1e16, 1e-32, 1e-3, 1e-6, 1e32}; }

struct State {
    double x[6], cost, radius, decrease_factor;
    int iterations, term;
    bool done;
};

struct Step {
    double xc[6], mu, gdx, ddx, dx2, x2, gmax;
    bool ok;   // false: not positive definite or a candidate that is not finite; nothing to evaluate, accept() shrinks the radius
};

// start() and verdict() run on the scalars every state of this rule has (cost, radius, decrease_factor, iterations, term,
// done): S is this State or vg_lmn.hpp's, which owns no parameters; T the matching Step (mu, gdx, ddx, dx2, x2, gmax, ok).

// the state of a solve that starts where the cost is `cost`
template <class S>
VG_LM6_FN void start(const Rule &r, S &s, double cost)
{
    s.cost = cost;
    s.radius = r.radius0;
    s.decrease_factor = 2.;
    s.iterations = 0;
    s.term = VG_TERM_NO_CONVERGENCE;
    s.done = r.max_iter < 1;
}

// (J^T J + mu D) dx = -J^T r, D = clamp(diag(J^T J)), mu = 1 / radius: the candidate s.x + dx and what accept() needs of the step
VG_LM6_FN void step(const Rule &r, const State &s, const double *G, Step &st)
{
    double A[6][6], Lc[6][6], g[6], D[6], y[6], dx[6];
    int q = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++, q++) A[i][j] = A[j][i] = G[q];
    st.mu = 1. / s.radius;
    for (int i = 0; i < 6; i++) {
        g[i] = G[21 + i];
        D[i] = A[i][i] < r.dmin ? r.dmin : (A[i][i] > r.dmax ? r.dmax : A[i][i]);
        A[i][i] += st.mu * D[i];
    }
    st.ok = true;
    for (int row = 0; row < 6; row++)
        for (int c = 0; c <= row; c++) {
            double v = A[row][c];
            for (int k = 0; k < c; k++) v -= Lc[row][k] * Lc[c][k];
            if (row == c) {
                if (!(v > 0.)) {
                    st.ok = false;
                    v = 1.;
                }
                Lc[row][row] = std::sqrt(v);
            } else {
                Lc[row][c] = v / Lc[c][c];
            }
        }
    for (int row = 0; row < 6; row++) {
        double v = g[row];
        for (int k = 0; k < row; k++) v -= Lc[row][k] * y[k];
        y[row] = v / Lc[row][row];
    }
    for (int row = 5; row >= 0; row--) {
        double v = y[row];
        for (int k = row + 1; k < 6; k++) v -= Lc[k][row] * dx[k];
        dx[row] = v / Lc[row][row];
    }
    st.gdx = st.ddx = st.dx2 = st.x2 = st.gmax = 0.;
    for (int k = 0; k < 6; k++) {
        dx[k] = -dx[k];
        st.xc[k] = s.x[k] + dx[k];
        st.gdx += g[k] * dx[k];
        st.ddx += D[k] * dx[k] * dx[k];
        st.dx2 += dx[k] * dx[k];
        st.x2 += s.x[k] * s.x[k];
        st.gmax = std::fmax(st.gmax, std::fabs(g[k]));
        if (!std::isfinite(st.xc[k])) st.ok = false;
    }
}

// One iteration's verdict on the candidate of `st`, whose cost is cost_c (anything when !st.ok).  true: the candidate is taken
// (s.cost has moved; the owner of the parameters moves them) and the caller's sums at the candidate become its current ones.
// s.done ends the solve.  x / xc: the six parameters of a state that owns them and their candidate, moved where the cost moves
// (the device build of accept() keeps its statement order only with the copy at this place).
template <class S, class T>
VG_LM6_FN bool verdict(const Rule &r, S &s, const T &st, double cost_c, double *x = nullptr, const double *xc = nullptr)
{
    s.iterations++;
    double rho = 0.;
    if (st.ok) {
        const double model_change = 0.5 * (st.mu * st.ddx - st.gdx);
        rho = model_change > 0. ? (s.cost - cost_c) / model_change : -1.;
        if (st.gmax <= r.gtol) {
            s.term = VG_TERM_CONVERGENCE_GRADIENT;
            s.done = true;
        } else if (std::sqrt(st.dx2) <= r.ptol * (std::sqrt(st.x2) + r.ptol)) {
            s.term = VG_TERM_CONVERGENCE_PARAMETER;
            s.done = true;
        } else if (model_change > 0. && std::isfinite(cost_c) && std::fabs(s.cost - cost_c) <= r.ftol * s.cost) {
            s.term = VG_TERM_CONVERGENCE_FUNCTION;
            s.done = true;
        }
    }
    if (s.done) return false;
    bool taken = false;
    if (st.ok && std::isfinite(cost_c) && rho > r.min_rel_decrease) {
        if (x)
            for (int k = 0; k < 6; k++) x[k] = xc[k];
        s.cost = cost_c;
        const double t = 2. * rho - 1.;
        s.radius = std::fmin(s.radius / std::fmax(1. - t * t * t, 1. / 3.), r.max_radius);
        s.decrease_factor = 2.;
        taken = true;
    } else {
        s.radius /= s.decrease_factor;
        s.decrease_factor *= 2.;
        if (s.radius < r.min_radius) {
            s.term = VG_TERM_RADIUS_TOO_SMALL;
            s.done = true;
        }
    }
    if (s.iterations >= r.max_iter) s.done = true;
    return taken;
}

// the verdict for the state that owns its six parameters: s.x moves with s.cost
VG_LM6_FN bool accept(const Rule &r, State &s, const Step &st, double cost_c) { return verdict(r, s, st, cost_c, s.x, st.xc); }

}  // namespace vglm6
