// vg_lmn.hpp -- the trust-region rule of vg_lm6.hpp for N = K + m parameters of which the last m are eliminated exactly before
// the K x K system is solved (photometric bundle adjustment, vg_dense_ba_tu.hip: K = 6 F pose parameters, m key-frame depths
// with a diagonal block).  The rule is the same one -- D the clamped diagonal of J^T J, mu = 1 / radius, the gain ratio against
// 1/2 (mu sum D dx^2 - g . dx), the three tolerances tested BEFORE the candidate is taken, the radius update and the doubling
// decrease factor -- split where the work splits: the caller reduces the eliminated block on the device and brings
//   dense_step   the reduced system S dx = -rhs (S = H_pp + mu D_p - sum w w^T / e already formed), by the Cholesky of vg_lm6.hpp
//   head_sums    what accept() needs of the K dense parameters, in vg_lm6.hpp's order
//   add_tail     the same five numbers of the m eliminated parameters, summed by the caller in a fixed order
//   accept       the verdict (vglm6::verdict itself, as start is vglm6::start); the caller owns the parameters and moves
//                them when it returns true
// With m = 0 and K = 6 every statement has the shape of vglm6::step / accept: the bits are the same (tests/host/lmn_check.cpp).
//
// Self-contained like vg_lm6.hpp, whose Rule it shares: a plain host compiler takes it.
#pragma once

#include "vg_lm6.hpp"

namespace vglmn {

using vglm6::Rule;

constexpr int kMaxDense = 48;   // 8 frames of 6

struct State {
    double cost, radius, decrease_factor;
    int iterations, term;
    bool done;
};

struct Step {
    double dx[kMaxDense], mu, gdx, ddx, dx2, x2, gmax;
    bool ok;   // false: not positive definite or a candidate that is not finite; nothing to evaluate, accept() shrinks the radius
};

using vglm6::start;

// D of one diagonal entry of J^T J
inline double clamp_diag(const Rule &r, double a) { return a < r.dmin ? r.dmin : (a > r.dmax ? r.dmax : a); }

// S dx = -rhs for the K x K reduced system (row-major, the lower triangle is read): st.dx, st.ok and st.mu
inline void dense_step(int K, const double *S, const double *rhs, double mu, Step &st)
{
    static_assert(kMaxDense >= 6, "the pose block");
    double Lc[kMaxDense][kMaxDense], y[kMaxDense];
    st.mu = mu;
    st.ok = true;
    for (int row = 0; row < K; row++)
        for (int c = 0; c <= row; c++) {
            double v = S[row * K + c];
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
    for (int row = 0; row < K; row++) {
        double v = rhs[row];
        for (int k = 0; k < row; k++) v -= Lc[row][k] * y[k];
        y[row] = v / Lc[row][row];
    }
    for (int row = K - 1; row >= 0; row--) {
        double v = y[row];
        for (int k = row + 1; k < K; k++) v -= Lc[k][row] * st.dx[k];
        st.dx[row] = v / Lc[row][row];
    }
    for (int k = 0; k < K; k++) st.dx[k] = -st.dx[k];
}

// the sums of the K dense parameters at x with gradient g and clamped diagonal D; xc = x + dx
inline void head_sums(int K, const double *x, const double *g, const double *D, Step &st, double *xc)
{
    st.gdx = st.ddx = st.dx2 = st.x2 = st.gmax = 0.;
    for (int k = 0; k < K; k++) {
        xc[k] = x[k] + st.dx[k];
        st.gdx += g[k] * st.dx[k];
        st.ddx += D[k] * st.dx[k] * st.dx[k];
        st.dx2 += st.dx[k] * st.dx[k];
        st.x2 += x[k] * x[k];
        st.gmax = std::fmax(st.gmax, std::fabs(g[k]));
        if (!std::isfinite(xc[k])) st.ok = false;
    }
}

// the eliminated parameters' share: tail = [sum D dx^2, g . dx, |dx|^2, |x|^2, max |g|]; a share that is not finite is a
// candidate that is not finite
inline void add_tail(Step &st, const double *tail)
{
    st.ddx += tail[0];
    st.gdx += tail[1];
    st.dx2 += tail[2];
    st.x2 += tail[3];
    st.gmax = std::fmax(st.gmax, tail[4]);
    if (!(std::isfinite(tail[0]) && std::isfinite(tail[1]) && std::isfinite(tail[2]))) st.ok = false;
}

// One iteration's verdict on the candidate of `st`, whose cost is cost_c (anything when !st.ok).  true: the caller takes the
// candidate (s.cost has moved) and its sums at the candidate become the current ones.  s.done ends the solve.
inline bool accept(const Rule &r, State &s, const Step &st, double cost_c) { return vglm6::verdict(r, s, st, cost_c); }

}  // namespace vglmn
