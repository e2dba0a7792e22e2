// Host-only run of the N-parameter trust-region rule (visgeom_amd/csrc/vg_lmn.hpp: vglmn::start / dense_step / head_sums /
// add_tail / accept) next to the 6-parameter rule it generalises (vg_lm6.hpp), for tests/test_dense_ba_cpu.py: with no
// eliminated parameters (m = 0) and one frame (K = 6) every step and every verdict must have the bits of vglm6::step / accept.
//
// Input: tests/host/lm6_check.cpp's (the number of problems, then per problem
//   m  max_iter ftol gtol ptol radius0 max_radius min_radius min_rel_decrease dmin dmax  wall
//   x0 (6) | A (m x 6, row-major) | b (m) | C (m x 6, row-major));
// the residuals are r(x) = A x - b + C (x o x), the cost 0.5 r.r; with wall != 0 the cost is +inf wherever x differs from x0.
// Output, one line per problem: iterations accepted termination mismatches -- the last counts the numbers whose bits differed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../visgeom_amd/csrc/vg_lmn.hpp"

namespace {

struct Problem {
    int m = 0, wall = 0;
    double x0[6];
    std::vector<double> A, b, C;

    void evaluate(const double *x, double *G) const
    {
        for (int e = 0; e < 28; e++) G[e] = 0.;
        bool moved = false;
        for (int k = 0; k < 6; k++) moved = moved || x[k] != x0[k];
        for (int i = 0; i < m; i++) {
            double r = -b[i], J[6];
            for (int k = 0; k < 6; k++) {
                r += A[6 * i + k] * x[k] + C[6 * i + k] * (x[k] * x[k]);
                J[k] = A[6 * i + k] + 2. * C[6 * i + k] * x[k];
            }
            int q = 0;
            for (int k = 0; k < 6; k++)
                for (int l = k; l < 6; l++, q++) G[q] += J[k] * J[l];
            for (int k = 0; k < 6; k++) G[21 + k] += J[k] * r;
            G[27] += 0.5 * (r * r);
        }
        if (wall && moved) G[27] = std::numeric_limits<double>::infinity();
    }
};

bool read(double &v) { return std::scanf("%lf", &v) == 1; }

bool read(std::vector<double> &v, int n)
{
    v.resize((size_t)n);
    for (double &e : v)
        if (!read(e)) return false;
    return true;
}

int differ(double a, double b) { return std::memcmp(&a, &b, sizeof a) != 0; }

}  // namespace

int main()
{
    int n = 0;
    if (std::scanf("%d", &n) != 1) return 2;
    for (int p = 0; p < n; p++) {
        Problem P;
        vglm6::Rule rule;
        if (std::scanf("%d %d", &P.m, &rule.max_iter) != 2 || P.m < 1 || P.m > 64) return 2;
        double *tol[9] = {&rule.ftol, &rule.gtol, &rule.ptol, &rule.radius0, &rule.max_radius, &rule.min_radius, &rule.min_rel_decrease, &rule.dmin, &rule.dmax};
        for (double *t : tol)
            if (!read(*t)) return 2;
        if (std::scanf("%d", &P.wall) != 1) return 2;
        for (double &e : P.x0)
            if (!read(e)) return 2;
        if (!read(P.A, 6 * P.m) || !read(P.b, P.m) || !read(P.C, 6 * P.m)) return 2;

        double G[2][28], x[6];
        int cur = 0, accepted = 0, mismatches = 0;
        vglm6::State S6;
        vglmn::State SN;
        for (int k = 0; k < 6; k++) x[k] = S6.x[k] = P.x0[k];
        P.evaluate(x, G[0]);
        vglm6::start(rule, S6, G[0][27]);
        vglmn::start(rule, SN, G[0][27]);
        while (!S6.done && !SN.done) {
            vglm6::Step s6;
            vglm6::step(rule, S6, G[cur], s6);
            // what the library's reduce forms for m = 0: S = H + mu D - 0, rhs = g - 0
            vglmn::Step sn;
            const double mu = 1. / SN.radius, zero_tail[5] = {0., 0., 0., 0., 0.};
            double S[36], g[6], D[6], xc[6];
            int q = 0;
            for (int i = 0; i < 6; i++)
                for (int j = i; j < 6; j++, q++) S[6 * i + j] = S[6 * j + i] = G[cur][q];
            for (int i = 0; i < 6; i++) {
                g[i] = G[cur][21 + i] - 0.;
                D[i] = vglmn::clamp_diag(rule, S[7 * i]);
                S[7 * i] = (S[7 * i] + mu * D[i]) - 0.;
            }
            vglmn::dense_step(6, S, g, mu, sn);
            vglmn::head_sums(6, x, g, D, sn, xc);
            if (sn.ok) vglmn::add_tail(sn, zero_tail);
            mismatches += (s6.ok != sn.ok) + differ(s6.mu, sn.mu);
            if (s6.ok && sn.ok) {
                for (int k = 0; k < 6; k++) mismatches += differ(s6.xc[k], xc[k]);
                mismatches += differ(s6.gdx, sn.gdx) + differ(s6.ddx, sn.ddx) + differ(s6.dx2, sn.dx2) + differ(s6.x2, sn.x2) + differ(s6.gmax, sn.gmax);
            }
            double cost_c = 0.;
            if (s6.ok) {
                P.evaluate(s6.xc, G[1 - cur]);
                cost_c = G[1 - cur][27];
            }
            const bool t6 = vglm6::accept(rule, S6, s6, cost_c), tn = vglmn::accept(rule, SN, sn, cost_c);
            mismatches += (t6 != tn) + differ(S6.cost, SN.cost) + differ(S6.radius, SN.radius) + differ(S6.decrease_factor, SN.decrease_factor) +
                          (S6.iterations != SN.iterations) + (S6.term != SN.term) + (S6.done != SN.done);
            if (tn) {
                for (int k = 0; k < 6; k++) x[k] = xc[k];
                cur = 1 - cur;
                accepted++;
            }
            for (int k = 0; k < 6; k++) mismatches += differ(S6.x[k], x[k]);
        }
        mismatches += (S6.done != SN.done);
        std::printf("%d %d %d %d\n", SN.iterations, accepted, SN.term, mismatches);
    }
    return 0;
}
