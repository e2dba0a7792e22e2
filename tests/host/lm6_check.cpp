// Host-only run of the pose solves' trust-region rule (visgeom_amd/csrc/vg_lm6.hpp: vglm6::start / step / accept) on small
// 6-parameter least-squares problems read from stdin, for tests/test_lm6_cpu.py to compare with tests/lm6_ref.py.
//
// Input: the number of problems, then per problem
//   m  max_iter ftol gtol ptol radius0 max_radius min_radius min_rel_decrease dmin dmax  wall
//   x0 (6) | A (m x 6, row-major) | b (m) | C (m x 6, row-major)
// The residuals are r(x) = A x - b + C (x o x), the cost 0.5 r.r; with wall != 0 the cost is +inf wherever x differs from x0.
// Output, one line per problem: x (6) iterations accepted initial_cost final_cost termination.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../visgeom_amd/csrc/vg_lm6.hpp"

namespace {

struct Problem {
    int m = 0, wall = 0;
    double x0[6];
    std::vector<double> A, b, C;

    // the 28 sums [J^T J (21, upper triangle row-major) | J^T r (6) | cost] at x
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

        double G[2][28];   // the sums at the current point and at the candidate
        int cur = 0, accepted = 0;
        vglm6::State S;
        for (int k = 0; k < 6; k++) S.x[k] = P.x0[k];
        P.evaluate(S.x, G[0]);
        vglm6::start(rule, S, G[0][27]);
        const double initial_cost = S.cost;
        while (!S.done) {
            vglm6::Step st;
            vglm6::step(rule, S, G[cur], st);
            double cost_c = 0.;
            if (st.ok) {
                P.evaluate(st.xc, G[1 - cur]);
                cost_c = G[1 - cur][27];
            }
            if (vglm6::accept(rule, S, st, cost_c)) {
                cur = 1 - cur;
                accepted++;
            }
        }
        for (int k = 0; k < 6; k++) std::printf("%.17g ", S.x[k]);
        std::printf("%d %d %.17g %.17g %d\n", S.iterations, accepted, initial_cost, S.cost, S.term);
    }
    return 0;
}
