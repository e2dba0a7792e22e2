// bfgs_check.cpp -- vg_bfgs.hpp on its own, compiled by a plain host compiler (tests/test_trajectory_cpu.py; also the
// stand-alone target of a -fsanitize=address,undefined build): the Rosenbrock function in `dim` dimensions from
// (-1.2, 1, -1.2, 1, ...), with a wall of +inf outside |x_k| <= 3 so that trials fail on the way.
//   bfgs_check [dim [gtol [max_iterations]]]
// prints: termination iterations failed_trials evaluations cost max|x - 1| max|g|, then x.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../visgeom_amd/csrc/vg_bfgs.hpp"

static double rosenbrock(const double *x, int n, double *g)
{
    for (int k = 0; k < n; k++)
        if (std::fabs(x[k]) > 3.) return HUGE_VAL;   // the wall: g is left unwritten, as a failed evaluation leaves it
    double f = 0.;
    for (int k = 0; k < n; k++) g[k] = 0.;
    for (int k = 0; k + 1 < n; k++) {
        const double a = x[k + 1] - x[k] * x[k], b = 1. - x[k];
        f += 100. * a * a + b * b;
        g[k] += -400. * x[k] * a - 2. * b;
        g[k + 1] += 200. * a;
    }
    return f;
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? std::atoi(argv[1]) : 10;
    if (n < 2 || n > 1000) return 2;
    vgb::Bfgs s;
    s.gtol = argc > 2 ? std::atof(argv[2]) : 1e-8;
    s.ftol = 0.;   // only the gradient test and the cap can end the run
    s.ptol = 0.;
    s.max_iterations = argc > 3 ? std::atoi(argv[3]) : 1000;
    std::vector<double> x0((size_t)n), g((size_t)n);
    for (int k = 0; k < n; k++) x0[k] = k % 2 ? 1. : -1.2;
    s.start(x0.data(), n);
    long evaluations = 0;
    int failed = 0;
    while (!s.done) {
        const bool finite = s.trial_finite();
        const double f = finite ? rosenbrock(s.trial(), n, g.data()) : HUGE_VAL;
        evaluations++;
        failed += !std::isfinite(f);
        s.consume(f, g.data(), finite && std::isfinite(f));
        if (evaluations > 100000) return 3;
    }
    double err = 0.;
    for (int k = 0; k < n; k++) err = std::fmax(err, std::fabs(s.x[k] - 1.));
    std::printf("%d %d %d %ld %.17g %.17g %.17g\n", s.term, s.iterations, failed, evaluations, s.f, err, vgb::Bfgs::max_abs(s.g));
    for (int k = 0; k < n; k++) std::printf("%.17g%c", s.x[k], k + 1 < n ? ' ' : '\n');
    return failed == s.failed_trials ? 0 : 4;
}
