// vg_bfgs.hpp -- BFGS with a strong-Wolfe line search (Nocedal & Wright, algorithms 3.5 and 3.6, cubic interpolation 3.59) in any
// dimension, as a state machine: trial() is the point to evaluate next, consume() takes cost and gradient there, so that many
// minimisations advance in lock-step on one batched evaluation per round.  The rules are those of MiBfgs
// (vg_photometric_mi.hpp), which stays the six-parameter solver of the MI pose estimation: the inverse Hessian starts at the
// identity, the first step length is min(1, 1 / max|g|) and 1 afterwards, a search spends at most 20 evaluations, the update is
// skipped when s^T y <= 0.  A trial whose cost or gradient is not finite is a failed trial -- "too far" -- and the search
// shrinks towards the last valid point.  Host only, no HIP.
#pragma once

#include <cmath>
#include <vector>

namespace vgb {

// what vg_termination names (include/visgeom_amd.h); restated so that this header stands alone
enum : int { kTermFunction = 0, kTermGradient = 1, kTermParameter = 2, kTermNoConvergence = 3, kTermFailure = 5 };

struct Bfgs {
    static constexpr double kC1 = 1e-4, kC2 = 0.9;
    static constexpr int kMaxSearchEvals = 20;
    // a tolerance of zero switches its test off
    double ftol = 1e-6, gtol = 1e-10, ptol = 1e-8;
    int max_iterations = 1000;
    int n = 0;
    std::vector<double> x, g, H, d, xt;
    double f = 0.;
    double phi0 = 0., dphi0 = 0.;                        // the search: phi(alpha) = f(x + alpha d)
    double alpha = 0., a_prev = 0., phi_prev = 0., dphi_prev = 0.;
    double a_lo = 0., phi_lo = 0., dphi_lo = 0., a_hi = 0., phi_hi = 0., dphi_hi = 0.;
    int evals = 0, iterations = 0, failed_trials = 0, term = kTermNoConvergence;
    bool zoom = false, done = false, started = false;
    double initial_cost = 0.;

    static double max_abs(const std::vector<double> &v)
    {
        double m = 0.;
        for (double e : v) m = std::fmax(m, std::fabs(e));
        return m;
    }
    void identity()
    {
        for (int k = 0; k < n * n; k++) H[(size_t)k] = k % (n + 1) == 0 ? 1. : 0.;
    }
    void start(const double *x0, int dim)
    {
        n = dim;
        x.assign(x0, x0 + n);
        xt = x;
        g.assign((size_t)n, 0.);
        d.assign((size_t)n, 0.);
        H.assign((size_t)n * n, 0.);
        identity();
        done = started = zoom = false;
        iterations = evals = failed_trials = 0;
        term = kTermNoConvergence;
    }
    const double *trial() const { return xt.data(); }
    bool trial_finite() const
    {
        for (double e : xt)
            if (!std::isfinite(e)) return false;
        return true;
    }
    void finish(int t)
    {
        term = t;
        done = true;
    }
    void set_trial(double a)
    {
        alpha = a;
        for (int k = 0; k < n; k++) xt[k] = x[k] + a * d[k];
    }
    // a new search from x along -H g (steepest descent when that is no descent direction)
    void begin_search()
    {
        if (iterations >= max_iterations) return finish(kTermNoConvergence);
        double gd = 0.;
        for (int r = 0; r < n; r++) {
            d[r] = 0.;
            for (int k = 0; k < n; k++) d[r] -= H[(size_t)n * r + k] * g[k];
            gd += g[r] * d[r];
        }
        if (!(gd < 0.)) {
            identity();
            gd = 0.;
            for (int k = 0; k < n; k++) {
                d[k] = -g[k];
                gd -= g[k] * g[k];
            }
        }
        phi0 = f;
        dphi0 = gd;
        a_prev = 0.;
        phi_prev = phi0;
        dphi_prev = dphi0;
        evals = 0;
        zoom = false;
        set_trial(iterations == 0 ? std::fmin(1., 1. / max_abs(g)) : 1.);
    }
    // the minimiser of the cubic through (a, fa, da) and (b, fb, db), kept a tenth of the interval away from both ends; the
    // midpoint when the cubic has none there or a value is not finite
    static double interpolate(double a, double fa, double da, double b, double fb, double db)
    {
        const double mid = 0.5 * (a + b), lo = std::fmin(a, b), hi = std::fmax(a, b), w = hi - lo;
        const double d1 = da + db - 3. * (fa - fb) / (a - b);
        const double rad = d1 * d1 - da * db;
        if (!(rad >= 0.) || !std::isfinite(rad)) return mid;
        const double d2 = (b > a ? 1. : -1.) * std::sqrt(rad);
        const double t = b - (b - a) * (db + d2 - d1) / (db - da + 2. * d2);
        if (!std::isfinite(t) || t < lo + 0.1 * w || t > hi - 0.1 * w) return mid;
        return t;
    }
    void zoom_trial()
    {
        zoom = true;
        if (evals >= kMaxSearchEvals) return finish(kTermFailure);
        set_trial(interpolate(a_lo, phi_lo, dphi_lo, a_hi, phi_hi, dphi_hi));
    }
    // the step to x + alpha d is taken: the update, the tests, the next search
    void accept(double fn, const double *gn)
    {
        std::vector<double> s((size_t)n), y((size_t)n);
        double sy = 0., s2 = 0., x2 = 0.;
        for (int k = 0; k < n; k++) {
            s[k] = xt[k] - x[k];
            y[k] = gn[k] - g[k];
            sy += s[k] * y[k];
            s2 += s[k] * s[k];
            x2 += x[k] * x[k];
        }
        if (sy > 0.) {   // H = (I - rho s y^T) H (I - rho y s^T) + rho s s^T
            const double rho = 1. / sy;
            std::vector<double> Hy((size_t)n);
            double yHy = 0.;
            for (int r = 0; r < n; r++) {
                Hy[r] = 0.;
                for (int k = 0; k < n; k++) Hy[r] += H[(size_t)n * r + k] * y[k];
            }
            for (int k = 0; k < n; k++) yHy += y[k] * Hy[k];
            for (int r = 0; r < n; r++)
                for (int q = 0; q < n; q++)
                    H[(size_t)n * r + q] += -rho * (s[r] * Hy[q] + Hy[r] * s[q]) + (rho * rho * yHy + rho) * s[r] * s[q];
        }
        const double f_old = f;
        x = xt;
        g.assign(gn, gn + n);
        f = fn;
        iterations++;
        if (max_abs(g) <= gtol) return finish(kTermGradient);
        if (ftol > 0. && std::fabs(f - f_old) <= ftol * std::fabs(f_old)) return finish(kTermFunction);
        if (ptol > 0. && std::sqrt(s2) <= ptol * (std::sqrt(x2) + ptol)) return finish(kTermParameter);
        begin_search();
    }
    // cost and gradient at trial(); ok = false: nothing usable was evaluated there (the trial point, its cost or its gradient is
    // not finite)
    void consume(double ft, const double *gt, bool ok)
    {
        ok = ok && std::isfinite(ft);
        for (int k = 0; ok && k < n; k++) ok = std::isfinite(gt[k]);
        if (!started) {
            started = true;
            if (!ok) {   // the start itself cannot be evaluated
                f = initial_cost = HUGE_VAL;
                return finish(kTermFailure);
            }
            f = initial_cost = ft;
            g.assign(gt, gt + n);
            if (max_abs(g) <= gtol) return finish(kTermGradient);
            return begin_search();
        }
        evals++;
        double dphi = 0.;
        for (int k = 0; ok && k < n; k++) dphi += gt[k] * d[k];
        if (!ok) failed_trials++;
        const double phi = ok ? ft : HUGE_VAL;   // a failed trial: too far
        const bool armijo = phi <= phi0 + kC1 * alpha * dphi0, wolfe = std::fabs(dphi) <= -kC2 * dphi0;
        if (!zoom) {
            if (!armijo || (evals > 1 && phi >= phi_prev)) {
                a_lo = a_prev, phi_lo = phi_prev, dphi_lo = dphi_prev;
                a_hi = alpha, phi_hi = phi, dphi_hi = dphi;
                return zoom_trial();
            }
            if (wolfe) return accept(ft, gt);
            if (dphi >= 0.) {
                a_lo = alpha, phi_lo = phi, dphi_lo = dphi;
                a_hi = a_prev, phi_hi = phi_prev, dphi_hi = dphi_prev;
                return zoom_trial();
            }
            if (evals >= kMaxSearchEvals) return finish(kTermFailure);
            a_prev = alpha, phi_prev = phi, dphi_prev = dphi;
            return set_trial(2. * alpha);
        }
        if (!armijo || phi >= phi_lo) {
            a_hi = alpha, phi_hi = phi, dphi_hi = dphi;
        } else {
            if (wolfe) return accept(ft, gt);
            if (dphi * (a_hi - a_lo) >= 0.) a_hi = a_lo, phi_hi = phi_lo, dphi_hi = dphi_lo;
            a_lo = alpha, phi_lo = phi, dphi_lo = dphi;
        }
        zoom_trial();
    }
};

}  // namespace vgb
