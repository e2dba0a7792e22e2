"""The trust-region rule of the pose solves on its own (visgeom_amd/csrc/vg_lm6.hpp, the one definition the photometric host
loop and the sparse odometry kernel share): tests/host/lm6_check.cpp drives vglm6::start / step / accept on small 6-parameter
least-squares problems, compiled by a plain host compiler, and tests/lm6_ref.py solves the same problems in numpy.  One problem
per branch of the rule; the cases state which branch they reach and the test checks that they do.

Tolerance: the C++ solves the damped 6 x 6 system with its own Cholesky, numpy with LAPACK's, on sums that differ in their
last bits (plain loops against BLAS).  The matrices here have a condition below 1e4, so the iterates agree to
1e4 x 2^-53 x a few dozen operations < 1e-12; iteration counts and terminations are decisions far from their thresholds."""
import os
import subprocess

import numpy as np
import pytest

from tests import lm6_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(max_iterations=25, ftol=lm6_ref.FTOL, gtol=lm6_ref.GTOL, ptol=lm6_ref.PTOL, radius0=lm6_ref.RADIUS0,
                max_radius=lm6_ref.MAX_RADIUS, min_radius=lm6_ref.MIN_RADIUS, min_rel_decrease=lm6_ref.MIN_REL_DECREASE,
                diag_min=lm6_ref.DIAG_MIN, diag_max=lm6_ref.DIAG_MAX)
RULE_ORDER = ("ftol", "gtol", "ptol", "radius0", "max_radius", "min_radius", "min_rel_decrease", "diag_min", "diag_max")


def problem(name, A, b, C, x0, wall=False, **rule):
    A, b, C, x0 = (np.asarray(a, float) for a in (A, b, C, x0))
    assert A.shape == C.shape == (len(b), 6) and 8 <= len(b) <= 12 and x0.shape == (6,)
    return dict(name=name, A=A, b=b, C=C, x0=x0, wall=wall, rule=dict(DEFAULTS, **rule))


def normal(p, x):
    """(cost, J^T J, J^T r) of r(x) = A x - b + C (x o x); behind the wall the cost is +inf wherever x differs from x0"""
    r = p["A"] @ x - p["b"] + p["C"] @ (x * x)
    J = p["A"] + 2. * p["C"] * x
    cost = 0.5 * float(r @ r)
    if p["wall"] and not np.array_equal(x, p["x0"]):
        cost = float("inf")
    return cost, J.T @ J, J.T @ r


def problems():
    rs = np.random.RandomState(20)   # the legacy generator: its stream is frozen
    A = rs.randint(-8, 9, (10, 6)) / 4.
    C = rs.randint(-8, 9, (10, 6)) / 16.
    x_true = np.array([0.5, -0.25, 0.75, 0.125, -0.5, 0.25])
    b = A @ x_true + C @ (x_true * x_true) + rs.randint(-8, 9, 10) / 64.
    far = x_true + np.array([1.5, -1.25, 1., -1.5, 1.25, -1.])
    A8 = rs.randint(-8, 9, (8, 6)) / 4.
    b8 = rs.randint(-8, 9, 8) / 4.
    x_opt = np.linalg.lstsq(A8, b8, rcond=None)[0]
    zero, b12 = np.zeros((12, 6)), np.arange(1., 13.) / 8.
    return [
        # function tolerance, after at least one candidate that was refused on the way
        problem("function", A, b, C, far),
        # the cap: the same problem stopped early
        problem("cap0", A, b, C, far, max_iterations=0),
        problem("cap1", A, b, C, far, max_iterations=1),
        problem("cap3", A, b, C, far, max_iterations=3),
        # a linear problem started at its optimum: the gradient is rounding error, tested first, in iteration 1
        problem("gradient", A8, b8, np.zeros((8, 6)), x_opt),
        # a linear problem under a parameter tolerance of 1e-3: the first step is damped by 1 / radius0 = 1e-4 and lands 1e-4 of
        # its length short of the optimum, the second is that remainder: below 1e-3 |x|, tested before the function tolerance
        problem("parameter", A8, b8, np.zeros((8, 6)), x_opt + 1., ptol=1e-3),
        # J = 0 and no floor under the damping diagonal: the matrix is zero, never positive definite, the radius shrinks
        problem("singular", zero, b12, zero, np.zeros(6), diag_min=0.),
        # every candidate costs +inf and the parameter tolerance is off: refused until the radius is below its minimum
        problem("wall", A8, b8, np.zeros((8, 6)), np.zeros(6), wall=True, ptol=0.),
        # a finite cost (residuals of 1e150) under rows of 1e200, one parameter each: J^T J and J^T r overflow, the factor of the
        # diagonal matrix exists (inf > 0) and the step is inf / inf: the candidate is not finite, nothing is evaluated
        problem("candidate", 1e200 * np.eye(6)[np.arange(8) % 6], np.full(8, 1e150), np.zeros((8, 6)), np.zeros(6)),
    ]


def to_text(ps):
    out = [str(len(ps))]
    for p in ps:
        r = p["rule"]
        out.append(" ".join([str(len(p["b"])), str(r["max_iterations"])] + [repr(float(r[k])) for k in RULE_ORDER] + [str(int(p["wall"]))]))
        for a in (p["x0"], p["A"], p["b"], p["C"]):
            out.append(" ".join(repr(float(v)) for v in a.ravel()))
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def solved(tmp_path_factory):
    """(problems, the C++ rows, lm6_ref's results, the points lm6_ref evaluated), computed once"""
    exe = str(tmp_path_factory.mktemp("lm6") / "lm6_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tests", "host", "lm6_check.cpp"), "-o", exe])
    ps = problems()
    r = subprocess.run([exe], input=to_text(ps).encode(), stdout=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stdout.decode()
    rows = [[float(v) for v in line.split()] for line in r.stdout.decode().strip().split("\n")]
    assert len(rows) == len(ps) and all(len(row) == 11 for row in rows)
    got = {p["name"]: dict(x=np.array(row[:6]), iterations=int(row[6]), accepted=int(row[7]), initial_cost=row[8], final_cost=row[9],
                           termination=int(row[10])) for p, row in zip(ps, rows)}
    ref, visited = {}, {}
    for p in ps:
        seen = visited[p["name"]] = []

        def f(x):
            seen.append(x.copy())
            return normal(p, x)

        with np.errstate(over="ignore", invalid="ignore"):   # the candidate case overflows on purpose
            ref[p["name"]] = lm6_ref.solve(f, p["x0"], **p["rule"])
    return {p["name"]: p for p in ps}, got, ref, visited


def test_the_problems_are_well_conditioned(solved):
    """the 1e-12 of the comparison presumes damped matrices of condition <= 1e4"""
    ps, _, _, visited = solved
    for name, p in ps.items():
        if name in ("singular", "candidate"):   # no finite system is solved in either
            continue
        for x in visited[name]:   # the damping only adds to the diagonal: J^T J bounds the condition of what is solved
            JtJ = normal(p, x)[1]
            assert np.linalg.cond(JtJ) <= 1e4, (name, np.linalg.cond(JtJ))


def test_the_rule_equals_the_restatement(solved):
    ps, got, ref, _ = solved
    for name in ps:
        g, (x, rep) = got[name], ref[name]
        print(name, g, rep)
        assert g["iterations"] == rep["iterations"], name
        assert g["termination"] == rep["termination"], name
        for key in ("initial_cost", "final_cost"):
            assert abs(g[key] - rep[key]) <= 1e-12 * abs(rep[key]), (name, key, g[key], rep[key])
        assert np.all(np.abs(g["x"] - x) <= 1e-12 * np.maximum(1., np.abs(x))), (name, g["x"], x)


def test_every_branch_is_reached(solved):
    ps, got, _, _ = solved
    cap = ps["function"]["rule"]["max_iterations"]
    g = got["function"]
    assert g["termination"] == lm6_ref.TERM_FUNCTION and g["iterations"] < cap
    assert g["iterations"] - 1 - g["accepted"] >= 1      # the last iteration stops the solve; of the others one was refused
    assert g["accepted"] >= 2 and g["final_cost"] < 1e-2 * g["initial_cost"]
    for n in (0, 1, 3):                                   # the cap, on a problem that needs more
        c = got["cap%d" % n]
        assert c["iterations"] == n < g["iterations"] and c["termination"] == lm6_ref.TERM_NO_CONVERGENCE
    c = got["cap0"]
    assert np.array_equal(c["x"], ps["cap0"]["x0"]) and c["final_cost"] == c["initial_cost"]
    assert got["cap3"]["final_cost"] < got["cap3"]["initial_cost"]
    g = got["gradient"]
    assert g["termination"] == lm6_ref.TERM_GRADIENT and g["iterations"] == 1 and g["accepted"] == 0
    assert np.array_equal(g["x"], ps["gradient"]["x0"])
    g = got["parameter"]
    assert g["termination"] == lm6_ref.TERM_PARAMETER and g["accepted"] == g["iterations"] - 1 >= 1
    for name in ("singular", "wall", "candidate"):                  # 1e4 / (2 x 4 x ... x 2^k) < 1e-32 first at k = 15: 2^120 = 1.3e36
        g = got[name]
        assert g["termination"] == lm6_ref.TERM_RADIUS and g["iterations"] == 15 and g["accepted"] == 0
        assert np.array_equal(g["x"], ps[name]["x0"]) and g["final_cost"] == g["initial_cost"]
    seen = {g["termination"] for g in got.values()}
    assert seen == {lm6_ref.TERM_FUNCTION, lm6_ref.TERM_GRADIENT, lm6_ref.TERM_PARAMETER, lm6_ref.TERM_NO_CONVERGENCE, lm6_ref.TERM_RADIUS}
