"""CPU checks of tests/oracle_lm.py, the damped-step reference of tests/test_gpu_lm_steps.py: its arrow (Schur) form equals a
dense solve of the damped normal equations, mu = 0 is the Gauss-Newton step of tests/oracle_gn.py, and the step metric of
the GPU tests (blockwise backward error) is at rounding level for a right step and far above the GPU bar for subtly wrong
ones -- shown here, before any GPU runs."""
import numpy as np
import pytest

from tests import golden_cases as G
from tests import lm_cases as C
from tests import oracle_gn as O
from tests import oracle_lm as L
from tests.oracle_lm import BAR, RHO_MARGIN

MUS = (1e-4, 1.0, 1e2)


def _with_constants(name):
    c = G.case(name)
    if name == "stereo":
        c["const_cameras"], c["const_poses"] = [0], {1: [0, 5]}
    return c


def _ucm_on_bound():
    c = C._ucm_on_bound()
    c["name"] = "ucm_bound"
    x = G.layout(c)[2]
    return c, x


def _dense_step(c, x, mu, held, pose_fixed):
    """(J^T J + mu clamp(diag J^T J)) delta = -J^T r from the stacked oracle rows, the columns of held globals and fixed
    poses removed"""
    r, J = G.oracle_rows(c, x)
    H, g = J.T @ J, J.T @ r
    sy = L.arrow_system(c, x)
    fixed = np.zeros(x.size, dtype=bool)
    fixed[sy["gcols"][held]] = True
    for i in np.nonzero(pose_fixed)[0]:
        fixed[sy["pose_param"][i]:sy["pose_param"][i] + 6] = True
    f = ~fixed
    A = H[np.ix_(f, f)] + mu * np.diag(L.clamp_diag(np.diag(H)[f]))
    d = np.zeros(x.size)
    d[f] = np.linalg.solve(A, -g[f])
    return d


def _scatter(sy, dg, dp, n):
    full = np.zeros(n)
    full[sy["gcols"]] = dg
    full[sy["pose_param"][:, None] + np.arange(6)[None, :]] = dp
    return full


@pytest.mark.parametrize("mu", (0.0,) + MUS)
@pytest.mark.parametrize("name", G.NAMES + ["stereo_constants", "ucm_bound"])
def test_damped_arrow_step_equals_the_dense_solve(name, mu):
    if name == "ucm_bound":
        c, x = _ucm_on_bound()
    else:
        c = _with_constants("stereo") if name == "stereo_constants" else G.case(name)
        x = G.layout(c)[2]
    sy = L.arrow_system(c, x)
    st = L.damped_step(sy, mu)
    d = _dense_step(c, x, mu, st["held"], ~sy["pose_free"])
    a = _scatter(sy, st["dg"], st["dp"], x.size)
    if mu > 0:
        assert np.max(np.abs(a - d)) <= 1e-9 * np.max(np.abs(d))
    # ... and, independent of conditioning (mu = 0 on the Mei case: kappa ~ 1e12), it solves the dense damped system
    r, J = G.oracle_rows(c, x)
    f = (a != 0.0) | (d != 0.0)
    H = J.T @ J
    A = H[np.ix_(f, f)] + mu * np.diag(L.clamp_diag(np.diag(H)[f]))
    g = J[:, f].T @ r
    assert np.linalg.norm(A @ a[f] + g) <= 1e-12 * (np.linalg.norm(A) * np.linalg.norm(a[f]) + np.linalg.norm(g))
    if name == "stereo_constants":
        assert st["held"].sum() == 6 and np.all(st["dg"][:6] == 0) and np.all(st["dp"][[0, 5]] == 0)
    if name == "ucm_bound":      # xi sits on its upper bound; with little damping its step points outwards: held
        s0 = L.damped_step(sy, 1e-16)
        assert s0["held"][0] and s0["dg"][0] == 0.0 and s0["held"].sum() == 1
        d0 = _dense_step(c, x, 1e-16, s0["held"], ~sy["pose_free"])
        assert np.max(np.abs(_scatter(sy, s0["dg"], s0["dp"], x.size) - d0)) <= 1e-9 * np.max(np.abs(d0))
    # the model change 1/2 d^T (mu D d - g) is the decrease of the Gauss-Newton model |r + J d|^2 / 2 along the damped step
    r, J = G.oracle_rows(c, x)
    free = np.ones(x.size, dtype=bool)
    free[sy["gcols"][st["held"]]] = False
    Jd = J[:, free] @ a[free]
    m_dec = -(r @ Jd) - 0.5 * Jd @ Jd
    assert abs(L.model_change(sy, st, mu) - m_dec) <= 1e-9 * abs(m_dec)


@pytest.mark.parametrize("name", G.NAMES)
def test_mu_zero_is_the_gauss_newton_step(name):
    """a wiring check: gauss_newton_step IS damped_step at mu = 0 (the dense-solve test above pins mu = 0 to an independent
    dense solve, tests/test_oracle_gn.py pins it to a dense least-squares solve)"""
    c = G.case(name)
    x = G.layout(c)[2] * (1 + 1e-3)
    sy = L.arrow_system(c, x)
    st = L.damped_step(sy, 0.0)
    g = O.gauss_newton_step(c, x)
    assert np.array_equal(st["dg"], g["dg"]) and np.array_equal(st["dp"], g["dp"])
    assert g["cost"] == sy["cost"] == L.cost(c, x)


def test_soft_l1_rows_are_the_corrected_rows():
    """SoftLOne(a): the gradient of sum 1/2 rho(|r_b|^2) is J^T r weighted by rho'; the arrow system's cost is that sum"""
    c = G.case("stereo")
    x = G.layout(c)[2]
    a = 2.0
    sy = L.arrow_system(c, x, a)
    r, J = G.oracle_rows(c, x)
    N = np.asarray(c["datasets"][0][2]).shape[0]
    s = np.sum(r.reshape(-1, 2 * N) ** 2, axis=1)
    rho, w = L.soft_l1(s, a)
    assert abs(sy["cost"] - 0.5 * np.sum(rho)) <= 1e-13 * sy["cost"]
    g = J.T @ (np.repeat(w, 2 * N) * r)
    assert np.max(np.abs(g[sy["gcols"]] - sy["gg"])) <= 1e-10 * np.max(np.abs(g))
    gp = g[sy["pose_param"][:, None] + np.arange(6)[None, :]]
    assert np.max(np.abs(gp - sy["gp"])) <= 1e-10 * np.max(np.abs(g))


@pytest.mark.parametrize("name", ["mono_eucm", "stereo", "rig"])
def test_step_metric_separates_right_from_subtly_wrong_steps(name):
    """the reference's own step is at rounding level; planted errors are at least 100x above the GPU bar.  (A 1 % error of mu
    changes the system by 1e-2 mu relative to its diagonal: at mu = 1e-4 that is ~1e-7 in this metric, which is why the bar
    sits at 1e-11 and not at 1e-9.)"""
    c = G.case(name)
    x = G.layout(c)[2]
    sy = L.arrow_system(c, x)
    for mu in MUS:
        st = L.damped_step(sy, mu)
        assert L.step_backward_error(sy, mu, st["dg"], st["dp"]) <= 1e-14
        for plant in ({"mu_scale": 1.01}, {"no_pose_damping": 1}, {"drop_w": 3}, {"drop_rhs": 3}):
            q = L.damped_step(sy, mu, plant=plant)
            assert L.step_backward_error(sy, mu, q["dg"], q["dp"]) >= 100 * BAR, (mu, plant)


def test_radius_rule_and_rejections():
    """the chain's radius follows the rule; a far start with radius 1e16 gives an accepted step followed by rejections
    (radius / 2, then / 4), each decision far from min_relative_decrease"""
    c = C.case("mono_eucm_far")
    ch = L.lm_chain(c, G.layout(c)[2], 3, {"initial_trust_region_radius": 1e16})
    assert [it["success"] for it in ch] == [True, False, False]
    rho = ch[0]["rho"]
    r1 = min(1e16 / max(1 - (2 * rho - 1) ** 3, 1 / 3), 1e16)
    assert ch[0]["radius"] == r1 and ch[1]["radius"] == r1 / 2 and ch[2]["radius"] == r1 / 8
    assert [it["n_success"] for it in ch] == [1, 1, 1]
    assert np.array_equal(ch[2]["x"], ch[0]["x"])
    assert all(abs(it["rho"] - 1e-3) > RHO_MARGIN for it in ch)
    assert ch[1]["cost"] == ch[0]["cost"] < L.cost(c, G.layout(c)[2])


def test_rounding_floor_covers_the_rounding_of_x():
    """a right step recovered as fl(x + delta) - x: its backward error stays within the floor backward_error reports (plus
    rounding of the metric itself), also at mu = 100 where the pose steps are small"""
    for name in ("mono_eucm", "stereo"):
        c = G.case(name)
        x = G.layout(c)[2]
        sy = L.arrow_system(c, x)
        for mu in MUS:
            st = L.damped_step(sy, mu)
            x_next = L.apply_step(sy, st["dg"], st["dp"])
            excess, be, floor = L.recovered_step_error(sy, mu, x_next)
            assert excess <= 1e-14 and floor < BAR, (name, mu, be, floor)


@pytest.mark.parametrize("model", ["eucm", "ucm", "mei"])
def test_pose_lm_step_is_the_damped_6x6_solve(model):
    """the per-image reference: its first step solves the damped 6 x 6 system (backward error at rounding level), a planted
    1 % error of mu is far above the bar, and the rule's counts hold (an accepted step moves the pose, a rejected one not)"""
    from visgeom_amd import synthetic as S

    d = S.make_mono(model, 4, 3)
    intr = d["gt_intrinsics"] * (1 + 1e-3)
    for a, R in ((25.0, 1e4), (0.0, 1.0)):
        for b in range(4):
            x0 = d["gt_poses"][b] + 0.02
            out = L.pose_lm(model, intr, d["board"], d["corners"][b], x0, {"max_num_iterations": 1, "initial_trust_region_radius": R,
                                                                            "soft_l1_scale": a})
            t = out["trace"][0]
            assert t["accepted"] and out["iterations"] == 1
            be, floor = L.pose_step_error(model, intr, d["board"], d["corners"][b], x0, out["x"], t["mu"], a)
            assert be - floor <= 1e-14
            r, J = L._pose_rows(model, intr, d["board"], d["corners"][b], x0)
            w = L.soft_l1(r @ r, a)[1]
            A, g = w * (J.T @ J), w * (J.T @ r)
            wrong = x0 - np.linalg.solve(A + 1.01 * t["mu"] * np.diag(L.clamp_diag(np.diag(A))), g)
            assert L.pose_step_error(model, intr, d["board"], d["corners"][b], x0, wrong, t["mu"], a)[0] >= 100 * BAR


# ---- the full system (prior and odometry blocks): tests/test_gpu_lm_coupled_steps.py holds the coupled route to it
FULL = ["stereo_prior", "mono_eucm_seq_prior", "handeye_lam005", "handeye_mid_anchor", "wheeled", "wheeled_const"]


@pytest.mark.parametrize("mu", (0.0,) + MUS)
@pytest.mark.parametrize("name", G.NAMES + ["stereo_constants", "ucm_bound"])
def test_dense_step_equals_the_arrow_step(name, mu):
    """on a case without prior / odometry blocks the full system is the arrow system written out: the same held columns,
    and each step solves the other's system at rounding level (backward error of each in the other's metric)"""
    if name == "ucm_bound":
        c, x = _ucm_on_bound()
    else:
        c = _with_constants("stereo") if name == "stereo_constants" else G.case(name)
        x = G.layout(c)[2]
    sa, sd = L.arrow_system(c, x), L.full_system(c, x)
    assert not L.has_extras(c) and sd["cost"] == sa["cost"]
    assert np.array_equal(sd["pose_free"], sa["pose_free"]) and np.array_equal(sd["gg"], sa["gg"])
    a, d = L.damped_step(sa, mu), L.damped_step(sd, mu)
    assert np.array_equal(a["held"], d["held"])
    for sy in (sa, sd):
        for st in (a, d):
            assert L.step_backward_error(sy, mu, st["dg"], st["dp"]) <= 1e-14, (name, mu, sy.get("dense"), st is d)
    if mu > 0:
        assert abs(L.model_change(sd, d, mu) - L.model_change(sa, a, mu)) <= 1e-9 * abs(L.model_change(sa, a, mu))


def _stacked_rows(c, x):
    """residual vector and dense Jacobian of the whole case at x, in the parameter vector's columns: the grid rows of every
    dataset (image_index honoured) and the prior / odometry rows, each straight from the oracle"""
    from oracle import vgo

    cam_off, tf_off, _, _, _ = G.layout(c)
    pb_off = G.block_offsets(c)
    rs, Js = [], []
    for cam, chain, board, corners, index in (L._dataset(c, d) for d in range(len(c["datasets"]))):
        model = vgo.MODELS[c["cameras"][cam][0]]
        K = vgo.NUM_INTRINSICS[model]
        n, N = corners.shape[0], board.shape[0]
        r, ji, jm = vgo.eval_dataset(model, [s for _, s in chain], board, corners, x, cam_off[cam], [tf_off[t] for t, _ in chain],
                                     [0 if c["transforms"][t][0] else 6 for t, _ in chain], index, want_jac=True, threads=4)
        J = np.zeros((n * 2 * N, x.size))
        for b in range(n):
            rows = slice(b * 2 * N, (b + 1) * 2 * N)
            J[rows, cam_off[cam]:cam_off[cam] + K] = ji[b]
            for l, (t, _) in enumerate(chain):
                o = tf_off[t] + (0 if c["transforms"][t][0] else 6 * index[b])
                J[rows, o:o + 6] += jm[l][b]
        rs.append(r.ravel())
        Js.append(J)

    def add(r, parts):
        J = np.zeros((6, x.size))
        for o, Jp in parts:
            J[:, o:o + Jp.shape[1]] += Jp
        rs.append(r)
        Js.append(J)

    for t, stiff, xp in c.get("priors", ()):
        r, J = vgo.transformation_prior(stiff, xp, x[tf_off[t]:tf_off[t] + 6])
        add(r, [(tf_off[t], J)])
    for t, i, eV, eW, lam, xi1, xi2 in c.get("odometry_priors", ()):
        o1, o2 = tf_off[t] + 6 * i, tf_off[t] + 6 * i + 6
        r, J1, J2 = vgo.OdometryPrior(eV, eW, lam, xi1, xi2).evaluate(x[o1:o1 + 6], x[o2:o2 + 6])
        add(r, [(o1, J1), (o2, J2)])
    for t, i, eV, eW, lam, dq, b in c.get("odometry_costs", ()):
        o1, o2, o3 = tf_off[t] + 6 * i, tf_off[t] + 6 * i + 6, pb_off[b]
        r, J1, J2, J3 = vgo.OdometryCost(eV, eW, lam, dq, c["parameter_blocks"][b][0]).evaluate(x[o1:o1 + 6], x[o2:o2 + 6], x[o3:o3 + 3])
        add(r, [(o1, J1), (o2, J2), (o3, J3)])
    return np.concatenate(rs), np.concatenate(Js)


@pytest.mark.parametrize("name", ["handeye_mid_anchor", "wheeled", "mono_eucm_seq_prior"])
def test_full_system_step_is_the_least_squares_step_of_the_stacked_rows(name):
    """an assembly check independent of full_system: at mu = 0 its step is np.linalg.lstsq of the stacked rows (grid, prior
    and odometry rows, each from the oracle) over the free columns; at mu > 0 the damped step is lstsq of the rows stacked
    over sqrt(mu D).  (The planar wheeled set has a gauge direction, where mu = 0 is singular: there the fitted rows J delta
    are compared.)"""
    c = C.case(name)
    x = G.layout(c)[2] * (1 + 1e-4)
    sy = L.full_system(c, x)
    r, J = _stacked_rows(c, x)
    assert abs(0.5 * r @ r - sy["cost"]) <= 1e-12 * sy["cost"]
    assert abs(L.cost(c, x) - sy["cost"]) <= 1e-12 * sy["cost"]
    for mu in (0.0, 1e-4, 1.0):
        st = L.damped_step(sy, mu)
        d = _scatter(sy, st["dg"], st["dp"], x.size)
        f = np.zeros(x.size, dtype=bool)
        f[sy["gcols"][~st["held"]]] = True
        f[(sy["pose_param"][sy["pose_free"]][:, None] + np.arange(6)[None, :]).ravel()] = True
        assert np.all(d[~f] == 0.0)
        A, b = J[:, f], -r
        if mu:
            Dm = L.clamp_diag(np.sum(A * A, axis=0))
            A, b = np.vstack([A, np.diag(np.sqrt(mu * Dm))]), np.concatenate([b, np.zeros(f.sum())])
        ls = np.linalg.lstsq(A, b, rcond=None)[0]
        if name == "wheeled" and mu == 0.0:
            assert np.linalg.norm(J[:, f] @ (d[f] - ls)) <= 1e-8 * np.linalg.norm(J[:, f] @ ls), name
        else:
            assert np.max(np.abs(d[f] - ls)) <= 1e-8 * np.max(np.abs(ls)), (name, mu, np.max(np.abs(d[f] - ls)) / np.max(np.abs(ls)))


def _planted(name):
    """(case, plants) of the planted-error test"""
    if name == "handeye_prior_mid_anchor":   # anchor 6, frame 3 without an image, a prior on element 0
        c = C._seq_prior(C.case("handeye_mid_anchor"))
        return c, [("image_only_diag", {"image_only_diag": 1}), ("drop_e", {"drop_e": 8}), ("prior_twice", {"prior_twice": 1}),
                   ("keep_frozen", {"keep_frozen": 6})]
    if name == "wheeled":
        # (at mu = 1e-4 the damping of the wheeled poses is too small a part of their system for a wrong one to reach the bar:
        # 7e-10 there; the hand-eye case above covers that plant at every mu)
        return C.case(name), [("image_only_diag", {"image_only_diag": 1}, (1.0, 1e2)), ("drop_e", {"drop_e": 3}),
                              ("drop_wodo", {"drop_wodo": 1})]
    return C.case(name), [("prior_twice", {"prior_twice": 1})]


@pytest.mark.parametrize("name", ["handeye_prior_mid_anchor", "wheeled", "stereo_prior"])
def test_step_metric_separates_right_from_subtly_wrong_full_steps(name):
    """the full system's own step is at rounding level; the errors the coupled route could make land at least 100x above the
    GPU bar: pose damping clamped from the image-only diagonal, one odometry coupling E_i dropped, the OdometryCost
    pose-global coupling dropped, a prior counted twice (added on every rank before the sum), a constant middle element
    whose coupling is kept"""
    c, plants = _planted(name)
    x = G.layout(c)[2]
    sy = L.full_system(c, x)
    for mu in MUS:
        st = L.damped_step(sy, mu)
        assert L.step_backward_error(sy, mu, st["dg"], st["dp"]) <= 1e-14
        for label, plant, *mus in plants:
            if mus and mu not in mus[0]:
                continue
            q = L.damped_step(sy, mu, plant=plant)
            be = L.step_backward_error(sy, mu, q["dg"], q["dp"])
            print("planted %-24s %-16s mu=%-6g backward error %.2e = %.1e x BAR" % (name, label, mu, be, be / BAR))
            assert be >= 100 * BAR, (name, label, mu, be)


@pytest.mark.parametrize("name", FULL)
def test_rounding_floor_covers_the_rounding_of_x_on_the_full_system(name):
    """as test_rounding_floor_covers_the_rounding_of_x, on the cases with prior and odometry blocks"""
    c = C.case(name)
    x = G.layout(c)[2]
    sy = L.full_system(c, x)
    for mu in MUS:
        st = L.damped_step(sy, mu)
        x_next = L.apply_step(sy, st["dg"], st["dp"])
        excess, be, floor = L.recovered_step_error(sy, mu, x_next)
        assert excess <= 1e-14 and floor < BAR, (name, mu, be, floor)


def test_model_change_of_the_full_system_is_the_decrease_of_the_linear_model():
    """1/2 d^T (mu D d - g) is the decrease of |r + J d|^2 / 2 along the damped step, prior and odometry rows included"""
    for name in ("handeye_mid_anchor", "wheeled"):
        c = C.case(name)
        x = G.layout(c)[2]
        sy = L.full_system(c, x)
        r, J = _stacked_rows(c, x)
        for mu in MUS:
            st = L.damped_step(sy, mu)
            Jd = J @ _scatter(sy, st["dg"], st["dp"], x.size)
            m_dec = -(r @ Jd) - 0.5 * Jd @ Jd
            assert abs(L.model_change(sy, st, mu) - m_dec) <= 1e-9 * abs(m_dec), (name, mu)
