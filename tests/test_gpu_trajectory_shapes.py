"""Trajectory planning on the GPU (vg_trajectory.hpp) at its batch, board and trajectory limits, on the inputs of
tests/trajectory_shapes.py against the long-double restatement (tests/trajectory_ref.py) at the bars of
tests/test_gpu_trajectory.py: cost and terms to 1e-10 max(1, |ref|), info to 1e-10 and cov to 64 eps cond(JtCJ) in the Frobenius
norm, a gradient entry to 64 eps max(1, |cost|) / delta_i; whatever is "the same" is so bit for bit.
A  8 trajectories, four of a single slot: the tables pose0[] and slot0[], the slot -> trajectory search, the order of the finish;
   two invalid poses in the middle of a point; a gradient of 40 parameters (81 points, 648 prepass items)
B  trajectories of 256 poses next to one of 2 in the lanes of one prepass wave; 2040 slots per point
C  boards of 1024, 1023, 4, 66, 66, 65 and 128 corners: every pass count of the corner and the cell loops, 16 KB of LDS
D  130 points of 3 trajectories: several blocks of the prepass and the finish, points astride a block boundary
E  65 535 points in one call, and a small batch on the grown buffers afterwards; the largest gradient batch and one beyond it
F  seven starts minimised in lock-step: 147 points a round
tests/test_trajectory_shapes_cpu.py asserts on the restatement alone that the inputs are what these tests take them for and that
the restatement's float64 / long-double spread, printed beside every comparison, stays below 1e-12 max(1, |ref|).  The worst
|difference| / bar of every case is printed when the module ends."""
import numpy as np
import pytest

from tests import trajectory_shapes as ts

pytestmark = pytest.mark.gpu
BAR = 1e-10
_WORST = {}


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _fro(a):
    return float(np.sqrt((_f64(a) ** 2).sum()))


@pytest.fixture(scope="module")
def planners():
    """planner(setting, steps, board=None): one handle per scene, closed when the module ends"""
    from visgeom_amd.trajectory import TrajectoryPlanner

    made = {}

    def get(setting, steps, board=None):
        key = (setting, tuple(steps), board)
        if key not in made:
            p = ts.plan()
            made[key] = TrajectoryPlanner(p["cam"], p["w"], p["h"], ts.quality_parameters(setting, board), steps)
        return made[key]

    yield get
    for p in made.values():
        p.close()


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    for case in sorted(_WORST):
        print("\ncase %s: worst |difference| / bar %.3g" % (case, _WORST[case]))


def note(case, d, bar):
    _WORST[case] = max(_WORST.get(case, 0.), d / bar)


def compare(case, what, got, ref, r64):
    bar = BAR * max(1., abs(float(ref)))
    d = abs(float(got) - float(ref))
    print("%s %s: %.12g against %.12g, |d| %.3g of %.3g (restatement's spread %.3g)" % (case, what, got, float(ref), d, bar, abs(float(r64) - float(ref))))
    note(case, d, bar)
    assert d <= bar, (case, what)


def compare_point(case, result, ref):
    """cost and the five terms of a valid point against reference()"""
    cost, terms, invalid = result
    assert invalid == 0 and ref["ld"][2] == 0
    compare(case, "cost", cost, ref["ld"][0], ref["f64"][0])
    for k, name in enumerate(ts.TERMS):
        compare(case, name, terms[k], ref["ld"][1][k], ref["f64"][1][k])


def same(a, b):
    """(cost, terms, invalid) of two evaluations, rows or batches: the same bits"""
    return all(np.array_equal(_f64(x).view(np.uint64), _f64(y).view(np.uint64)) for x, y in zip(a[:2], b[:2])) and np.array_equal(a[2], b[2])


def row(batch, k):
    return batch[0][k], batch[1][k], batch[2][k]


# ---- A -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("setting", ts.SETTINGS)
def test_a_eight_trajectories_match_the_restatement(planners, setting):
    p = ts.a_params()
    compare_point("A " + setting, planners(setting, ts.A_STEPS).evaluate(p), ts.reference(setting, ts.A_STEPS, p))


def test_a_invalid_poses_in_the_middle_of_a_point(planners):
    """two invalid poses of trajectory 5: cost and information +inf, the penalties the sums over the 16 valid poses, among them
    the 5 of the trajectories behind; the neighbours in the batch keep the bits they have alone"""
    P = planners("plan", ts.A_STEPS)
    good, bad = ts.a_params(), ts.a_params(invalid=True)
    ref = ts.reference("plan", ts.A_STEPS, bad)
    alone = P.evaluate(good)
    cost, terms, invalid = P.evaluate(bad)
    assert invalid == 2 == ref["ld"][2] and cost == np.inf and terms[0] == np.inf
    for k in range(1, 5):
        compare("A-invalid", ts.TERMS[k], terms[k], ref["ld"][1][k], ref["f64"][1][k])
    batch = P.evaluate(np.stack([good, bad, good]))
    assert batch[2].tolist() == [0, 2, 0]
    assert same(row(batch, 0), alone) and same(row(batch, 2), alone) and same(row(batch, 1), (cost, terms, invalid))


def test_a_gradient_of_forty_parameters(planners):
    """81 points of 8 trajectories in one batch of three launches: the library's own differences bit for bit, and the long-double
    gradient within the rounding of two costs over the step"""
    from visgeom_amd import trajectory

    P = planners("plan", ts.A_STEPS)
    p = ts.a_params()
    pts, delta = trajectory.gradient_points(p)
    assert pts.shape == (81, 40) and ts.blocks_of(81 * 8) == 11
    c, _, inv = P.evaluate(pts)
    assert inv.tolist() == [0] * 81
    before = P.launches
    cost, grad, invalid = P.gradient(p)
    assert P.launches - before == 3 and invalid == 0 and cost == c[0]
    assert np.array_equal(grad, (c[1::2] - c[2::2]) / (2 * delta))
    ref = ts.gradient_reference("plan", ts.A_STEPS, p)
    assert np.array_equal(ref["delta"], delta)
    bound = 64 * ts.EPS * max(1., abs(cost)) / delta
    for i in range(grad.size):
        d = abs(grad[i] - float(ref["ld"][i]))
        print("A g[%d] = %.9g against %.9g: |d| %.3g of %.3g (the float64 restatement's own %.3g)" % (
            i, grad[i], float(ref["ld"][i]), d, bound[i], abs(float(ref["f64"][i]) - float(ref["ld"][i]))))
        note("A gradient", d, bound[i])
    assert (np.abs(grad - _f64(ref["ld"])) <= bound).all()


# ---- B -------------------------------------------------------------------------------------------------------------

def test_b_a_long_trajectory_next_to_a_short_one(planners):
    """[256, 2]: against the restatement; then 33 points whose odd rows perturb the second trajectory: lanes of 256 and of 2 steps
    alternate through one prepass wave (66 items, the last two in a second block), and the unperturbed rows keep their bits"""
    P = planners("plan", ts.B1_STEPS)
    alone = P.evaluate(ts.B1_PARAMS)
    compare_point("B [256, 2]", alone, ts.reference("plan", ts.B1_STEPS, ts.B1_PARAMS))
    batch = ts.b1_batch()
    out = P.evaluate(batch)
    assert out[2].tolist() == [0] * 33
    for k in range(0, 33, 2):
        assert same(row(out, k), alone), k
    assert len(set(out[0][1::2].tolist())) == 16 and alone[0] not in out[0][1::2]   # the others are other points
    ones = [P.evaluate(batch[k]) for k in (1, 31)]
    assert same(row(out, 1), ones[0]) and same(row(out, 31), ones[1])


def test_b_eight_trajectories_of_256_poses(planners):
    p = ts.b8_params()
    compare_point("B [256] * 8", planners("plan", ts.B8_STEPS).evaluate(p), ts.reference("plan", ts.B8_STEPS, p))


# ---- C -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("board", ts.BOARDS, ids=["%dx%d" % b[:2] for b in ts.BOARDS])
def test_c_boards(board):
    """evaluate in both settings, and visual_cov at the three camera poses of the point in the plan's setting, alone and in one
    batch"""
    from visgeom_amd.trajectory import TrajectoryPlanner

    p = ts.plan()
    case = "C %dx%d" % board[:2]
    for setting in ts.SETTINGS:
        P = TrajectoryPlanner(p["cam"], p["w"], p["h"], ts.quality_parameters(setting, board), ts.C_STEPS)
        try:
            compare_point("%s %s" % (case, setting), P.evaluate(ts.C_PARAMS), ts.reference(setting, ts.C_STEPS, ts.C_PARAMS, board))
            if setting != "plan":
                continue
            poses, rows = ts.cov_reference(board)
            cov, info, invalid = P.visual_cov(poses)
            assert invalid.tolist() == [0, 0, 0]
            for k, r in enumerate(rows):
                V, JtJ = r["ld"][0], r["ld"][1]
                e_info, e_cov, bound = _fro(info[k] - JtJ) / _fro(JtJ), _fro(cov[k] - V) / _fro(V), 64 * ts.EPS * r["cond"]
                print("%s pose %d: info %.3g of %.3g (restatement's spread %.3g), cov %.3g of %.3g (spread %.3g), cond(JtCJ) %.3g" % (
                    case, k, e_info, BAR, _fro(r["f64"][1] - JtJ) / _fro(JtJ), e_cov, bound, _fro(r["f64"][0] - V) / _fro(V), r["cond"]))
                note(case + " info", e_info, BAR)
                note(case + " cov", e_cov, bound)
                assert e_info <= BAR and e_cov <= bound
                one = P.visual_cov(poses[k])
                assert np.array_equal(one[0], cov[k]) and np.array_equal(one[1], info[k]) and one[2] == 0
        finally:
            P.close()


# ---- D -------------------------------------------------------------------------------------------------------------

def test_d_a_batch_of_several_blocks(planners):
    """130 points x 3 trajectories: 7 prepass blocks and 3 finish blocks, points 21 and 42 with their items in two blocks.  The
    same points in calls of at most 21, which are one wave for both kernels: the same bits"""
    P = planners("plan", ts.D_STEPS)
    pts = ts.d_points()
    out = P.evaluate(pts)
    assert out[2].tolist() == [0] * 130 and len(set(out[0].tolist())) == 130
    for k in ts.D_CHECKED:
        compare_point("D", row(out, k), ts.reference("plan", ts.D_STEPS, pts[k]))
    for first in range(0, 130, ts.D_CHUNK):
        part = P.evaluate(pts[first:first + ts.D_CHUNK])
        assert same(part, tuple(a[first:first + ts.D_CHUNK] for a in out)), first
    assert same(P.evaluate(pts[129]), row(out, 129))


def test_d_gradients_in_one_call(planners):
    """5 points, 155 evaluations of 3 trajectories: each gradient is the one of its point alone"""
    P = planners("plan", ts.D_STEPS)
    pts = ts.d_points()[[0, 21, 42, 64, 129]]
    before = P.launches
    cost, grad, invalid = P.gradient(pts)
    assert P.launches - before == 3 and invalid.tolist() == [0] * 5
    for k, p in enumerate(pts):
        c, g, i = P.gradient(p)
        assert c == cost[k] and np.array_equal(g, grad[k]) and i == 0 and np.isfinite(g).all()
    assert len(set(cost.tolist())) == 5


# ---- E -------------------------------------------------------------------------------------------------------------

def test_e_the_cap_of_65535_points(planners):
    """grid dimension y of the pose launch at its limit; afterwards the grown buffers serve a small batch"""
    from visgeom_amd import capi

    P = planners("plan", ts.E_STEPS, ts.E_BOARD)
    three = _f64(ts.E_THREE)
    alone = [P.evaluate(p) for p in three]
    for k, p in enumerate(ts.E_THREE):
        compare_point("E", alone[k], ts.reference("plan", ts.E_STEPS, p, ts.E_BOARD))
    assert capi.TRAJECTORY_MAX_POINTS == ts.E_POINTS
    before = P.launches
    cost, terms, invalid = P.evaluate(ts.e_points())
    assert P.launches - before == 3 and cost.shape == (65535,)
    assert not invalid.any()
    for k in range(3):
        assert (cost[k::3].view(np.uint64) == np.float64(alone[k][0]).view(np.uint64)).all(), k
        assert (terms[k::3].view(np.uint64) == alone[k][1].view(np.uint64)).all(), k
    for k, p in enumerate(three):       # a small batch in the grown buffers
        assert same(P.evaluate(p), alone[k])
    assert same(P.evaluate(three), tuple(np.array([a[j] for a in alone]) for j in range(3)))
    # gradients: 11 points each
    grads = [P.gradient(p) for p in three]
    pts = ts.e_points()
    before = P.launches
    with pytest.raises(capi.VisgeomError) as err:
        P.gradient(pts[:5958])
    assert err.value.code == capi.ERR_INVALID_ARGUMENT and P.launches == before
    cost, grad, invalid = P.gradient(pts[:5957])
    assert P.launches - before == 3 and not invalid.any()
    for k in range(3):
        assert grads[k][2] == 0 and np.isfinite(grads[k][1]).all()
        assert (cost[k::3] == grads[k][0]).all() and (grad[k::3].view(np.uint64) == grads[k][1].view(np.uint64)).all(), k


# ---- F -------------------------------------------------------------------------------------------------------------

def test_f_seven_starts_in_lock_step(planners):
    """7 x 21 = 147 points a round while all are live: 3 finish blocks, 5 prepass blocks.  Every start ends where it ends alone"""
    P = planners("plan", ts.plan()["steps"])
    starts = ts.f_starts()
    options = dict(max_iterations=5)
    assert P.evaluate(starts)[2].tolist() == [0] * 7
    before = P.launches
    params, cost, iterations, termination = P.optimize(starts, options=options)
    rounds = P.launches - before
    assert rounds % 3 == 0 and rounds >= 3
    print("F: iterations %s termination %s, %d rounds" % (iterations.tolist(), termination.tolist(), rounds // 3))
    for k, s in enumerate(starts):
        one = P.optimize(s, options=options)
        assert np.array_equal(params[k], one[0]) and cost[k] == one[1] and iterations[k] == one[2] and termination[k] == one[3], k
    c, _, inv = P.evaluate(params)
    assert np.array_equal(c, cost) and inv.tolist() == [0] * 7
    assert (iterations <= 5).all() and (cost <= P.evaluate(starts)[0]).all()
