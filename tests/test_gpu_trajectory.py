"""Trajectory planning on the GPU (section 17) against the numpy restatement (tests/trajectory_ref.py) on the scene of
tests/golden/trajectory_plan.json: 2 trajectories of 4 and 7 poses in front of an 8 x 5 board (40 corners, a partial wave).
The reference values are the restatement's in long double; its float64 / long-double spread -- the restatement's own error -- is
printed next to every comparison."""
import copy
import os

import numpy as np
import pytest

from tests import trajectory_ref as tr

pytestmark = pytest.mark.gpu
PLAN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trajectory_plan.json")
EPS = 2. ** -52
LD = np.longdouble
PROBE = [0.1, 0.1, 0., 0., 0., 0.1]          # the robot pose of the reference program's "Test the visual covariance"
TILT = 0.7                                    # about the board's y axis: normalCost becomes active
ALPHA_LAST_INVALID = -0.30                    # the turn per step of trajectory 2 that takes only its last pose out of view
YAWS = (0.6, 1.6, 3.1)                        # of a camera 1 m in front of a board of step 0.3: no, some, all corners fail


def _f64(a):
    return np.asarray(a, dtype=np.float64)


@pytest.fixture(scope="module")
def scene():
    cam, w, h, q, steps, start = tr.load_plan(PLAN)
    tilted = copy.deepcopy(q)
    tilted["min_camera_dist"] = 3.5
    tilted["xiOrigBoard"] = [float(v) for v in tr.compose(_f64(q["xiOrigBoard"]), _f64([0, 0, 0, 0, TILT, 0]))]
    board72 = copy.deepcopy(q)
    board72["board"] = dict(cols=9, rows=8, step=0.05)
    wide = copy.deepcopy(q)
    wide["board"]["step"] = 0.3
    return dict(cam=cam, w=w, h=h, steps=steps, start=_f64(start), q=dict(scene=q, tilted=tilted, board72=board72, wide=wide))


@pytest.fixture(scope="module")
def planners(scene):
    from visgeom_amd.trajectory import TrajectoryPlanner

    made = {}

    def get(name):
        if name not in made:
            made[name] = TrajectoryPlanner(scene["cam"], scene["w"], scene["h"], scene["q"][name], scene["steps"])
        return made[name]

    yield get
    for p in made.values():
        p.close()


def _quality(scene, name, dtype=np.float64):
    return tr.Quality(scene["cam"], scene["w"], scene["h"], scene["q"][name], scene["steps"], dtype)


@pytest.fixture(scope="module")
def start_ref(scene):
    """the restatement at the start, computed once: long double and float64"""
    return dict(ld=_quality(scene, "scene", LD).evaluate(scene["start"]), f64=_quality(scene, "scene").evaluate(scene["start"]))


def _fro(a):
    return float(np.sqrt((_f64(a) ** 2).sum()))


@pytest.mark.parametrize("name", ["scene", "board72"])
def test_visual_cov_matches_the_restatement(scene, planners, name):
    """info = JtJ to 1e-10 in the Frobenius norm; cov = JtCJ^-T JtJ JtCJ^-1 to 64 eps cond(JtCJ): backward stability of two
    applications of a 6 x 6 inverse, the 64 covering the constants of n = 6 and an elimination order that is not LAPACK's.
    board72: 72 corners, the second pass of the wave's loop."""
    Q, QL = _quality(scene, name), _quality(scene, name, LD)
    poses = np.concatenate([Q.camera_poses(scene["start"]), [tr.compose(_f64(PROBE), Q.xi_cam)]])
    assert poses.shape == (10, 6)
    cov, info, invalid = planners(name).visual_cov(poses)
    assert invalid.tolist() == [0] * 10
    for k, pose in enumerate(poses):
        V, JtJ, JtCJ, ok = QL.visual_cov(pose)
        V64, JtJ64, _, ok64 = Q.visual_cov(pose)
        assert ok and ok64
        cond = np.linalg.cond(_f64(JtCJ))
        e_info, e_cov, bound = _fro(info[k] - JtJ) / _fro(JtJ), _fro(cov[k] - V) / _fro(V), 64 * EPS * cond
        print("%s pose %d: info %.3g (restatement's spread %.3g), cov %.3g (spread %.3g) of %.3g, cond(JtCJ) %.3g" % (
            name, k, e_info, _fro(JtJ64 - JtJ) / _fro(JtJ), e_cov, _fro(V64 - V) / _fro(V), bound, cond))
        assert e_info <= 1e-10
        assert e_cov <= bound
    one = planners(name).visual_cov(poses[3])
    assert np.array_equal(one[0], cov[3]) and np.array_equal(one[1], info[3]) and one[2] == 0   # a pose's result does not depend on its batch


@pytest.mark.parametrize("name", ["scene", "tilted"])
def test_evaluate_matches_the_restatement(scene, planners, name):
    """cost and each of the five terms to 1e-10 max(1, |ref|).  tilted: min_camera_dist 3.5 and the board turned until normalCost
    is active, so that with the start's image-limit and curvature penalties all four are covered."""
    ref_cost, ref_terms, ref_invalid = _quality(scene, name, LD).evaluate(scene["start"])
    c64, t64, _ = _quality(scene, name).evaluate(scene["start"])
    assert ref_invalid == 0
    if name == "tilted":
        assert (ref_terms[1:] > 1.).all(), ref_terms
    else:
        assert ref_terms[1] > 1. and ref_terms[2] > 1. and ref_terms[3] == ref_terms[4] == 0.
    cost, terms, invalid = planners(name).evaluate(scene["start"])
    assert invalid == 0
    pairs = [("cost", cost, ref_cost, c64)] + [(n, terms[k], ref_terms[k], t64[k]) for k, n in enumerate(("information", "image_limits", "curvature",
                                                                                                               "distance", "normal"))]
    for what, got, ref, r64 in pairs:
        bar = 1e-10 * max(1., abs(float(ref)))
        print("%s %s: %.12g against %.12g, |d| %.3g of %.3g (restatement's spread %.3g)" % (name, what, got, float(ref), abs(got - float(ref)), bar,
                                                                                             abs(float(r64) - float(ref))))
        assert abs(got - float(ref)) <= bar, what


def test_a_point_s_result_does_not_depend_on_its_batch(scene, planners):
    """the start alone, first, middle and last of 21 points, and within 3: identical bits"""
    P = planners("scene")
    s = scene["start"]
    alone = P.evaluate(s)
    rng = np.random.default_rng(5)
    batch = s + 0.01 * rng.standard_normal((21, s.size))
    for k in (0, 10, 20):
        batch[k] = s
    c21, t21, i21 = P.evaluate(batch)
    c3, t3, i3 = P.evaluate(np.stack([batch[1], s, batch[2]]))
    for c, t, i in [(c21[0], t21[0], i21[0]), (c21[10], t21[10], i21[10]), (c21[20], t21[20], i21[20]), (c3[1], t3[1], i3[1])]:
        assert c == alone[0] and np.array_equal(t, alone[1]) and i == alone[2] == 0
    assert len(set(c21.tolist())) == 19 and np.array_equal(c21[1:3], c3[[0, 2]])   # the others are other points, and theirs hold too


def test_gradient_is_the_library_s_own_differences(scene, planners):
    """bit for bit (cost+ - cost-) / (2 delta) from evaluate at the 2 P perturbed points; one batch of three launches"""
    from visgeom_amd import trajectory

    P = planners("scene")
    s = scene["start"]
    pts, delta = trajectory.gradient_points(s)
    c, _, inv = P.evaluate(pts)
    assert inv.tolist() == [0] * 21
    before = P.launches
    cost, grad, invalid = P.gradient(s)
    assert P.launches - before == 3
    assert invalid == 0 and cost == c[0]
    assert np.array_equal(grad, (c[1::2] - c[2::2]) / (2 * delta))
    two = P.gradient(np.stack([s, s]))
    assert np.array_equal(two[1][0], grad) and np.array_equal(two[1][1], grad) and two[0].tolist() == [cost, cost]


def test_gradient_matches_the_long_double_restatement(scene, planners, start_ref):
    """entry i to 64 eps max(1, |cost|) / delta_i: the rounding of the two costs divided by the step is the only error a correct
    implementation has.  Loose for small entries by construction; every entry's slack is printed."""
    g_ref, delta = _quality(scene, "scene", LD).gradient(scene["start"])
    g64, _ = _quality(scene, "scene").gradient(scene["start"])
    cost, grad, invalid = planners("scene").gradient(scene["start"])
    assert invalid == 0
    bound = 64 * EPS * max(1., abs(cost)) / delta
    for i in range(grad.size):
        d = abs(grad[i] - float(g_ref[i]))
        print("g[%d] = %.9g against %.9g: |d| %.3g of %.3g (slack x%.1f; the float64 restatement's own %.3g)" % (
            i, grad[i], float(g_ref[i]), d, bound[i], bound[i] / max(d, 1e-300), abs(g64[i] - float(g_ref[i]))))
    assert (np.abs(grad - _f64(g_ref)) <= bound).all()


def test_invalid_poses_are_reported_and_cost_infinity(scene, planners):
    """hand-placed through visual_cov: a camera 1 m in front of a board of step 0.3, turned about its y axis until no, some and
    all corners leave the projection's domain; then a parameter point whose last pose alone is invalid, between two neighbours
    whose bits must not change"""
    Q = _quality(scene, "wide")
    base = tr.compose(Q.xi_board, _f64([0.3 * 3.5, 0.3 * 2, -1., 0, 0, 0]))
    poses = np.array([tr.compose(base, _f64([0, 0, 0, 0, yaw, 0])) for yaw in YAWS])
    failed = [int((~Q.projections(p)[1]).sum()) for p in poses]
    print("corners that fail in the restatement:", failed)
    assert failed[0] == 0 and 0 < failed[1] < 40 and failed[2] == 40
    cov, info, invalid = planners("wide").visual_cov(poses)
    assert invalid.tolist() == [0, 1, 1]
    assert np.isfinite(cov[0]).all() and np.isfinite(info[0]).all()
    for k in (1, 2):
        assert (cov[k] == np.inf).all() and (info[k] == np.inf).all()
    V = Q.visual_cov(poses[0])[0]
    assert _fro(cov[0] - V) <= 1e-8 * _fro(V)
    # a parameter point
    P, s = planners("scene"), scene["start"]
    bad = s.copy()
    bad[9] = ALPHA_LAST_INVALID
    ref = _quality(scene, "scene").evaluate(bad, detail=True)
    assert ref[2] == 1 and [p["valid"] for p in ref[3]] == [True] * 8 + [False]
    alone = P.evaluate(s)
    cost, terms, invalid = P.evaluate(np.stack([s, bad, s]))
    assert cost[1] == np.inf and terms[1, 0] == np.inf and invalid.tolist() == [0, 1, 0]
    assert np.abs(terms[1, 1:] - _f64(ref[1][1:])).max() <= 1e-10 * max(1., np.abs(_f64(ref[1][1:])).max())   # penalties of the valid poses
    for k in (0, 2):
        assert cost[k] == alone[0] and np.array_equal(terms[k], alone[1])
    c, g, inv = P.gradient(np.stack([s, bad]))
    assert inv.tolist() == [0, 1] and np.isnan(g[1]).all() and np.isfinite(g[0]).all() and c[1] == np.inf


@pytest.fixture(scope="module")
def optimum(scene, planners):
    return planners("scene").optimize(scene["start"])


def test_optimize_works_the_penalties_off(scene, planners, optimum, start_ref):
    """from the start with default options: the returned cost is evaluate's at the returned parameters, the restatement agrees,
    every pose is valid and the cost is no higher than the start's own information term (about -33.87): the 970 of penalty are
    worked off with no net loss of information"""
    P = planners("scene")
    params, cost, iterations, termination = optimum
    start_cost, start_terms, _ = P.evaluate(scene["start"])
    c, terms, invalid = P.evaluate(params)
    ref = _quality(scene, "scene").evaluate(params)
    print("optimize: cost %.10g (information %.6g, penalties %s) after %d iterations, termination %d; the start: %.10g, information %.8g; "
          "the restatement at the result: %.10g" % (cost, terms[0], terms[1:].tolist(), iterations, termination, start_cost, start_terms[0], ref[0]))
    assert cost == c and invalid == 0 and ref[2] == 0
    assert abs(cost - ref[0]) <= 1e-10 * max(1., abs(ref[0]))
    assert abs(start_terms[0] - float(start_ref["ld"][1][0])) <= 1e-10 * abs(start_terms[0])
    assert cost <= start_terms[0]
    assert 1 <= iterations <= 1000 and termination in (0, 1, 2)


def test_two_starts_in_one_call_are_the_two_runs_alone(scene, planners, optimum):
    P = planners("scene")
    other = scene["start"] * np.array([1., 1., 1., 1.2, 0.9, 1., 1., 1., 0.8, 0.7])
    assert P.evaluate(other)[2] == 0
    alone = P.optimize(other)
    before = P.launches
    params, cost, iterations, termination = P.optimize(np.stack([scene["start"], other]))
    assert (P.launches - before) % 3 == 0
    for k, ref in enumerate((optimum, alone)):
        assert np.array_equal(params[k], ref[0]) and cost[k] == ref[1] and iterations[k] == ref[2] and termination[k] == ref[3]
    one = P.optimize(scene["start"], options=dict(max_iterations=2))
    assert one[2] == 2 and one[3] == 3 and one[1] < P.evaluate(scene["start"])[0]   # VG_TERM_NO_CONVERGENCE at the cap


def test_the_program_writes_the_trajectories_and_the_views(scene, planners, tmp_path):
    """`trajectory plan.json` on a copy of the scene without the minimisation and with "views": the start cost it prints is the
    library's, trajectory.json holds [x, y, theta] of every pose, and every pose has its image of the projected corners"""
    import json
    import subprocess

    from visgeom_amd import _build, trajectory

    with open(PLAN) as fh:
        plan = json.load(fh)
    plan["optimize"] = False
    plan["views"] = True
    path = tmp_path / "plan.json"
    path.write_text(json.dumps(plan))
    r = subprocess.run([_build.TRAJECTORY_CLI, str(path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out
    cost = planners("scene").evaluate(scene["start"])[0]
    assert "start cost %.10g " % cost in out and "invalid poses 0" in out
    xi, _ = trajectory.trajectory_poses(scene["start"], scene["steps"])
    with open(tmp_path / "trajectory.json") as fh:
        written = json.load(fh)
    rows = np.array(written["trajectory1"] + written["trajectory2"])
    assert [len(written["trajectory1"]), len(written["trajectory2"])] == scene["steps"]
    assert np.array_equal(rows, xi[:, [0, 1, 5]])
    Q = _quality(scene, "scene")
    o = 0
    for t, n in enumerate(scene["steps"]):
        for i in range(n):
            data = (tmp_path / ("points_%d_%d.pgm" % (t + 1, i))).read_bytes()
            head = b"P5\n1024 768\n255\n"
            assert data.startswith(head) and len(data) == len(head) + 1024 * 768
            img = np.frombuffer(data[len(head):], dtype=np.uint8).reshape(768, 1024)
            uv, ok = Q.projections(tr.compose(xi[o], Q.xi_cam))
            assert ok.all() and (img[:2] == 0).all() and (img[-2:] == 0).all()
            inside = [(int(np.floor(u + 0.5)), int(np.floor(v + 0.5))) for u, v in uv if 1 <= u < 1022 and 3 <= v < 764]
            assert len(inside) >= 30 and all(img[v, u] == 0 and img[v, u - 1] == 0 and img[v + 1, u] == 0 for u, v in inside)
            assert (img[2:-2] == 255).sum() >= 764 * 1024 - 5 * 40
            o += 1
