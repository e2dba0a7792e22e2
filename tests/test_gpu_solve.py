"""The LM driver.  BASELINE.json: "converge to the same intrinsics within 1e-6".  Ceres is
absent on both boxes, so convergence is anchored as SURVEY 8(c) prescribes: (i) noise-free synthetic sets, where
every correct least-squares solver must return the generating intrinsics, and (ii) a noisy set cross-solved with
scipy.optimize.least_squares over the CPU oracle -- the optimum is solver independent."""
import threading

import numpy as np
import pytest

from oracle import vgo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vg():
    import torch

    assert torch.cuda.is_available()
    import visgeom_amd

    return visgeom_amd


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0))


def mono_problem(vg, d, model, lo=0, hi=None, constant_camera=False):
    hi = d["corners"].shape[0] if hi is None else hi
    p = vg.CalibrationProblem(0)
    cam = p.add_camera(model, d["init_intrinsics"], constant=constant_camera)
    seq = p.add_transform(False, d["init_poses"][lo:hi])
    ds = p.add_dataset(cam, [(seq, 0)], d["board"], d["corners"][lo:hi])
    p.finalize()
    return p, cam, seq, ds


@pytest.mark.parametrize("model,n", [("eucm", 200), ("ucm", 120), ("mei", 150)])
def test_noise_free_mono_recovers_generating_intrinsics(vg, model, n):
    from visgeom_amd import synthetic as S

    d = S.make_mono(model, n, 2, sigma=0.0)
    p, cam, seq, ds = mono_problem(vg, d, model)
    s = p.solve(max_num_iterations=100)
    x = p.get_parameters()
    K = len(d["gt_intrinsics"])
    print(model, s["termination"], s["num_iterations"], "cost %.3e -> %.3e" % (s["initial_cost"], s["final_cost"]),
          "intr err %.2e" % rel(x[:K], d["gt_intrinsics"]))
    assert s["final_cost"] < 1e-12 * s["initial_cost"]
    assert rel(x[:K], d["gt_intrinsics"]) < 1e-6
    assert np.max(np.abs(x[K:].reshape(-1, 6) - d["gt_poses"])) < 1e-6
    assert s["num_global_columns"] == K and s["num_pose_blocks"] == n
    p.close()


def test_noise_free_stereo_with_global_transform_and_missing_frames(vg):
    """config-3 shape: two cameras, xiCam12 global (INVERSE in cam-2's chain), poses shared by image index."""
    from visgeom_amd import synthetic as S

    n = 150
    s_ = S.make_stereo(n, sigma=0.0)
    keep2 = np.array([i for i in range(n) if i % 5 != 1], dtype=np.int32)
    p = vg.CalibrationProblem(0)
    c1 = p.add_camera("eucm", s_["init_intrinsics1"])
    c2 = p.add_camera("eucm", s_["init_intrinsics2"])
    x12 = p.add_transform(True, s_["init_xi12"])
    seq = p.add_transform(False, s_["init_poses"])
    p.add_dataset(c1, [(seq, 0)], s_["board"], s_["corners1"])
    p.add_dataset(c2, [(x12, 1), (seq, 0)], s_["board"], s_["corners2"][keep2], image_index=keep2)
    p.finalize()
    s = p.solve(max_num_iterations=100)
    x = p.get_parameters()
    print("stereo", s["termination"], s["num_iterations"], "cost %.3e -> %.3e" % (s["initial_cost"], s["final_cost"]))
    assert s["num_global_columns"] == 18
    assert rel(x[0:6], s_["gt_intrinsics1"]) < 1e-6 and rel(x[6:12], s_["gt_intrinsics2"]) < 1e-6
    assert np.max(np.abs(x[12:18] - s_["gt_xi12"])) < 1e-6
    assert np.max(np.abs(x[18:].reshape(-1, 6) - s_["gt_poses"])) < 1e-6
    p.close()


def test_constant_blocks_stay_fixed(vg):
    from visgeom_amd import synthetic as S

    d = S.make_mono("eucm", 60, 2, sigma=0.0)
    d["init_intrinsics"] = d["gt_intrinsics"].copy()
    p, cam, seq, ds = mono_problem(vg, d, "eucm", constant_camera=True)
    s = p.solve(max_num_iterations=50)
    x = p.get_parameters()
    assert np.array_equal(x[:6], d["gt_intrinsics"])  # SetParameterBlockConstant (unified_calibration.cpp:614-617)
    assert np.max(np.abs(x[6:].reshape(-1, 6) - d["gt_poses"])) < 1e-7
    assert s["final_cost"] < 1e-12 * s["initial_cost"]
    p.close()


def test_noisy_set_matches_scipy_least_squares_on_the_oracle(vg):
    """the least-squares optimum does not depend on the solver: scipy trf over the oracle's residuals and
    Jacobians stands in for "what Ceres would converge to" (SURVEY 8(c))."""
    from scipy.optimize import least_squares

    from visgeom_amd import synthetic as S

    n, N = 16, 96
    d = S.make_mono("eucm", n, 2, sigma=0.1)
    x0 = np.concatenate([d["init_intrinsics"], d["init_poses"].ravel()])

    def fun(x):
        r, _, _ = vgo.eval_dataset(vgo.MODEL_EUCM, [0], d["board"], d["corners"], x, 0, [6], [6], np.arange(n), want_jac=False)
        return r.ravel()

    def jac(x):
        _, ji, jm = vgo.eval_dataset(vgo.MODEL_EUCM, [0], d["board"], d["corners"], x, 0, [6], [6], np.arange(n))
        J = np.zeros((n * 2 * N, x.size))
        J[:, :6] = ji.reshape(-1, 6)
        for b in range(n):
            J[b * 2 * N:(b + 1) * 2 * N, 6 + 6 * b:12 + 6 * b] = jm[0][b]
        return J

    lb = np.full(x0.size, -np.inf)
    ub = np.full(x0.size, np.inf)
    lb[:6] = [0, 0.1, 1, 1, 1, 1]       # eucm.h:228-246
    ub[:6] = [1, 10, 1e5, 1e5, 1e5, 1e5]
    ref = least_squares(fun, x0, jac=jac, bounds=(lb, ub), method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                        max_nfev=400)
    p, cam, seq, ds = mono_problem(vg, d, "eucm")
    s = p.solve(max_num_iterations=200)
    x = p.get_parameters()
    print("noisy", s["termination"], s["num_iterations"], "cost gpu %.12e scipy %.12e" % (s["final_cost"], ref.cost),
          "intr diff %.2e" % rel(x[:6], ref.x[:6]))
    assert abs(s["final_cost"] - ref.cost) <= 1e-9 * ref.cost
    assert rel(x[:6], ref.x[:6]) < 1e-6
    assert np.max(np.abs(x[6:] - ref.x[6:])) < 1e-6
    p.close()


def test_two_shards_with_allreduce_equal_one_problem(vg):
    """multi-GPU path by construction: images split over two problem instances (two "ranks", here two host
    threads on one GPU), global parameters replicated, one summing all-reduce callback.  The result must equal
    the single-problem solve."""
    import torch

    from visgeom_amd import synthetic as S

    n = 120
    d = S.make_mono("eucm", n, 2, sigma=0.1)
    p, *_ = mono_problem(vg, d, "eucm")
    s_ref = p.solve(max_num_iterations=60)
    x_ref = p.get_parameters()
    p.close()

    barrier = threading.Barrier(2)
    slots = [None, None]
    results = [None, None]

    def make_allreduce(rank):
        def allreduce(buf):
            slots[rank] = buf.copy()
            barrier.wait()
            total = slots[0] + slots[1]
            barrier.wait()
            buf[:] = total
        return allreduce

    def worker(rank):
        with torch.cuda.stream(torch.cuda.Stream()):
            lo, hi = (0, 70) if rank == 0 else (70, n)
            q, *_ = mono_problem(vg, d, "eucm", lo, hi)
            s = q.solve(allreduce=make_allreduce(rank), max_num_iterations=60)
            results[rank] = (s, q.get_parameters())
            q.close()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert all(r is not None for r in results)
    (s0, x0), (s1, x1) = results
    assert s0["num_iterations"] == s1["num_iterations"] and s0["termination"] == s1["termination"]
    assert np.array_equal(x0[:6], x1[:6])                       # replicated global block stays bit-identical
    assert rel(x0[:6], x_ref[:6]) < 1e-8
    assert abs(s0["final_cost"] - s_ref["final_cost"]) <= 1e-9 * s_ref["final_cost"]
    poses = np.concatenate([x0[6:], x1[6:]])
    assert np.max(np.abs(poses - x_ref[6:])) < 1e-7


def test_transformation_prior_matches_scipy_on_the_oracle(vg):
    """a stiff TransformationPrior on the stereo transform (parseData :808-829): the optimum of grid residuals +
    prior block must equal scipy's over the oracle's residuals (grid rows + vgo.transformation_prior)."""
    from scipy.optimize import least_squares

    from visgeom_amd import synthetic as S

    n, N = 10, 96
    s = S.make_stereo(n, sigma=0.1)
    prior = s["gt_xi12"] + np.array([0.02, -0.01, 0.015, 0.01, -0.02, 0.01])   # a deliberately wrong prior
    stiff = np.array([300.0, 300.0, 300.0, 500.0, 500.0, 500.0])
    x0 = np.concatenate([s["init_intrinsics1"], s["init_intrinsics2"], prior, s["init_poses"].ravel()])

    def parts(x, jac):
        r1, j1i, j1m = vgo.eval_dataset(0, [0], s["board"], s["corners1"], x, 0, [18], [6], np.arange(n), want_jac=jac)
        r2, j2i, j2m = vgo.eval_dataset(0, [1, 0], s["board"], s["corners2"], x, 6, [12, 18], [0, 6], np.arange(n), want_jac=jac)
        rp, Jp = vgo.transformation_prior(stiff, prior, x[12:18])
        return r1, j1i, j1m, r2, j2i, j2m, rp, Jp

    def fun(x):
        r1, _, _, r2, _, _, rp, _ = parts(x, False)
        return np.concatenate([r1.ravel(), r2.ravel(), rp])

    def jac(x):
        r1, j1i, j1m, r2, j2i, j2m, rp, Jp = parts(x, True)
        J = np.zeros((2 * n * 2 * N + 6, x.size))
        for b in range(n):
            rows = slice(b * 2 * N, (b + 1) * 2 * N)
            J[rows, 0:6] = j1i[b]
            J[rows, 18 + 6 * b:24 + 6 * b] = j1m[0][b]
            rows = slice(n * 2 * N + b * 2 * N, n * 2 * N + (b + 1) * 2 * N)
            J[rows, 6:12] = j2i[b]
            J[rows, 12:18] = j2m[0][b]
            J[rows, 18 + 6 * b:24 + 6 * b] = j2m[1][b]
        J[-6:, 12:18] = Jp
        return J

    ref = least_squares(fun, x0, jac=jac, method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=500)
    p = vg.CalibrationProblem(0)
    c1 = p.add_camera("eucm", s["init_intrinsics1"])
    c2 = p.add_camera("eucm", s["init_intrinsics2"])
    x12 = p.add_transform(True, prior)
    seq = p.add_transform(False, s["init_poses"])
    p.add_dataset(c1, [(seq, 0)], s["board"], s["corners1"])
    p.add_dataset(c2, [(x12, 1), (seq, 0)], s["board"], s["corners2"])
    p.add_transformation_prior(x12, stiff)
    p.finalize()
    summ = p.solve(max_num_iterations=300, use_bounds=0)
    x = p.get_parameters()
    print("prior", summ["termination"], summ["num_iterations"], "cost gpu %.10e scipy %.10e" % (summ["final_cost"], ref.cost))
    # The reference's prior Jacobian is the CONSTANT matrix A (calib_cost_functions.cpp:224-227), exact only at
    # xi = prior.  J^T r = 0 and "cost minimal" are then two slightly different points (the prior sits 2 cm / 1 deg
    # off on purpose), every trust-region solver ends between them, so solver-to-solver agreement is 1e-6 in cost
    # and 1e-4 in parameters here, not the 1e-14 of the exact-Jacobian problems above.
    g = jac(x).T @ fun(x)
    g0 = jac(x0).T @ fun(x0)
    assert np.max(np.abs(g)) <= 1e-6 * np.max(np.abs(g0))
    assert summ["final_cost"] <= ref.cost * (1 + 1e-12) and abs(summ["final_cost"] - ref.cost) <= 1e-6 * ref.cost
    assert np.max(np.abs(x[12:18] - ref.x[12:18])) < 1e-4
    assert rel(x[:12], ref.x[:12]) < 1e-4
    # the prior really pulls: without it the transform sits elsewhere
    assert np.max(np.abs(ref.x[12:18] - s["gt_xi12"])) > 1e-4
    p.close()


def _handeye_reference(d, n, errV, errW, lam, x0):
    """scipy over the oracle: grid rows of the chain [xiBaseCam I, xiOdomBase_i I, xiOdomBoard D] + one
    vgo.OdometryPrior per consecutive pair; element 0 of the sequence is held constant (anchor)."""
    from scipy.optimize import least_squares

    N = d["board"].shape[0]
    blocks = [vgo.OdometryPrior(errV, errW, lam, d["odometry"][i], d["odometry"][i + 1]) for i in range(n - 1)]
    free = np.ones(x0.size, dtype=bool)
    free[18:24] = False

    def full(z):
        x = x0.copy()
        x[free] = z
        return x

    def fun(z):
        x = full(z)
        r, _, _ = vgo.eval_dataset(0, [1, 1, 0], d["board"], d["corners"], x, 0, [6, 18, 12], [0, 6, 0], np.arange(n), want_jac=False)
        ro = [b.evaluate(x[18 + 6 * i:24 + 6 * i], x[24 + 6 * i:30 + 6 * i])[0] for i, b in enumerate(blocks)]
        return np.concatenate([r.ravel()] + ro)

    def jac(z):
        x = full(z)
        _, ji, jm = vgo.eval_dataset(0, [1, 1, 0], d["board"], d["corners"], x, 0, [6, 18, 12], [0, 6, 0], np.arange(n), want_jac=True)
        J = np.zeros((2 * N * n + 6 * (n - 1), x.size))
        for b in range(n):
            rows = slice(b * 2 * N, (b + 1) * 2 * N)
            J[rows, 0:6] = ji[b]
            J[rows, 6:12] = jm[0][b]
            J[rows, 18 + 6 * b:24 + 6 * b] = jm[1][b]
            J[rows, 12:18] = jm[2][b]
        for i, blk in enumerate(blocks):
            _, J1, J2 = blk.evaluate(x[18 + 6 * i:24 + 6 * i], x[24 + 6 * i:30 + 6 * i])
            rows = slice(2 * N * n + 6 * i, 2 * N * n + 6 * i + 6)
            J[rows, 18 + 6 * i:24 + 6 * i] = J1
            J[rows, 24 + 6 * i:30 + 6 * i] = J2
        return J[:, free]

    ref = least_squares(fun, x0[free], jac=jac, method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=500)
    return ref, full, fun, jac, free


@pytest.mark.parametrize("lam", [0.05, 1.0])
def test_odometry_prior_matches_scipy_on_the_oracle(vg, lam):
    """data type "odometry" (unified_calibration.cpp:743-807): OdometryPrior blocks couple consecutive elements of
    the sequence, so the pose system is block tridiagonal instead of block diagonal; anchor = element 0 constant.
    Hand-eye set: camera on a moving base, chain [xiBaseCam I, xiOdomBase_i I, xiOdomBoard D]."""
    from visgeom_amd import synthetic as S

    n = 12
    d = S.make_handeye(n, sigma=0.1)
    errV, errW = 0.05, 0.05
    x0 = np.concatenate([d["init_intrinsics"], d["init_xi_base_cam"], d["init_xi_odom_board"], d["odometry"].ravel()])
    ref, full, fun, jac, free = _handeye_reference(d, n, errV, errW, lam, x0)

    p = vg.CalibrationProblem(0)
    cam = p.add_camera("eucm", d["init_intrinsics"])
    bc = p.add_transform(True, d["init_xi_base_cam"])
    ob = p.add_transform(True, d["init_xi_odom_board"])
    seq = p.add_transform(False, d["odometry"])
    p.add_dataset(cam, [(bc, 1), (seq, 1), (ob, 0)], d["board"], d["corners"])
    for i in range(n - 1):
        p.add_odometry_prior(seq, i, errV, errW, lam, d["odometry"][i], d["odometry"][i + 1])
    p.set_pose_constant(seq, 0)
    p.finalize()
    summ = p.solve(max_num_iterations=300, use_bounds=0)
    x = p.get_parameters()
    print("odometry lam=%g" % lam, summ["termination"], summ["num_iterations"],
          "cost gpu %.10e scipy %.10e (initial %.4e)" % (summ["final_cost"], ref.cost, summ["initial_cost"]))
    assert np.array_equal(x[18:24], x0[18:24])                      # the anchor did not move
    assert abs(summ["initial_cost"] - 0.5 * np.sum(fun(x0[free]) ** 2)) <= 1e-10 * summ["initial_cost"]
    assert abs(summ["final_cost"] - 0.5 * np.sum(fun(x[free]) ** 2)) <= 1e-10 * summ["final_cost"]
    # the reference's odometry Jacobians are first-order approximations (tests/test_oracle_math.py), so like the
    # TransformationPrior case the comparison is solver-to-solver: gradient (by the reference's J) reduced, same cost.
    g = jac(x[free]).T @ fun(x[free])
    g0 = jac(x0[free]).T @ fun(x0[free])
    assert np.max(np.abs(g)) <= 1e-5 * np.max(np.abs(g0))
    assert abs(summ["final_cost"] - ref.cost) <= 1e-5 * ref.cost
    assert rel(x[:6], full(ref.x)[:6]) < 1e-4
    assert np.max(np.abs(x[6:] - full(ref.x)[6:])) < 1e-3
    # calibration sanity: the hand-eye transform is recovered
    assert np.max(np.abs(x[6:12] - d["gt_xi_base_cam"])) < 5e-3
    p.close()


@pytest.mark.parametrize("with_odometry", [False, True])
def test_transformation_prior_on_a_sequence_acts_on_element_zero(vg, with_odometry):
    """parseData :808-829 hands getTransformData(name) = element 0 of a sequence to TransformationPrior.  Mono EUCM
    set, a stiff and deliberately wrong prior on pose 0; optionally odometry blocks on the same sequence (then both
    kinds of block meet in the same block-tridiagonal elimination)."""
    from scipy.optimize import least_squares

    from visgeom_amd import synthetic as S

    n, N = 8, 96
    d = S.make_mono("eucm", n, 2, sigma=0.1)
    # The reference's prior Jacobian is diag(stiffness) * M(prior rot) where the exact one is diag * R * M: off by the
    # prior's rotation.  With a board pose of 2-3 rad it is unusable (every solver stalls somewhere else), so pose 0
    # is replaced by a nearly fronto-parallel one (|rot| = 0.04), the regime the block can work in.
    gt0 = np.array([-0.55, -0.35, 1.0, 0.03, -0.02, 0.015])
    uv, ok = S.project("eucm", d["gt_intrinsics"], (S.rodrigues(gt0[3:]) @ d["board"].T).T + gt0[:3])
    assert ok.all() and uv.min() > 20 and uv[:, 0].max() < S.IMAGE_W - 20 and uv[:, 1].max() < S.IMAGE_H - 20
    d["corners"][0] = uv + 0.1 * np.random.default_rng(8).standard_normal(uv.shape)
    d["gt_poses"][0] = gt0
    d["init_poses"][0] = gt0 + np.array([0.008, -0.006, 0.009, -0.007, 0.005, 0.006])
    x0 = np.concatenate([d["init_intrinsics"], d["init_poses"].ravel()])
    prior = d["init_poses"][0].copy()
    stiff = np.array([400.0, 400.0, 400.0, 600.0, 600.0, 600.0])
    odo = d["gt_poses"] + 0.003 * np.random.default_rng(3).standard_normal((n, 6))
    blocks = [vgo.OdometryPrior(0.05, 0.05, 0.2, odo[i], odo[i + 1]) for i in range(n - 1)] if with_odometry else []

    def fun(x):
        r, _, _ = vgo.eval_dataset(0, [0], d["board"], d["corners"], x, 0, [6], [6], np.arange(n), want_jac=False)
        rp, _ = vgo.transformation_prior(stiff, prior, x[6:12])
        ro = [b.evaluate(x[6 + 6 * i:12 + 6 * i], x[12 + 6 * i:18 + 6 * i])[0] for i, b in enumerate(blocks)]
        return np.concatenate([r.ravel(), rp] + ro)

    def jac(x):
        _, ji, jm = vgo.eval_dataset(0, [0], d["board"], d["corners"], x, 0, [6], [6], np.arange(n), want_jac=True)
        J = np.zeros((2 * N * n + 6 + 6 * len(blocks), x.size))
        for b in range(n):
            rows = slice(b * 2 * N, (b + 1) * 2 * N)
            J[rows, 0:6] = ji[b]
            J[rows, 6 + 6 * b:12 + 6 * b] = jm[0][b]
        J[2 * N * n:2 * N * n + 6, 6:12] = vgo.transformation_prior(stiff, prior, x[6:12])[1]
        for i, blk in enumerate(blocks):
            _, J1, J2 = blk.evaluate(x[6 + 6 * i:12 + 6 * i], x[12 + 6 * i:18 + 6 * i])
            rows = slice(2 * N * n + 6 + 6 * i, 2 * N * n + 12 + 6 * i)
            J[rows, 6 + 6 * i:12 + 6 * i] = J1
            J[rows, 12 + 6 * i:18 + 6 * i] = J2
        return J

    ref = least_squares(fun, x0, jac=jac, method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=500)
    p = vg.CalibrationProblem(0)
    cam = p.add_camera("eucm", d["init_intrinsics"])
    seq = p.add_transform(False, d["init_poses"])
    p.add_dataset(cam, [(seq, 0)], d["board"], d["corners"])
    p.add_transformation_prior(seq, stiff)
    for i in range(len(blocks)):
        p.add_odometry_prior(seq, i, 0.05, 0.05, 0.2, odo[i], odo[i + 1])
    p.finalize()
    summ = p.solve(max_num_iterations=300, use_bounds=0)
    x = p.get_parameters()
    print("sequence prior odo=%s" % with_odometry, summ["termination"], summ["num_iterations"],
          "cost gpu %.10e scipy %.10e" % (summ["final_cost"], ref.cost))
    assert abs(summ["initial_cost"] - 0.5 * np.sum(fun(x0) ** 2)) <= 1e-10 * summ["initial_cost"]
    assert abs(summ["final_cost"] - 0.5 * np.sum(fun(x) ** 2)) <= 1e-10 * summ["final_cost"]
    g, g0 = jac(x).T @ fun(x), jac(x0).T @ fun(x0)
    assert np.max(np.abs(g)) <= 1e-5 * np.max(np.abs(g0))
    assert abs(summ["final_cost"] - ref.cost) <= 1e-5 * ref.cost
    assert np.max(np.abs(x[6:] - ref.x[6:])) < 1e-3 and rel(x[:6], ref.x[:6]) < 1e-4
    # the prior pulls pose 0 away from where the images alone put it
    free = least_squares(lambda z: fun(z)[:2 * N * n], x0, method="trf", x_scale="jac", max_nfev=200)
    assert np.max(np.abs(x[6:12] - free.x[6:12])) > 1e-4
    p.close()


def test_soft_l1_loss_per_residual_block(vg):
    """vg_solve_options.soft_l1_scale = a: ceres::SoftLOneLoss(a) on every grid block (what the reference's initial
    refinements use, unified_calibration.cpp:379-401 a = 1, :1143 a = 25).  Intrinsics free, poses constant, one image
    with corners shifted by 25 px: the robust optimum must equal scipy's minimum of sum_b rho(|r_b|^2) over the
    oracle's residuals, and sit closer to the generating intrinsics than the plain least-squares one."""
    from scipy.optimize import least_squares

    from visgeom_amd import synthetic as S

    n, N, a = 12, 96, 1.0
    d = S.make_mono("eucm", n, 2, sigma=0.1)
    corners = d["corners"].copy()
    corners[4] += np.array([25.0, -15.0])
    x0 = np.concatenate([d["init_intrinsics"], d["gt_poses"].ravel()])

    def blocks(k):
        x = x0.copy()
        x[:6] = k
        r, _, _ = vgo.eval_dataset(0, [0], d["board"], corners, x, 0, [6], [6], np.arange(n), want_jac=False)
        return r.reshape(n, -1)

    def robust(k):
        r = blocks(k)
        s = np.sum(r * r, axis=1)
        rho = 2 * a * a * (np.sqrt(1 + s / (a * a)) - 1)
        return (r * np.sqrt(rho / s)[:, None]).ravel()

    ref = least_squares(robust, x0[:6], jac="3-point", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    plain = least_squares(lambda k: blocks(k).ravel(), x0[:6], jac="3-point", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15)

    def solve(scale):
        p = vg.CalibrationProblem(0)
        cam = p.add_camera("eucm", d["init_intrinsics"])
        seq = p.add_transform(False, d["gt_poses"], constant=True)
        p.add_dataset(cam, [(seq, 0)], d["board"], corners)
        p.finalize()
        summ = p.solve(max_num_iterations=300, use_bounds=0, soft_l1_scale=scale)
        k = p.get_parameters()[:6]
        p.close()
        return summ, k

    s_rob, k_rob = solve(a)
    s_pl, k_pl = solve(0.0)
    print("soft-l1", s_rob["termination"], s_rob["num_iterations"], "cost %.8e scipy %.8e" % (s_rob["final_cost"], ref.cost),
          "| plain cost %.6e" % s_pl["final_cost"])
    assert abs(s_rob["final_cost"] - ref.cost) <= 1e-9 * ref.cost
    assert rel(k_rob, ref.x) < 1e-6
    assert abs(s_pl["final_cost"] - plain.cost) <= 1e-9 * plain.cost and rel(k_pl, plain.x) < 1e-6
    e_rob, e_pl = rel(k_rob, d["gt_intrinsics"]), rel(k_pl, d["gt_intrinsics"])
    print("error vs generating intrinsics: robust %.2e plain %.2e" % (e_rob, e_pl))
    assert e_rob < 0.5 * e_pl


def test_active_bound_matches_scipy_bounded_least_squares(vg):
    """box bounds of the camera models (ucm.h:199-215: xi in [0, 3]) are set on the intrinsic blocks
    (unified_calibration.cpp:621-627).  Data generated with xi = 3.2: the constrained optimum sits ON the bound;
    it must equal scipy's bounded trust-region solution over the oracle."""
    from scipy.optimize import least_squares

    from visgeom_amd import synthetic as S

    n, N = 30, 96
    gt = S.GT_UCM.copy()
    gt[0] = 3.2
    gt[1:3] *= (1 + 3.2) / (1 + S.GT_UCM[0])      # keep the image scale: f / (1 + xi) unchanged
    d = S.make_mono("ucm", n, 2, sigma=0.1, gt=gt)
    x0 = np.concatenate([d["init_intrinsics"], d["init_poses"].ravel()])

    def parts(x, want):
        return vgo.eval_dataset(vgo.MODEL_UCM, [0], d["board"], d["corners"], x, 0, [5], [6], np.arange(n), want_jac=want)

    def fun(x):
        return parts(x, False)[0].ravel()

    def jac(x):
        _, ji, jm = parts(x, True)
        J = np.zeros((2 * N * n, x.size))
        for b in range(n):
            rows = slice(b * 2 * N, (b + 1) * 2 * N)
            J[rows, 0:5] = ji[b]
            J[rows, 5 + 6 * b:11 + 6 * b] = jm[0][b]
        return J

    lo = np.full(x0.size, -np.inf)
    hi = np.full(x0.size, np.inf)
    lo[:5] = [0, 1, 1, 1, 1]
    hi[:5] = [3, 1e5, 1e5, 1e5, 1e5]
    ref = least_squares(fun, x0, jac=jac, bounds=(lo, hi), method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=500)
    p, cam, seq, ds = mono_problem(vg, d, "ucm")
    s = p.solve(max_num_iterations=300)      # use_bounds = 1 is the default
    x = p.get_parameters()
    print("bounded", s["termination"], s["num_iterations"], "cost gpu %.10e scipy %.10e xi %.6f" % (s["final_cost"], ref.cost, x[0]))
    assert x[0] == 3.0                                           # exactly on the bound, never beyond
    assert abs(ref.x[0] - 3.0) < 1e-6
    assert abs(s["final_cost"] - ref.cost) <= 1e-7 * ref.cost
    assert rel(x[1:5], ref.x[1:5]) < 1e-5
    # without bounds the same data go past xi = 3
    p2, _, _, _ = mono_problem(vg, d, "ucm")
    p2.solve(max_num_iterations=300, use_bounds=0)
    assert p2.get_parameters()[0] > 3.05
    p.close()
    p2.close()


def test_degenerate_structures(vg):
    """nothing free; a dataset without images next to a populated one; one image only"""
    from visgeom_amd import synthetic as S

    d = S.make_mono("eucm", 12, 2, sigma=0.1)
    # (1) every block constant: the solve is a cost evaluation
    p = vg.CalibrationProblem(0)
    cam = p.add_camera("eucm", d["init_intrinsics"], constant=True)
    seq = p.add_transform(False, d["init_poses"], constant=True)
    p.add_dataset(cam, [(seq, 0)], d["board"], d["corners"])
    p.finalize()
    x0 = p.get_parameters()
    s = p.solve(max_num_iterations=20)
    r, _, _ = vgo.eval_dataset(0, [0], d["board"], d["corners"], x0, 0, [6], [6], np.arange(12), want_jac=False)
    assert np.array_equal(p.get_parameters(), x0)
    assert abs(s["final_cost"] - 0.5 * np.sum(r * r)) <= 1e-12 * s["final_cost"] and s["initial_cost"] == s["final_cost"]
    p.close()
    # (2) an empty dataset (all of its frames had no pattern) next to a populated one
    p = vg.CalibrationProblem(0)
    cam = p.add_camera("eucm", d["init_intrinsics"])
    seq = p.add_transform(False, d["init_poses"])
    seq2 = p.add_transform(False, d["init_poses"][:3])
    p.add_dataset(cam, [(seq, 0)], d["board"], d["corners"])
    p.add_dataset(cam, [(seq2, 0)], d["board"], np.zeros((0, 96, 2)), image_index=np.zeros(0, dtype=np.int32))
    p.finalize()
    s = p.solve(max_num_iterations=100)
    x = p.get_parameters()
    assert rel(x[:6], d["gt_intrinsics"]) < 2e-2 and s["final_cost"] < 1e-3 * s["initial_cost"]
    assert np.array_equal(x[6 + 72:], d["init_poses"][:3].ravel())      # unreferenced poses do not move
    p.close()
    # (4) no sequence member at all: five noisy views of ONE board pose held by a global transform (no pose blocks)
    pose = d["gt_poses"][0]
    uv, ok = S.project("eucm", d["gt_intrinsics"], (S.rodrigues(pose[3:]) @ d["board"].T).T + pose[:3])
    assert ok.all()
    views = uv[None] + 0.1 * np.random.default_rng(2).standard_normal((5, 96, 2))
    p = vg.CalibrationProblem(0)
    cam = p.add_camera("eucm", d["gt_intrinsics"], constant=True)
    glob = p.add_transform(True, pose + 0.01)
    p.add_dataset(cam, [(glob, 0)], d["board"], views)
    p.finalize()
    s = p.solve(max_num_iterations=100)
    assert s["num_pose_blocks"] == 0 and s["num_global_columns"] == 12
    assert np.max(np.abs(p.get_parameters()[6:12] - pose)) < 1e-3 and s["final_cost"] < 1e-2 * s["initial_cost"]
    p.close()
    # (3) a single image: 6 + 6 unknowns against 192 residuals
    p = vg.CalibrationProblem(0)
    cam = p.add_camera("eucm", d["gt_intrinsics"], constant=True)
    seq = p.add_transform(False, d["init_poses"][:1])
    p.add_dataset(cam, [(seq, 0)], d["board"], d["corners"][:1])
    p.finalize()
    s = p.solve(max_num_iterations=100)
    assert np.max(np.abs(p.get_parameters()[6:] - d["gt_poses"][0])) < 2e-3
    p.close()


def test_no_device_memory_leak_over_repeated_problems(vg, tmp_path):
    """create -> use -> close, many times, for every object of the library that owns HIP memory: its own hipMalloc'ed
    workspaces (frames, partials, solver buffers, scratch, pinned host memory) must all be returned; device-wide free memory
    stays put.  The refinement's cached blocks go back through vg_release_cached_memory."""
    import torch

    from visgeom_amd import localization as loc, stereo, synthetic as S
    from visgeom_amd.calibration import GenericCameraCalibration, refine_poses
    from visgeom_amd.corners import CornerDetector
    from visgeom_amd.distributed import Comm
    from tests import stereo_scene

    d = S.make_mono("eucm", 300, 2, sigma=0.1)
    rng = np.random.default_rng(5)

    def problem():
        p, cam, seq, ds = mono_problem(vg, d, "eucm")
        res, ji, jm = p.alloc_outputs(ds)
        gram, gsum = p.alloc_gram(ds)
        p.prepare()
        p.evaluate_dataset(ds, res, ji, jm)
        p.gram_fused(ds, gram)
        p.gram_sum(ds, gram, gsum)
        hres = np.empty((300, 192))
        hji = np.empty((300, 192, 6))
        hjm = [np.empty((300, 192, 6))]
        p.evaluate_dataset_to_host(ds, hres, hji, hjm)
        p.solve(max_num_iterations=5)
        p.close()
        del res, ji, jm, gram, gsum

    prm = stereo.make_params(u_max=125, v_max=93, u0=15, v0=15, equal_margins=1, disp_max=32, error_max=150, flaw_cost=25,
                             desc_length=5, scales=[1, 2, 3, 5], desc_resp_thresh=2, use_uv_cache=0, epipole_margin=2500)
    pair = [torch.from_numpy(rng.integers(0, 256, (2, 93, 125), dtype=np.uint8)).cuda() for _ in range(2)]

    def dense_stereo():
        s = stereo.Stereo(stereo_scene.CAM1, stereo_scene.CAM2, stereo_scene.RIGS["sideways"], prm)
        s.compute(*pair)
        s.close()

    images = torch.from_numpy(rng.integers(0, 256, (2, 96, 128), dtype=np.uint8)).cuda()

    def corner_detector():
        det = CornerDetector(5, 4)
        det.detect(images)
        det.close()

    intr, xb = d["gt_intrinsics"], np.array([0.01, 0.02, 0.03, 0.0, 0.0, 0.1])
    x1 = np.column_stack([rng.uniform(-1, 1, (64, 2)), rng.uniform(2, 4, 64)])
    x2, p2, size = x1 + 0.1, rng.uniform(100, 200, (64, 2)), rng.uniform(0.5, 2, 64)

    def mono_reproject():
        cost = loc.MonoReprojectCost("eucm", intr, x1[:5], p2[:5], xb)
        cost.Evaluate([np.zeros(6), np.full(5, 3.0)])
        cost.close()

    def sparse_reproject():
        cost = loc.SparseReprojectCost("eucm", intr, x1, x2, p2, size, xb)
        cost.Evaluate([np.zeros(6)])
        cost.close()

    def block_group():
        group = vg.BlockGroup(0)
        blocks = [vg.GenericProjectionJac(d["corners"][i], d["board"], "eucm", [0], group=group) for i in range(4)]
        for _ in range(2):
            for i, b in enumerate(blocks):
                b.Evaluate([d["init_intrinsics"], d["init_poses"][i]])
        for b in blocks:
            b.close()
        group.close()

    def local_comm():
        (c,) = Comm.local_group(1)
        buf = torch.ones(1000, dtype=torch.float64, device="cuda")
        c.allreduce_sum(buf)
        torch.cuda.synchronize()
        c.close()

    small = S.make_mono("eucm", 20, 0, sigma=0.1)
    calib_json = S.write_calibration_json(str(tmp_path), small, "eucm", prior=False, init=True)

    def calibration():
        c = GenericCameraCalibration()
        c.addResiduals(calib_json)
        c.compute(max_num_iterations=5)
        c.close()

    def refinement():
        refine_poses("eucm", d["gt_intrinsics"], d["board"], d["corners"], d["init_poses"], max_num_iterations=5)
        vg.release_cached_memory()

    for once in (problem, dense_stereo, corner_detector, mono_reproject, sparse_reproject, block_group, local_comm, calibration,
                 refinement):
        for _ in range(3):
            once()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free0, _ = torch.cuda.mem_get_info()
        for _ in range(40):
            once()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free1, _ = torch.cuda.mem_get_info()
        assert free0 - free1 < 8 << 20, "%s leaked %.1f MiB over 40 cycles" % (once.__name__, (free0 - free1) / 2**20)


def test_argument_errors_of_the_block_level_entries(vg):
    """error behaviour of the prior / odometry / constant-pose entries: codes, not crashes; state errors after finalize"""
    from visgeom_amd import capi, synthetic as S

    d = S.make_mono("eucm", 4, 2)
    p = vg.CalibrationProblem(0)
    cam = p.add_camera("eucm", d["init_intrinsics"])
    glob = p.add_transform(True, [0.1, 0, 0, 0, 0, 0])
    seq = p.add_transform(False, d["init_poses"])
    xi = d["init_poses"]
    bad = [lambda: p.add_odometry_prior(glob, 0, 0.1, 0.1, 0.1, xi[0], xi[1]),       # not a sequence
           lambda: p.add_odometry_prior(seq, 3, 0.1, 0.1, 0.1, xi[0], xi[1]),        # couples 3 and 4: out of range
           lambda: p.add_odometry_prior(seq, -1, 0.1, 0.1, 0.1, xi[0], xi[1]),
           lambda: p.add_odometry_prior(seq, 0, 0.1, 0.1, 0.0, xi[0], xi[1]),        # lambda must be positive
           lambda: p.add_odometry_prior(99, 0, 0.1, 0.1, 0.1, xi[0], xi[1]),
           lambda: p.set_pose_constant(glob, 0),
           lambda: p.set_pose_constant(seq, 4),
           lambda: p.add_transformation_prior(42, np.ones(6))]
    for f in bad:
        with pytest.raises(capi.VisgeomError):
            f()
    with pytest.raises(ValueError):
        p.add_transformation_prior(glob, np.ones(5))
    p.add_dataset(cam, [(glob, 1), (seq, 0)], d["board"], d["corners"])
    p.add_odometry_prior(seq, 0, 0.1, 0.1, 0.1, xi[0], xi[1])
    p.finalize()
    for f in (lambda: p.add_odometry_prior(seq, 1, 0.1, 0.1, 0.1, xi[1], xi[2]), lambda: p.set_pose_constant(seq, 0),
              lambda: p.add_transformation_prior(glob, np.ones(6))):
        with pytest.raises(capi.VisgeomError) as e:
            f()
        assert "finalized" in str(e.value)
    # odometry blocks + a multi-rank all-reduce callback: refused (the coupled chain cannot be cut without an exchange)
    with pytest.raises(capi.VisgeomError) as e:
        p.solve(allreduce=lambda buf: None, max_num_iterations=2)
    assert "all-reduce" in str(e.value)
    p.close()


def _wheeled_reference(d, n, errV, errW, lam, x0):
    """scipy TRF on the oracle for the wheeled-base problem; x = [intrinsics 6 | xiBaseCam 6 | xiOdomBoard 6 |
    xiOdomBase n x 6 | wheels 3] (the product's layout: cameras, transforms, parameter blocks), element 0 constant."""
    from scipy.optimize import least_squares

    N = d["board"].shape[0]
    W = 18 + 6 * n
    blocks = [vgo.OdometryCost(errV, errW, lam, d["delta_q"][i], d["init_wheels"]) for i in range(n - 1)]
    free = np.ones(x0.size, dtype=bool)
    free[18:24] = False

    def full(z):
        x = x0.copy()
        x[free] = z
        return x

    def fun(z):
        x = full(z)
        r, _, _ = vgo.eval_dataset(0, [1, 1, 0], d["board"], d["corners"], x, 0, [6, 18, 12], [0, 6, 0], np.arange(n), want_jac=False)
        ro = [b.evaluate(x[18 + 6 * i:24 + 6 * i], x[24 + 6 * i:30 + 6 * i], x[W:W + 3])[0] for i, b in enumerate(blocks)]
        return np.concatenate([r.ravel()] + ro)

    def jac(z):
        x = full(z)
        _, ji, jm = vgo.eval_dataset(0, [1, 1, 0], d["board"], d["corners"], x, 0, [6, 18, 12], [0, 6, 0], np.arange(n), want_jac=True)
        J = np.zeros((2 * N * n + 6 * (n - 1), x.size))
        for b in range(n):
            rows = slice(b * 2 * N, (b + 1) * 2 * N)
            J[rows, 0:6] = ji[b]
            J[rows, 6:12] = jm[0][b]
            J[rows, 18 + 6 * b:24 + 6 * b] = jm[1][b]
            J[rows, 12:18] = jm[2][b]
        for i, blk in enumerate(blocks):
            _, J1, J2, J3 = blk.evaluate(x[18 + 6 * i:24 + 6 * i], x[24 + 6 * i:30 + 6 * i], x[W:W + 3])
            rows = slice(2 * N * n + 6 * i, 2 * N * n + 6 * i + 6)
            J[rows, 18 + 6 * i:24 + 6 * i] = J1
            J[rows, 24 + 6 * i:30 + 6 * i] = J2
            J[rows, W:W + 3] = J3
        return J[:, free]

    ref = least_squares(fun, x0[free], jac=jac, method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=500)
    return ref, full, fun, jac, free


def _wheeled_x0(d, n):
    seq = [np.zeros(6)]
    for i in range(n - 1):   # "init": true of the odometry_intrinsic entry: chain the priors (unified_calibration.cpp:724-730)
        seq.append(vgo.compose(seq[-1], vgo.OdometryCost(0.05, 0.05, 0.05, d["delta_q"][i], d["init_wheels"]).zeta))
    return np.concatenate([d["init_intrinsics"], d["init_xi_base_cam"], d["init_xi_odom_board"], np.concatenate(seq), d["init_wheels"]])


@pytest.mark.parametrize("lam", [0.05, 1.0])
def test_odometry_cost_matches_scipy_on_the_oracle(vg, lam):
    """data type "odometry_intrinsic" (unified_calibration.cpp:660-742): OdometryCost blocks (6, 6, 3) couple consecutive
    elements of the sequence AND a shared parameter block [radius_left, radius_right, track_gauge]: three more global
    columns, a pose-global coupling J_pose^T J_3 on top of the block-tridiagonal pose system."""
    from visgeom_amd import synthetic as S

    n = 12
    d = S.make_wheeled(n, sigma=0.1)
    errV, errW = 0.05, 0.05
    x0 = _wheeled_x0(d, n)
    ref, full, fun, jac, free = _wheeled_reference(d, n, errV, errW, lam, x0)

    p = vg.CalibrationProblem(0)
    cam = p.add_camera("eucm", d["init_intrinsics"])
    bc = p.add_transform(True, d["init_xi_base_cam"])
    ob = p.add_transform(True, d["init_xi_odom_board"])
    seq = p.add_transform(False, x0[18:18 + 6 * n].reshape(n, 6))
    wheels = p.add_parameter_block(d["init_wheels"])
    p.add_dataset(cam, [(bc, 1), (seq, 1), (ob, 0)], d["board"], d["corners"])
    for i in range(n - 1):
        p.add_odometry_cost(seq, i, errV, errW, lam, d["delta_q"][i], wheels)
    p.set_pose_constant(seq, 0)
    p.finalize()
    W = 18 + 6 * n
    assert p.parameter_block_offset(wheels) == W
    summ = p.solve(max_num_iterations=300, use_bounds=0)
    x = p.get_parameters()
    print("odometry cost lam=%g" % lam, summ["termination"], summ["num_iterations"],
          "cost gpu %.10e scipy %.10e (initial %.4e)" % (summ["final_cost"], ref.cost, summ["initial_cost"]), "wheels", x[W:], full(ref.x)[W:])
    assert summ["num_global_columns"] == 21
    assert np.array_equal(x[18:24], x0[18:24])                      # the anchor did not move
    assert abs(summ["initial_cost"] - 0.5 * np.sum(fun(x0[free]) ** 2)) <= 1e-10 * summ["initial_cost"]
    assert abs(summ["final_cost"] - 0.5 * np.sum(fun(x[free]) ** 2)) <= 1e-10 * summ["final_cost"]
    # the reference's odometry Jacobians are first-order approximations, so the comparison is solver-to-solver as in
    # the OdometryPrior case: gradient (by the reference's J) reduced, same cost, same optimum to solver tolerance
    g = jac(x[free]).T @ fun(x[free])
    g0 = jac(x0[free]).T @ fun(x0[free])
    assert np.max(np.abs(g)) <= 1e-5 * np.max(np.abs(g0))
    assert abs(summ["final_cost"] - ref.cost) <= 1e-5 * ref.cost
    # Planar motion leaves one gauge freedom: lifting the camera on the base by dz (xiBaseCam t_z, index 8) and the board in
    # the odometry frame by the same dz (xiOdomBoard t_z, index 14) changes no image.  Each solver stops somewhere else
    # along it, so those two are compared through their difference.
    xr = full(ref.x)
    keep = np.ones(W, dtype=bool)
    keep[[8, 14]] = False
    keep[:6] = False
    assert rel(x[:6], xr[:6]) < 1e-4
    assert np.max(np.abs(x[:W][keep] - xr[:W][keep])) < 1e-3
    assert abs((x[8] - x[14]) - (xr[8] - xr[14])) < 1e-3
    assert rel(x[W:], xr[W:]) < 1e-3
    # calibration sanity: wheel geometry and the observable part of the hand-eye transform recovered
    assert rel(x[W:], d["gt_wheels"]) < 2e-2
    obs = [6, 7, 9, 10, 11]
    assert np.max(np.abs(x[obs] - np.concatenate([d["gt_xi_base_cam"], []])[[0, 1, 3, 4, 5]])) < 1e-2
    p.close()


def test_constant_wheel_geometry_reduces_to_fixed_priors(vg):
    """A constant parameter block: its three global columns are frozen, the OdometryCost blocks act as odometry priors
    computed from the (fixed) wheel geometry."""
    from visgeom_amd import synthetic as S

    n = 8
    d = S.make_wheeled(n, sigma=0.1)
    x0 = _wheeled_x0(d, n)
    p = vg.CalibrationProblem(0)
    cam = p.add_camera("eucm", d["init_intrinsics"])
    bc = p.add_transform(True, d["init_xi_base_cam"])
    ob = p.add_transform(True, d["init_xi_odom_board"])
    seq = p.add_transform(False, x0[18:18 + 6 * n].reshape(n, 6))
    wheels = p.add_parameter_block(d["init_wheels"], constant=True)
    p.add_dataset(cam, [(bc, 1), (seq, 1), (ob, 0)], d["board"], d["corners"])
    for i in range(n - 1):
        p.add_odometry_cost(seq, i, 0.05, 0.05, 0.5, d["delta_q"][i], wheels)
    p.set_pose_constant(seq, 0)
    p.finalize()
    summ = p.solve(max_num_iterations=200, use_bounds=0)
    x = p.get_parameters()
    W = 18 + 6 * n
    assert np.array_equal(x[W:], d["init_wheels"])
    assert summ["final_cost"] < 1e-3 * summ["initial_cost"] and summ["termination"].startswith("CONVERGENCE")
    p.close()


def test_cached_solver_blocks_are_reused_and_released(vg):
    """vg_problem_solve works in one device block + one pinned block that the library keeps for the next solve
    (vg_release_cached_memory returns them): a solve after the release, a solve on the reused blocks and the first solve
    give the same answer bit for bit, a smaller problem fits the kept blocks, and the release really frees the memory."""
    import torch

    from visgeom_amd import capi, synthetic as S

    lib = capi.load()

    BIG = 20000   # large enough that the kept blocks (~150 MB) dwarf whatever the HIP runtime allocates for itself on the way
    data = {}

    def solve(n):
        d = data.setdefault(n, S.make_mono("eucm", n, 2, sigma=0.1))
        p, cam, seq, ds = mono_problem(vg, d, "eucm")
        s = p.solve(max_num_iterations=30)
        x = p.get_parameters()
        p.close()
        return s, x

    solve(300)                              # first use of the library in a process: code objects, runtime pools
    solve(BIG)
    lib.vg_release_cached_memory()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    s1, x1 = solve(BIG)                    # allocates the blocks
    free_kept, _ = torch.cuda.mem_get_info()
    s2, x2 = solve(BIG)                    # reuses them
    s3, x3 = solve(300)                     # a smaller problem fits
    s4, x4 = solve(BIG)
    assert free0 - free_kept > 64 << 20      # something is being kept (two Gram sets of 20 000 images alone are 54 MB)
    lib.vg_release_cached_memory()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < (free0 - free_kept) // 4, "the released blocks did not come back: %.1f of %.1f MiB" % (
        (free0 - free1) / 2**20, (free0 - free_kept) / 2**20)
    s5, x5 = solve(BIG)                    # allocates again
    for s, x in ((s2, x2), (s4, x4), (s5, x5)):
        assert np.array_equal(x, x1) and s["final_cost"] == s1["final_cost"] and s["num_iterations"] == s1["num_iterations"]
    assert s3["termination"].startswith("CONVERGENCE")
    lib.vg_release_cached_memory()
    lib.vg_release_cached_memory()          # idempotent


def test_soft_l1_loss_on_a_stereo_pair(vg):
    """The robust loss on a problem with SEVERAL datasets (the merged Gram launch, then the per-dataset re-weighting, then
    the slab sums -- the partial-sum shortcut must stay off): stereo pair, both cameras' intrinsics and the stereo
    transform free, poses constant, one image of camera 2 shifted by 20 px; against scipy's minimum of sum_b rho(|r_b|^2)
    over the oracle's residuals."""
    from scipy.optimize import least_squares

    from visgeom_amd import synthetic as S

    n, a = 10, 1.5
    st = S.make_stereo(n, sigma=0.1)
    c2 = st["corners2"].copy()
    c2[3] += np.array([20.0, 12.0])
    K = 6
    x0 = np.concatenate([st["init_intrinsics1"], st["init_intrinsics2"], st["init_xi12"], st["gt_poses"].ravel()])

    def blocks(z):
        x = x0.copy()
        x[:18] = z
        r1, _, _ = vgo.eval_dataset(0, [0], st["board"], st["corners1"], x, 0, [18], [6], np.arange(n), want_jac=False)
        r2, _, _ = vgo.eval_dataset(0, [1, 0], st["board"], c2, x, K, [12, 18], [0, 6], np.arange(n), want_jac=False)
        return np.concatenate([r1.reshape(n, -1), r2.reshape(n, -1)])

    def robust(z):
        r = blocks(z)
        s = np.sum(r * r, axis=1)
        rho = 2 * a * a * (np.sqrt(1 + s / (a * a)) - 1)
        return (r * np.sqrt(rho / s)[:, None]).ravel()

    ref = least_squares(robust, x0[:18], jac="3-point", x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=4000)
    p = vg.CalibrationProblem(0)
    cam1 = p.add_camera("eucm", st["init_intrinsics1"])
    cam2 = p.add_camera("eucm", st["init_intrinsics2"])
    x12 = p.add_transform(True, st["init_xi12"])
    seq = p.add_transform(False, st["gt_poses"], constant=True)
    p.add_dataset(cam1, [(seq, 0)], st["board"], st["corners1"])
    p.add_dataset(cam2, [(x12, 1), (seq, 0)], st["board"], c2)
    p.finalize()
    summ = p.solve(max_num_iterations=400, use_bounds=0, soft_l1_scale=a)
    z = p.get_parameters()[:18]
    p.close()
    print("soft-l1 stereo", summ["termination"], summ["num_iterations"], "cost %.8e scipy %.8e" % (summ["final_cost"], ref.cost))
    assert abs(summ["final_cost"] - ref.cost) <= 1e-8 * ref.cost
    assert rel(z[:12], ref.x[:12]) < 1e-5 and np.max(np.abs(z[12:] - ref.x[12:])) < 1e-6


@pytest.mark.parametrize("model", ["eucm", "mei"])
def test_iteration_limits_of_the_device_resident_loop(vg, model):
    """max_num_iterations = 0, 1, 2, 3 ... on the device-resident loop, which queues iteration k + 1 before it knows the
    outcome of iteration k: the limit must hold exactly (no queued iteration may slip in), the cost must be the one a longer
    run shows after the same number of iterations, and a run stopped by the limit can be continued to the same optimum."""
    from visgeom_amd import synthetic as S

    d = S.make_mono(model, 64, 2, sigma=0.1)
    x_start = None
    costs = []
    for k in range(0, 6):
        p, cam, seq, ds = mono_problem(vg, d, model)
        if x_start is None:
            x_start = p.get_parameters()
        s = p.solve(max_num_iterations=k)
        x = p.get_parameters()
        assert s["num_iterations"] == k, s
        if k == 0:
            assert np.array_equal(x, x_start) and s["final_cost"] == s["initial_cost"]
        assert s["termination"] in ("NO_CONVERGENCE",) or k >= 3, s
        costs.append(s["final_cost"])
        if k == 3:   # continue from where the limit stopped it
            s2 = p.solve(max_num_iterations=200)
            x2 = p.get_parameters()
            assert s2["termination"].startswith("CONVERGENCE") and abs(s2["initial_cost"] - s["final_cost"]) <= 1e-12 * s["final_cost"]
        p.close()
    assert all(b <= a for a, b in zip(costs, costs[1:])), costs
    q, _, _, _ = mono_problem(vg, d, model)
    sf = q.solve(max_num_iterations=200)
    xf = q.get_parameters()
    q.close()
    assert abs(s2["final_cost"] - sf["final_cost"]) <= 1e-10 * sf["final_cost"]
    assert np.max(np.abs(x2 - xf) / np.maximum(np.abs(xf), 1.0)) < 1e-7


@pytest.mark.parametrize("case", ["mono", "stereo_empty_second_dataset", "stereo_soft_l1"])
def test_host_driven_loop_equals_the_device_resident_loop(vg, case):
    """the host-driven loop (taken for wide systems, priors, odometry; forced here through the debug hook) delivers what
    the host reads through pinned memory written by the kernels themselves -- no copy commands: same iterates as the
    device-resident loop on a mono set, on a stereo pair whose second dataset is EMPTY (its slot of the sums is cleared by
    a memset on the pinned block) and with the SoftLOne loss (the re-weighting kernel runs between Gram and sums)"""
    from visgeom_amd import capi, synthetic as S

    def build():
        p = vg.CalibrationProblem(0)
        if case == "mono":
            d = S.make_mono("eucm", 300, 1)
            c = p.add_camera("eucm", d["init_intrinsics"])
            s = p.add_transform(False, d["init_poses"])
            p.add_dataset(c, [(s, 0)], d["board"], d["corners"])
        else:
            st = S.make_stereo(40, sigma=0.1)
            c1 = p.add_camera("eucm", st["init_intrinsics1"])
            c2 = p.add_camera("eucm", st["init_intrinsics2"], constant=(case == "stereo_empty_second_dataset"))
            x12 = p.add_transform(True, st["init_xi12"], constant=(case == "stereo_empty_second_dataset"))
            seq = p.add_transform(False, st["init_poses"])
            p.add_dataset(c1, [(seq, 0)], st["board"], st["corners1"])
            n2 = 0 if case == "stereo_empty_second_dataset" else 40
            p.add_dataset(c2, [(x12, 1), (seq, 0)], st["board"], st["corners2"][:n2], image_index=np.arange(n2, dtype=np.int32))
        p.finalize()
        return p

    kw = {"max_num_iterations": 60}
    if case == "stereo_soft_l1":
        kw["soft_l1_scale"] = 2.0
    out = []
    for host in (0, 1):
        capi.debug_set("solver_host_loop", host)
        try:
            p = build()
            s = p.solve(**kw)
            out.append((s, p.get_parameters()))
            p.close()
        finally:
            capi.debug_set("solver_host_loop", 0)
    (s_dev, x_dev), (s_host, x_host) = out
    assert s_dev["termination"].startswith("CONVERGENCE") and s_host["termination"].startswith("CONVERGENCE")
    assert abs(s_host["initial_cost"] - s_dev["initial_cost"]) <= 1e-13 * s_dev["initial_cost"]
    assert abs(s_host["final_cost"] - s_dev["final_cost"]) <= 1e-9 * s_dev["final_cost"]
    assert np.max(np.abs(x_host - x_dev) / np.maximum(np.abs(x_dev), 1.0)) < 1e-6


def test_wide_system_on_the_device_resident_loop(vg):
    """45 global columns (a four-camera rig) take the host-driven loop by default; forced onto the device-resident loop the
    reduced system is factorised by the entry-parallel one-workgroup kernel (vg_lm_reduced_solve_entries_kernel, 24 < G <=
    63): same optimum (iteration counts differ at the tail: with tolerances of 1e-15 the last accept / reject decisions hang
    on the last bits of the two loops' differently ordered sums)"""
    from tests.test_gpu_rig import build_rig
    from visgeom_amd import capi, synthetic as S

    r = S.make_rig(30, sigma=0.1)
    out = []
    for device in (0, 1):
        capi.debug_set("solver_device_loop", device)
        try:
            p, cams, x1k, seq, dss = build_rig(vg, r)
            s = p.solve(max_num_iterations=200)
            out.append((s, p.get_parameters()))
            p.close()
        finally:
            capi.debug_set("solver_device_loop", 0)
    (s_host, x_host), (s_dev, x_dev) = out
    assert s_host["num_global_columns"] == 45
    assert s_dev["termination"].startswith("CONVERGENCE") and s_host["termination"].startswith("CONVERGENCE")
    assert abs(s_host["final_cost"] - s_dev["final_cost"]) <= 1e-9 * s_dev["final_cost"]
    assert np.max(np.abs(x_host - x_dev) / np.maximum(np.abs(x_dev), 1.0)) < 1e-6


def test_tail_of_a_solve_ends_on_the_function_tolerance_within_ten_iterations(vg):
    """With the reference's tolerances of 1e-15 (unified_calibration.cpp:47-49) the last steps of a solve are rounding noise.
    Ceres tests |cost change| <= function_tolerance * cost on every evaluated candidate BEFORE the acceptance test; with that
    order a rejected noise-level step ends the solve within a radius reduction or two, and the iteration count no longer flips
    between 6 and 16 with the summation order of a kernel (round 4: two variants of the reduced solve inside the
    back-substitution launch)."""
    from visgeom_amd import synthetic as S

    d = S.make_mono("eucm", 1000, 1)
    p = mono_problem(vg, d, "eucm")[0]
    s = p.solve(max_num_iterations=100)
    p.close()
    assert s["termination"] == "CONVERGENCE_FUNCTION"
    assert s["num_iterations"] <= 10


def test_host_loop_waits_on_sequence_words_and_converges(vg):
    """The host-driven loop (here: a transformation prior forces it) learns of its two read-backs per iteration from pinned
    sequence words (a counter in the strided sum's last workgroup, a one-thread kernel behind the evaluation) instead of
    hipStreamSynchronize."""
    from visgeom_amd import synthetic as S

    st = S.make_stereo(60)
    p = vg.CalibrationProblem(0)
    c1 = p.add_camera("eucm", st["init_intrinsics1"])
    c2 = p.add_camera("eucm", st["init_intrinsics2"])
    x12 = p.add_transform(True, st["init_xi12"])
    seq = p.add_transform(False, st["init_poses"])
    p.add_dataset(c1, [(seq, 0)], st["board"], st["corners1"])
    p.add_dataset(c2, [(x12, 1), (seq, 0)], st["board"], st["corners2"])
    p.add_transformation_prior(x12, np.full(6, 0.5))
    p.finalize()
    s = p.solve(max_num_iterations=60)
    p.close()
    assert s["termination"].startswith("CONVERGENCE")
