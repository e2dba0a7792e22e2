"""Kannala-Brandt and double-sphere cameras, the part that needs no GPU: the numpy reference of tests/camera_models_ref.py against
its 50-digit restatement (whose Jacobians are numerical derivatives of the projection: this checks the closed forms), the model
queries, the host-side reconstruction and pose initialisation, the JSON front end, the entries that refuse the new models, and
the synthetic generator's unchanged output for the three models it had."""
import ctypes
import json
import os

import mpmath as mp
import numpy as np
import pytest

from tests import camera_models_ref as ref

TOL = 1e-12
MODEL_ID = {"kb": 4, "ds": 5}
_dp = ctypes.POINTER(ctypes.c_double)


def _ptr(a):
    return a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def S():
    from visgeom_amd import synthetic

    return synthetic


@pytest.fixture(scope="module")
def L():
    from visgeom_amd import capi

    return capi.load()


def params_of(S, model):
    """the synthetic ground truth and one perturbed set"""
    gt = S.GT[model]
    if model == "kb":
        return [gt, gt + np.array([0.02, -0.006, 0.002, -0.0003, 11.0, -7.0, 5.0, -3.0])]
    return [gt, gt + np.array([0.25, -0.17, 9.0, -6.0, 4.0, -2.0])]


KB_FOLDED = np.array([-0.4, 0.0, 0.0, 0.0, 380.0, 375.0, 640.0, 400.0])   # d' = 1 - 1.2 theta^2 = 0 at theta = 0.9129


def point_groups(model, p):
    """name -> [n, 3] camera-frame points"""
    rng = np.random.default_rng(20261021)
    g = {}
    X = rng.uniform(-1, 1, (12, 3))
    X[:, 2] = rng.uniform(0.3, 2.0, 12)
    g["generic"] = X
    g["axis"] = np.array([[0, 0, 1.0], [0, 0, 0.37], [0, 0, 25.0], [0, 0, -1.0], [0, 0, 0.0]])
    # r / z from 1e-18 to 1e-3: both sides of the on-axis threshold (1e-15) and the decades above it
    ratios = [1e-18, 1e-16, 0.99e-15, 1.01e-15, 1e-14] + [10.0 ** -k for k in range(12, 2, -1)]
    g["near_axis"] = np.array([[q * 0.8 * z, -q * 0.6 * z, z] for q, z in zip(ratios, np.linspace(0.4, 3.0, len(ratios)))])
    g["near_axis_one_coordinate"] = np.array([[q, 0.0, 1.0] for q in ratios] + [[0.0, -q, 2.0] for q in ratios])
    e = 1e-9
    g["around_half_pi"] = np.array([[0.6, 0.8, e], [0.6, 0.8, -e], [-0.3, 0.4, 1e-3], [-0.3, 0.4, -1e-3], [1.0, 0.0, 0.0]])
    g["behind"] = np.array([[0.5, -0.2, -0.1], [0.3, 0.4, -0.5], [-0.7, 0.1, -0.25]])
    if model == "ds":
        xi, al = p[0], p[1]
        w1 = al / (1 - al) if al <= 0.5 else (1 - al) / al
        w2 = (w1 + xi) / np.sqrt(2 * w1 * xi + xi * xi + 1)
        rows = []
        for az in (0.3, 2.1, 4.4):
            for eps in (-1e-3, -1e-9, 1e-9, 1e-3):   # cos(angle to the axis) = -w2 + eps: inside for eps > 0
                cz = -w2 + eps
                sr = np.sqrt(1 - cz * cz)
                rows.append(1.7 * np.array([sr * np.cos(az), sr * np.sin(az), cz]))
        g["ds_boundary"] = np.array(rows)
    return g


def close(got, ref_mp, what, floor_rel=1e-3):
    """SURVEY 8(c) metric at 1e-12, the comparison itself in 50 digits (as tests/test_oracle_mpmath.py)"""
    got = np.asarray(got, float)
    flat = list(ref_mp)
    refn = np.array([float(x) for x in flat]).reshape(got.shape)
    diff = np.array([float(mp.mpf(float(g)) - r) for g, r in zip(got.ravel(), flat)]).reshape(got.shape)
    nrm = np.linalg.norm(refn)
    if nrm == 0:
        assert np.all(got == 0), what
        return 0.0
    e1 = np.linalg.norm(diff) / nrm
    e2 = np.max(np.abs(diff) / np.maximum(np.abs(refn), floor_rel * np.max(np.abs(refn))))
    assert e1 <= TOL and e2 <= TOL, "%s: normwise %.2e elementwise %.2e" % (what, e1, e2)
    return max(e1, e2)


def check_group(model, p, X, what):
    uv, ok = ref.project(model, p, X)
    P = ref.projection_jacobian(model, p, X)
    J = ref.intrinsic_jacobian(model, p, X)
    mp_uv = [ref.mp_project(model, p, x) for x in X]
    assert [m is not None for m in mp_uv] == list(ok), "%s: failure flags differ" % what
    assert np.all(P[~ok] == 0) and np.all(J[~ok] == 0)
    for i in np.nonzero(ok)[0]:   # one point = one block of the metric: no point hides behind another's large entries
        mP, mJ = ref.mp_jacobians(model, p, X[i])
        # residual metric: |du| against the projection's norm and against max(|r|, 1 px) -- here with r = the projection itself
        close(uv[i], mp_uv[i], "%s point %d uv" % (what, i), floor_rel=0.)
        close(P[i], mP[0] + mP[1], "%s point %d d/dX" % (what, i))
        close(J[i], mJ[0] + mJ[1], "%s point %d d/dintrinsics" % (what, i))
    return ok


@pytest.mark.parametrize("model", ["kb", "ds"])
def test_numpy_reference_against_50_digits(S, model):
    n_fail = 0
    for k, p in enumerate(params_of(S, model)):
        for name, X in point_groups(model, p).items():
            ok = check_group(model, p, X, "%s set %d %s" % (model, k, name))
            n_fail += int((~ok).sum())
            if name == "axis":
                assert list(ok) == [True, True, True, False, False]
            if name == "behind" and model == "kb":
                assert ok.all()   # behind the camera with r > 0 is inside the Kannala-Brandt image
            if name == "ds_boundary":
                assert list(ok) == [False, False, True, True] * 3
            if name == "near_axis":
                assert ok.all()
    assert n_fail > 0


def test_kannala_brandt_fold_over_fails_in_both():
    """d' crosses zero at theta = 0.9129 for k1 = -0.4: points on both sides of it, in numpy and in 50 digits"""
    th = np.array([0.2, 0.7, 0.91, 0.9128, 0.9130, 0.92, 1.2, 2.0])
    X = np.stack([np.sin(th) * 0.6, np.sin(th) * -0.8, np.cos(th)], -1) * 1.3
    ok = check_group("kb", KB_FOLDED, X, "folded")
    assert list(ok) == [True, True, True, True, False, False, False, False]


@pytest.mark.parametrize("model", ["kb", "ds"])
def test_unprojection_inverts_the_projection_in_both(S, model):
    rng = np.random.default_rng(7)
    for p in params_of(S, model):
        X = rng.standard_normal((40, 3))
        X[:, 2] = np.abs(X[:, 2]) + 0.05
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        uv, ok = ref.project(model, p, X)
        assert ok.all()
        ray, ok2 = ref.unproject(model, p, uv)
        assert ok2.all()
        ray /= np.linalg.norm(ray, axis=1, keepdims=True)
        assert np.max(np.linalg.norm(ray - X, axis=1)) <= 1e-12
        for i in range(0, 40, 8):
            m = ref.mp_unproject(model, p, uv[i])
            assert max(abs(float(mp.mpf(float(ray[i, c])) - m[c])) for c in range(3)) <= 1e-12


# ------------------------------------------------------------------------------------------ the library, host side
def test_model_queries(L):
    from visgeom_amd import capi

    assert capi.MODELS["kb"] == 4 and capi.MODELS["ds"] == 5
    assert capi.NUM_INTRINSICS[4] == 8 and capi.NUM_INTRINSICS[5] == 6
    assert [L.vg_num_intrinsics(m) for m in (4, 5, 3)] == [8, 6, -1]
    assert L.vg_abi_version() == 1
    lo, hi = ctypes.c_double(), ctypes.c_double()
    want = {4: [(-10., 10.)] * 4 + [(1., 1e5)] * 4, 5: [(-0.9, 3.), (0., 1.)] + [(1., 1e5)] * 4}
    for m, bounds in want.items():
        for i, b in enumerate(bounds):
            assert L.vg_intrinsic_bounds(m, i, ctypes.byref(lo), ctypes.byref(hi)) == 0
            assert (lo.value, hi.value) == b, (m, i)
        assert L.vg_intrinsic_bounds(m, len(bounds), ctypes.byref(lo), ctypes.byref(hi)) == capi.ERR_INVALID_ARGUMENT
    assert L.vg_intrinsic_bounds(3, 0, ctypes.byref(lo), ctypes.byref(hi)) == capi.ERR_INVALID_ARGUMENT


def _reconstruct(L, model, p, uv):
    p, uv, X = np.ascontiguousarray(p, float), np.ascontiguousarray(uv, float), np.full(3, np.nan)
    rc = L.vg_reconstruct_point(MODEL_ID[model], _ptr(p), _ptr(uv), _ptr(X))
    return rc, X


@pytest.mark.parametrize("model", ["kb", "ds"])
def test_reconstruct_point_against_50_digits_and_round_trip(S, L, model):
    from visgeom_amd import capi

    rng = np.random.default_rng(11)
    for p in params_of(S, model):
        uvs = np.concatenate([np.stack([rng.uniform(0, S.IMAGE_W, 30), rng.uniform(0, S.IMAGE_H, 30)], -1),
                              [[p[-2], p[-1]], [p[-2] + 1e-9, p[-1]], [0., 0.], [S.IMAGE_W, S.IMAGE_H]]])
        for uv in uvs:
            rc, X = _reconstruct(L, model, p, uv)
            m = ref.mp_unproject(model, p, uv)
            assert (rc == 0) == (m is not None)
            if m is None:
                continue
            n = mp.sqrt(sum(mp.mpf(float(c)) ** 2 for c in X))
            assert max(abs(float(mp.mpf(float(X[c])) / n - m[c])) for c in range(3)) <= 1e-12, (model, uv)
            back, ok = ref.project(model, p, X[None, :])
            assert ok[0] and np.max(np.abs(back[0] - uv)) <= 1e-9 * max(S.IMAGE_W, S.IMAGE_H)
    if model == "ds":   # alpha > 0.5: pixels outside r^2 <= 1 / (2 alpha - 1) have no ray
        p = np.array([-0.2, 0.8, 245.6, 231.6, 642.617, 398.42])
        rc, _ = _reconstruct(L, model, p, [642.617 + 245.6 * 1.30, 398.42])   # r^2 = 1.69 > 1 / 0.6
        assert rc == capi.ERR_NUMERIC
        rc, _ = _reconstruct(L, model, p, [642.617 + 245.6 * 1.28, 398.42])   # r^2 = 1.6384 < 1.6667
        assert rc == 0
    else:           # the folded polynomial: image radii past its maximum d(0.9129) = 0.6086 have no ray
        rc, _ = _reconstruct(L, model, KB_FOLDED, [640.0 + 380.0 * 0.62, 400.0])
        assert rc == capi.ERR_NUMERIC
        rc, X = _reconstruct(L, model, KB_FOLDED, [640.0 + 380.0 * 0.60, 400.0])
        assert rc == 0 and ref.mp_unproject(model, KB_FOLDED, [640.0 + 380.0 * 0.60, 400.0]) is not None


@pytest.mark.parametrize("model", ["kb", "ds"])
def test_initial_grid_pose(S, L, model):
    """the cone and range test tests/test_pose_init_cpu.py applies to EUCM: at the generating intrinsics and noise-free corners the
    translation is the UL corner's viewing ray (exact: cosine within 1e-9) times a range within [0.6, 1.4] of the true one, and the
    rotation is a starting value (Frobenius distance below 0.8)"""
    from visgeom_amd import capi

    d = S.make_mono(model, 60, 2, sigma=0.0)
    N = d["board"].shape[0]
    idx = [0, S.BOARD_COLS - 1, N - S.BOARD_COLS, N - 1]
    b4 = np.ascontiguousarray(d["board"][idx])
    intr = np.ascontiguousarray(d["gt_intrinsics"])
    worst = 0.0
    for i in range(60):
        c4, xi = np.ascontiguousarray(d["corners"][i][idx]), np.full(6, np.nan)
        assert L.vg_initial_grid_pose(MODEL_ID[model], _ptr(intr), _ptr(b4), _ptr(c4), _ptr(xi)) == 0
        R = S.rodrigues(d["gt_poses"][i][3:])
        ul_cam = R @ d["board"][idx[0]] + d["gt_poses"][i][:3]
        cosang = xi[:3] @ ul_cam / (np.linalg.norm(xi[:3]) * np.linalg.norm(ul_cam))
        assert cosang > 1 - 1e-9 and 0.6 < np.linalg.norm(xi[:3]) / np.linalg.norm(ul_cam) < 1.4, (model, i)
        worst = max(worst, np.linalg.norm(S.rodrigues(xi[3:]) - R))
    assert worst < 0.8


@pytest.mark.parametrize("model", ["kb", "ds"])
def test_frontend_parses_the_new_cameras(S, tmp_path, model):
    from visgeom_amd import capi
    from visgeom_amd.calibration import GenericCameraCalibration

    d = S.make_mono(model, 5, 0)
    path = S.write_calibration_json(str(tmp_path), d, model, prior=True)   # the route of tests/test_frontend_cpu.py: no GPU
    c = GenericCameraCalibration()
    assert c.addResiduals(path)
    assert c.num_datasets() == 1
    got = c.intrinsics("cam")
    assert len(got) == ref.K_OF[model] and np.array_equal(got, d["init_intrinsics"])
    assert "Model : %s\n" % model.upper() in c.log()
    c.close()
    root = json.load(open(path))
    root["cameras"][0]["value"] = root["cameras"][0]["value"][:-1]
    json.dump(root, open(path, "w"))
    c = GenericCameraCalibration()
    with pytest.raises(capi.VisgeomError) as e:
        c.addResiduals(path)
    assert "invalid number of intrinsic parameters" in str(e.value)
    c.close()


@pytest.mark.parametrize("m", [4, 5])
def test_localization_and_trajectory_entries_refuse_the_new_models(L, m):
    """they are instantiated for EUCM / UCM / Mei (trajectory planning: EUCM) only, and say so before HIP is touched: this test has no GPU"""
    from visgeom_amd import capi

    intr, xb = np.ones(10), np.zeros(6)
    out = ctypes.c_void_p()
    x1, p2 = np.ones((5, 3)), np.ones((5, 2))
    assert L.vg_mono_reproject_create(ctypes.byref(out), 0, None, m, _ptr(intr), _ptr(xb), 1, _ptr(x1), _ptr(p2)) == capi.ERR_INVALID_ARGUMENT
    assert not out.value
    off, size = np.array([0, 5], dtype=np.int64), np.ones(5)
    assert L.vg_sparse_reproject_create(ctypes.byref(out), 0, None, m, _ptr(intr), _ptr(xb), 1, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                        _ptr(x1), _ptr(x1), _ptr(p2), _ptr(size)) == capi.ERR_INVALID_ARGUMENT
    assert not out.value
    T12, X2, J = np.zeros(6), np.ones((4, 3)), np.zeros((4, 12))
    assert L.vg_camera_jacobian_evaluate(0, None, m, _ptr(intr), _ptr(T12), None, 4, _ptr(X2), None, _ptr(J), None) == capi.ERR_INVALID_ARGUMENT
    assert "EUCM, UCM and Mei only" in L.vg_last_error().decode()
    q = capi.TrajectoryQuality()
    steps = (ctypes.c_int * 1)(4)
    assert L.vg_trajectory_create(ctypes.byref(out), 0, None, m, _ptr(intr), 1280, 800, ctypes.byref(q), 1, steps) == capi.ERR_INVALID_ARGUMENT
    assert not out.value
    uv, ok = np.zeros((96, 2)), np.zeros(96, dtype=np.int32)
    assert L.vg_trajectory_project_board(m, _ptr(intr), ctypes.byref(q), _ptr(xb), _ptr(uv), ok.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == capi.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("model", ["eucm", "ucm", "mei"])
def test_synthetic_sets_of_the_old_models_are_unchanged(S, golden_dir, model):
    """bit for bit against arrays stored before the generator learned the new models (bench.py and the suite generate from it)"""
    want = np.load(os.path.join(golden_dir, "synthetic_mono_%s_5_3.npz" % model))
    d = S.make_mono(model, 5, 3)
    assert sorted(want.files) == sorted(k for k, v in d.items() if isinstance(v, np.ndarray))
    for k in want.files:
        assert d[k].dtype == want[k].dtype and np.array_equal(d[k], want[k]), k


@pytest.mark.parametrize("model", ["kb", "ds"])
def test_synthetic_ground_truths_pass_the_pose_sampler(S, model):
    d = S.make_mono(model, 16, 2, sigma=0.0)
    uv, ok = ref.project(model, d["gt_intrinsics"], (np.einsum("nij,kj->nki", S.rodrigues(d["gt_poses"][:, 3:]), d["board"])
                                                     + d["gt_poses"][:, None, :3]).reshape(-1, 3))
    assert ok.all() and np.max(np.abs(uv.reshape(d["corners"].shape) - d["corners"])) <= 1e-9
    assert d["init_intrinsics"].size == ref.K_OF[model]
