"""The conditions the inputs of tests/trajectory_shapes.py have to meet for tests/test_gpu_trajectory_shapes.py to test what it
says, asserted on the restatement alone (tests/trajectory_ref.py): validity, the penalties that are active, the share of the
cell sizes, the block arithmetic, the condition numbers behind the bound on cov, and the restatement's own float64 /
long-double spread, which has to stay 100 times under the GPU bar of 1e-10 max(1, |ref|).  And, through the C ABI without a
device, that every shape used is accepted.  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import trajectory_shapes as ts

SPREAD = 1e-12     # of every compared quantity, relative to max(1, |ref|)


def check_spread(name, ref):
    s = ts.spread(ref)
    print("%s: cost %.10g terms %s, float64 / long double spread %.3g" % (name, float(ref["ld"][0]), [float(v) for v in ref["ld"][1]], s))
    assert s < SPREAD, name


def active(ref, names):
    """the penalties in `names` are above 1, the others exactly 0"""
    for k, name in enumerate(ts.TERMS[1:]):
        v = float(ref["ld"][1][1 + k])
        assert (v > 1.) if name in names else (v == 0.), (name, v)


def test_a_many_trajectories():
    assert len(ts.A_STEPS) == 8 and sum(n - 1 for n in ts.A_STEPS) == 18
    assert [n for n in ts.A_STEPS].count(2) >= 4 and ts.A_STEPS[:2] == [2, 2]   # single-slot trajectories, two adjacent at the front
    p = ts.a_params()
    assert p.shape == (40,) and p[19] == -0.25 and p[37] == ts.A_THETA_LAST
    plan, tilted = ts.reference("plan", ts.A_STEPS, p), ts.reference("tilted", ts.A_STEPS, p)
    for name, ref in (("A plan", plan), ("A tilted", tilted)):
        assert ref["ld"][2] == 0 and ref["f64"][2] == 0
        check_spread(name, ref)
    active(plan, ("image_limits", "curvature"))
    active(tilted, ("image_limits", "curvature", "distance", "normal"))
    # the image limits come from trajectory 8 (slots 15 .. 17, the last three) and the curvature from trajectories 1 and 4
    for ref in (plan, tilted):
        limits = [float(pose["penalties"][0]) for pose in ref["poses"]]
        assert sum(limits[15:]) > 1. and [k for k, pose in enumerate(ref["poses"]) if pose["penalties"][1] > 1.] == [0, 4]
    assert abs(float(plan["ld"][0]) - 154.71) < 0.01 and abs(float(plan["ld"][1][2]) - 183.56) < 0.01
    assert abs(float(tilted["ld"][1][3]) - 12.12) < 0.01 and abs(float(tilted["ld"][1][4]) - 25.99) < 0.01


def test_a_invalid_poses_are_in_the_middle():
    """slots 11 and 12: the last two of the 8 evaluated poses of trajectory 5 (slots 5 .. 12), with the 5 slots of trajectories 6,
    7 and 8 valid behind them; the penalties of the valid poses are finite and compared on the GPU"""
    p = ts.a_params(invalid=True)
    assert p[24] == -0.3 and np.array_equal(np.delete(p, 24), np.delete(ts.a_params(), 24))
    ref = ts.reference("plan", ts.A_STEPS, p)
    bad = [k for k, pose in enumerate(ref["poses"]) if not pose["valid"]]
    assert bad == ts.A_INVALID_SLOTS and ref["ld"][2] == ref["f64"][2] == 2
    slot0 = np.concatenate([[0], np.cumsum([n - 1 for n in ts.A_STEPS])])
    assert slot0[4] <= bad[0] and bad[1] < slot0[5] and slot0[5] + 5 == slot0[8] == len(ref["poses"]) == 18
    assert float(ref["ld"][0]) == np.inf and float(ref["ld"][1][0]) == np.inf and np.isfinite(np.asarray(ref["ld"][1][1:], float)).all()
    check_spread("A-invalid", ref)


def test_a_gradient_spread():
    """the long-double gradient the GPU test compares with: the float64 restatement is itself within the GPU bound of it"""
    g = ts.gradient_reference("plan", ts.A_STEPS, ts.a_params())
    cost = float(ts.reference("plan", ts.A_STEPS, ts.a_params())["ld"][0])
    bound = 64 * ts.EPS * max(1., abs(cost)) / g["delta"]
    d = np.abs(np.asarray(g["f64"], float) - np.asarray(g["ld"], float))
    print("gradient of A: the float64 restatement's largest |d| / bound %.3g" % (d / bound).max())
    assert g["delta"].shape == (40,) and np.isfinite(np.asarray(g["ld"], float)).all() and (d <= bound).all()


def test_b_long_trajectories():
    b1 = ts.reference("plan", ts.B1_STEPS, ts.B1_PARAMS)
    b8 = ts.reference("plan", ts.B8_STEPS, ts.b8_params())
    assert ts.b8_params().shape == (40,) and sum(n - 1 for n in ts.B8_STEPS) == 2040
    for name, ref in (("B [256, 2]", b1), ("B [256] * 8", b8)):
        assert ref["ld"][2] == 0 and ref["f64"][2] == 0
        check_spread(name, ref)
    active(b1, ("image_limits",))
    active(b8, ("image_limits",))
    assert abs(float(b1["ld"][0]) + 19.95) < 0.01 and abs(float(b1["ld"][1][1]) - 24.19) < 0.01 and abs(float(b8["ld"][0]) + 30.46) < 0.01
    batch = ts.b1_batch()
    assert batch.shape == (33, 10) and (batch[0::2] == np.asarray(ts.B1_PARAMS)).all() and (batch[1::2, :5] == batch[0, :5]).all()
    assert (batch[1::2, 5:] != batch[0, 5:]).all()


@pytest.mark.parametrize("board", ts.BOARDS)
def test_c_boards(board):
    """every pose valid in both settings; the cell sizes carry all of the image-limits term except on the 2 x 2 board, which has
    none; cond(JtCJ) leaves the bound on cov below 1e-6"""
    cols, rows, _ = board
    assert 4 <= cols * rows <= 1024
    for setting in ts.SETTINGS:
        ref = ts.reference(setting, ts.C_STEPS, ts.C_PARAMS, board)
        assert ref["ld"][2] == 0 and ref["f64"][2] == 0
        check_spread("C %s %s" % (board, setting), ref)
        whole, cells = ts.cell_share(setting, board)
        print("C %s %s: image limits %.6g, of which the cell sizes %.6g" % (board, setting, whole, cells))
        if (cols, rows) == (2, 2):
            assert whole == 0. and cells == 0.
        else:
            assert whole > 1. and cells == whole
        names = (() if (cols, rows) == (2, 2) else ("image_limits",)) + (("distance", "normal") if setting == "tilted" else ())
        active(ref, names)
    if (cols, rows) == (32, 32):
        assert abs(ts.cell_share("plan", board)[0] - 3086.) < 1.
    poses, covs = ts.cov_reference(board)
    assert poses.shape == (3, 6)
    for k, row in enumerate(covs):
        assert row["ld"][3] and row["f64"][3]
        V, V64, J, J64 = [np.asarray(a, float) for a in (row["ld"][0], row["f64"][0], row["ld"][1], row["f64"][1])]
        s_info, s_cov, bound = np.linalg.norm(J64 - J) / np.linalg.norm(J), np.linalg.norm(V64 - V) / np.linalg.norm(V), 64 * ts.EPS * row["cond"]
        print("C %s pose %d: cond(JtCJ) %.3g, spread of info %.3g, of cov %.3g of the bound %.3g" % (board, k, row["cond"], s_info, s_cov, bound))
        assert row["cond"] < ts.COND_MAX
        assert s_info < SPREAD and s_cov <= bound


def test_c_boards_cover_the_passes():
    """corners: 16 full passes of 64, a partial last one, one lane in the second, two full; cells: 31 passes at the cap"""
    n = {b: b[0] * b[1] for b in ts.BOARDS}
    assert n[ts.BOARDS[0]] == 1024 and n[ts.BOARDS[1]] == 1023 and ts.BOARDS[1][1] > ts.BOARDS[1][0]
    assert n[(13, 5, 0.06)] == 65 and n[(16, 8, 0.05)] == 128 and n[(2, 2, 0.5)] == 4
    cells = lambda c, r: (c - 1) * r + c * (r - 1)   # noqa: E731
    assert ts.blocks_of(cells(32, 32)) == 31 and 16 * 1024 == 16384
    assert cells(2, 33) == 33 + 2 * 32 and cells(33, 2) == cells(2, 33)


def test_d_batches():
    pts = ts.d_points()
    assert pts.shape == (130, 15) and np.array_equal(ts.d_start()[:10], ts.plan()["start"])
    Q = ts.quality("plan", ts.D_STEPS)
    res = [Q.evaluate(p) for p in pts]
    assert all(r[2] == 0 for r in res) and len(set(float(r[0]) for r in res)) == 130
    # the prepass takes items 3 k .. 3 k + 2 of point k: 21 sits on items 63, 64, 65 and 42 on 126, 127, 128
    assert ts.straddlers(130, 3) == [21, 42, 85, 106]   # item 192 = 3 * 64 begins both a point and a block
    assert ts.blocks_of(130 * 3) == 7 and ts.blocks_of(130) == 3
    assert ts.blocks_of(ts.D_CHUNK * 3) == 1 and ts.blocks_of(ts.D_CHUNK) == 1   # the chunks stay in one wave
    assert set(ts.D_CHECKED) >= {0, 21, 42, 63, 64, 65, 129}
    for k in ts.D_CHECKED:
        check_spread("D point %d" % k, ts.reference("plan", ts.D_STEPS, pts[k]))
    assert ts.blocks_of(5 * 31) == 3 and 5 * 31 == 155   # the gradient of 5 points


def test_e_the_cap():
    pts = ts.e_points()
    assert pts.shape == (65535, 5) and all((pts[k::3] == np.asarray(ts.E_THREE[k])).all() for k in range(3))
    refs = [ts.reference("plan", ts.E_STEPS, p, ts.E_BOARD) for p in ts.E_THREE]
    for k, ref in enumerate(refs):
        assert ref["ld"][2] == 0
        check_spread("E point %d" % k, ref)
    active(refs[0], ())
    active(refs[1], ("curvature",))
    active(refs[2], ())
    assert abs(float(refs[1]["ld"][1][2]) - 100.) < 1e-9
    assert [round(float(r["ld"][0]), 2) for r in refs] == [-27.73, 72.25, -27.66]
    n_poses, n_slots = 2, 1
    scratch = 65535 * 8 * (5 + 6 * n_poses + 36 * n_poses + 36 * n_slots + 4 * n_slots + 1 + 5) + 65535 * 4 * (n_slots + 1)
    print("device scratch at the cap: %.1f MB" % (scratch / 1e6))
    assert scratch < 100e6
    assert 5958 * 11 == 65538 > 65535 >= 5957 * 11   # the largest gradient batch of P = 5


def test_f_starts():
    starts = ts.f_starts()
    assert starts.shape == (7, 10)
    for k, p in enumerate(starts):
        ref = ts.reference("plan", ts.plan()["steps"], p)
        assert ref["ld"][2] == 0
        check_spread("F start %d" % k, ref)
    assert 7 * 21 == 147 and ts.blocks_of(147) == 3 and ts.blocks_of(147 * 2) == 5


def test_create_accepts_every_shape_used():
    """through the C ABI without a device: every (steps, board) of the cases passes the argument checks and fails only for want of
    a device"""
    import torch

    from visgeom_amd import _build, capi, trajectory

    _build.build()
    lib = capi.load()
    p = ts.plan()
    cam = np.array(p["cam"], dtype=np.float64)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    shapes = [(ts.A_STEPS, None), (ts.B1_STEPS, None), (ts.B8_STEPS, None), (ts.D_STEPS, None), (ts.E_STEPS, ts.E_BOARD), (p["steps"], None)]
    shapes += [(ts.C_STEPS, b) for b in ts.BOARDS]
    for steps, board in shapes:
        for setting in ts.SETTINGS:
            q = trajectory.make_quality(ts.quality_parameters(setting, board))
            s = np.array(steps, dtype=np.intc)
            h = ctypes.c_void_p()
            rc = lib.vg_trajectory_create(ctypes.byref(h), 0, None, capi.MODEL_EUCM, cam.ctypes.data_as(dp), p["w"], p["h"], ctypes.byref(q), s.size,
                                          s.ctypes.data_as(ip))
            assert rc == capi.ERR_NO_DEVICE and not h.value, (steps, board, setting, rc, lib.vg_last_error())
