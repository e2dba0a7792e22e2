"""The problems of tests/test_gpu_lm_steps.py, described once as cases of tests/oracle_lm.py (so that the CPU tests can check
what the reference does on them: which steps are rejected, which columns are held) and built on the HIP path.  Inputs from
the seeded generator (visgeom_amd/synthetic.py); start points moved away from the generator's initial values where a
case needs large steps or a rejected first step."""
import numpy as np

from tests import golden_cases as G


def _mono(model, n, seed=2, gt=None, scale=None):
    from visgeom_amd import synthetic as S

    d = S.make_mono(model, n, seed, gt=gt)
    intr = np.array(d["init_intrinsics"], float)
    if scale is not None:
        intr = intr * np.asarray(scale, float)
    return {"cameras": [(model, intr)], "transforms": [(False, d["init_poses"])],
            "datasets": [(0, [(0, 0)], d["board"], d["corners"])]}


def _stereo(n, missing=(), unobserved=()):
    """config 3 with cam-2 frames `missing` and pose elements `unobserved` (seen by neither camera)"""
    from visgeom_amd import synthetic as S

    s = S.make_stereo(n)
    k1 = np.array([i for i in range(n) if i not in unobserved], dtype=np.int64)
    k2 = np.array([i for i in range(n) if i not in unobserved and i not in missing], dtype=np.int64)
    return {"cameras": [("eucm", s["init_intrinsics1"]), ("eucm", s["init_intrinsics2"])],
            "transforms": [(True, s["init_xi12"][None, :]), (False, s["init_poses"])],
            "datasets": [(0, [(1, 0)], s["board"], s["corners1"][k1], k1), (1, [(0, 1), (1, 0)], s["board"], s["corners2"][k2], k2)]}


def _wide_rig(n_cam, n_frames=40):
    """n_cam Mei cameras on one rig (tests/test_gpu_rig.py): G = 10 n_cam + 6 (n_cam - 1), noise-free corners"""
    from visgeom_amd import synthetic as S

    board = S.board_points()
    gts = [S.GT_MEI * (1 + 0.002 * k * np.array([1, 0, 0, 0, 0, 0, 1, 1, 0.2, 0.2])) for k in range(n_cam)]
    xi1k = [np.array([0.06 * (k % 4), 0.06 * (k // 4), 0.0, 0.004 * k, -0.003 * k, 0.002 * k]) for k in range(1, n_cam)]
    cams = [("mei", gts[0], np.eye(3), np.zeros(3))]
    for k in range(n_cam - 1):
        R = S.rodrigues(xi1k[k][3:])
        cams.append(("mei", gts[k + 1], R.T, -R.T @ xi1k[k][:3]))
    poses = S.make_poses(S.BASE_SEED + 11, n_frames, cams, board)
    X1 = np.einsum("nij,kj->nki", S.rodrigues(poses[:, 3:]), board) + poses[:, None, :3]
    ds = []
    for k, (m, intr, Rc, tc) in enumerate(cams):
        uv, ok = S.project(m, intr, np.einsum("ij,nkj->nki", Rc, X1) + tc)
        assert ok.all()
        ds.append((k, [(n_cam - 1, 0)] if k == 0 else [(k - 1, 1), (n_cam - 1, 0)], board, uv))
    return {"cameras": [("mei", S.INIT["mei"]) for _ in range(n_cam)],
            "transforms": [(True, (x + 0.004)[None, :]) for x in xi1k] + [(False, poses + 0.005)], "datasets": ds}


def _rig(models, view_cam, n_frames=40):
    """a rig of views (view k sees the board through camera view_cam[k]; views 1.. through a global transform each, the
    same camera may serve several views): G = sum of the cameras' intrinsics + 6 (views - 1), noise-free corners"""
    from visgeom_amd import synthetic as S

    board = S.board_points()
    gts = [S.GT[m] * (1 + 0.002 * k) for k, m in enumerate(models)]
    V = len(view_cam)
    xi1k = [np.array([0.05 * (k % 4), 0.05 * (k // 4), 0.0, 0.004 * k, -0.003 * k, 0.002 * k]) for k in range(1, V)]
    views = [(models[view_cam[0]], gts[view_cam[0]], np.eye(3), np.zeros(3))]
    for k in range(V - 1):
        R = S.rodrigues(xi1k[k][3:])
        views.append((models[view_cam[k + 1]], gts[view_cam[k + 1]], R.T, -R.T @ xi1k[k][:3]))
    poses = S.make_poses(S.BASE_SEED + 13, n_frames, views, board)
    X1 = np.einsum("nij,kj->nki", S.rodrigues(poses[:, 3:]), board) + poses[:, None, :3]
    ds = []
    for k, (m, intr, Rc, tc) in enumerate(views):
        uv, ok = S.project(m, intr, np.einsum("ij,nkj->nki", Rc, X1) + tc)
        assert ok.all()
        ds.append((view_cam[k], [(V - 1, 0)] if k == 0 else [(k - 1, 1), (V - 1, 0)], board, uv))
    return {"cameras": [(m, S.INIT[m].copy()) for m in models],
            "transforms": [(True, (x + 0.004)[None, :]) for x in xi1k] + [(False, poses + 0.005)], "datasets": ds}


def _many_datasets(n):
    """n datasets of one image each: one camera, one pose sequence (image_index)"""
    c = _mono("eucm", n)
    _, chain, board, corners = c["datasets"][0]
    c["datasets"] = [(0, chain, board, corners[i:i + 1], np.array([i])) for i in range(n)]
    return c


def _ucm_on_bound():
    """data generated with xi = 3.2, start with xi ON its upper bound 3: the step points outwards, the column is held"""
    from visgeom_amd import synthetic as S

    gt = S.GT_UCM.copy()
    gt[0] = 3.2
    gt[1:3] *= (1 + 3.2) / (1 + S.GT_UCM[0])
    c = _mono("ucm", 200, gt=gt)
    c["cameras"][0][1][0] = 3.0
    return c


STIFF = np.array([300.0, 300.0, 300.0, 500.0, 500.0, 500.0])


def _seq_prior(c, stiff=STIFF):
    """a TransformationPrior on the case's sequence transform (acts on element 0, pulls towards its initial value)"""
    t = next(t for t, (g, _) in enumerate(c["transforms"]) if not g)
    c["priors"] = c.get("priors", []) + [(t, np.asarray(stiff, float), np.asarray(c["transforms"][t][1], float).reshape(-1, 6)[0].copy())]
    return c


def _handeye(n, lam, anchor=0, no_image=(), odo_sigma=0.002):
    """the hand-eye set of tests/test_gpu_solve.py: chain [xiBaseCam I, xiOdomBase_i I, xiOdomBoard D], OdometryPrior blocks
    between consecutive elements (odometry as the initial values), element `anchor` constant; frames `no_image` seen by no
    image (they move through the odometry alone).  G = 18."""
    from visgeom_amd import synthetic as S

    d = S.make_handeye(n, sigma=0.1, odo_sigma=odo_sigma)
    odo = d["odometry"]
    keep = np.array([i for i in range(n) if i not in set(no_image)], dtype=np.int64)
    return {"cameras": [("eucm", d["init_intrinsics"])],
            "transforms": [(True, d["init_xi_base_cam"][None, :]), (True, d["init_xi_odom_board"][None, :]), (False, odo.copy())],
            "datasets": [(0, [(0, 1), (2, 1), (1, 0)], d["board"], d["corners"][keep], keep)],
            "odometry_priors": [(2, i, 0.05, 0.05, lam, odo[i].copy(), odo[i + 1].copy()) for i in range(n - 1)],
            "const_poses": {2: [anchor]}}


def _wheeled(n, constant_wheels=False, lam=0.05):
    """the wheeled-base set of tests/test_gpu_solve.py: OdometryCost blocks between consecutive elements and a parameter
    block [radius_left, radius_right, track_gauge] (free or constant), the sequence started from the chained odometry,
    element 0 constant.  G = 21."""
    from oracle import vgo
    from visgeom_amd import synthetic as S

    d = S.make_wheeled(n, sigma=0.1)
    seq = [np.zeros(6)]
    for i in range(n - 1):
        seq.append(vgo.compose(seq[-1], vgo.OdometryCost(0.05, 0.05, 0.05, d["delta_q"][i], d["init_wheels"]).zeta))
    return {"cameras": [("eucm", d["init_intrinsics"])],
            "transforms": [(True, d["init_xi_base_cam"][None, :]), (True, d["init_xi_odom_board"][None, :]), (False, np.stack(seq))],
            "datasets": [(0, [(0, 1), (2, 1), (1, 0)], d["board"], d["corners"])],
            "parameter_blocks": [(d["init_wheels"].copy(), constant_wheels)],
            "odometry_costs": [(2, i, 0.05, 0.05, lam, d["delta_q"][i].copy(), 0) for i in range(n - 1)],
            "const_poses": {2: [0]}}


FAR = [0.5, 1.0, 1.0, 1.0, 1.0, 1.0]   # EUCM alpha halved: with radius 1e16 the second Gauss-Newton step overshoots


def case(name):
    """-> the case dict of tests/oracle_lm.py"""
    if name == "mono_eucm":
        c = _mono("eucm", 300)
    elif name == "mono_eucm_far":
        c = _mono("eucm", 300, scale=FAR)
    elif name == "mono_ucm_bound":
        c = _ucm_on_bound()
    elif name == "mono_eucm_16k":
        c = _mono("eucm", 16000, scale=[1.0, 1.0, 1.01, 1.01, 1.0, 1.0])
    elif name == "stereo_missing":
        c = _stereo(120, missing=set(range(1, 120, 5)), unobserved={7, 64})
    elif name == "stereo_const":
        c = _stereo(80, missing={3, 9})
        c["const_cameras"], c["const_poses"] = [0], {1: [0, 5, 41]}
    elif name == "stereo_const_transform":
        c = _stereo(80)
        c["const_transforms"] = [0]
    elif name == "rig4":
        c = G.case("rig")
    elif name == "rig_mei4":
        c = _wide_rig(4)
    elif name == "rig_mei8":
        c = _wide_rig(8)
    elif name == "rig_g16":      # one Mei camera seen through two views: 10 + 6
        c = _rig(["mei"], [0, 0])
    elif name == "rig_g24":      # one EUCM camera, four views: 6 + 3 x 6
        c = _rig(["eucm"], [0, 0, 0, 0])
    elif name == "stereo_mei":   # two Mei cameras: 2 x 10 + 6 = 26
        c = _rig(["mei", "mei"], [0, 1])
    elif name == "rig_g63":      # Mei + UCM, nine views: 15 + 8 x 6
        c = _rig(["mei", "ucm"], [0, 1, 0, 1, 0, 1, 0, 1, 0])
    elif name == "rig_g64":      # one Mei camera, ten views: 10 + 9 x 6
        c = _rig(["mei"], [0] * 10)
    elif name == "datasets_260":
        c = _many_datasets(260)
    # ---- prior / odometry cases (the full system of oracle_lm)
    elif name == "stereo_prior":           # a prior on the global stereo transform only
        c = _stereo(60, missing={4, 11})
        c["priors"] = [(0, STIFF, np.asarray(c["transforms"][0][1], float).ravel().copy())]
    elif name == "mono_eucm_seq_prior":    # a prior on element 0 of the mono sequence: G = 6
        c = _seq_prior(_mono("eucm", 60))
    elif name == "mono_mei_seq_prior":     # G = 10
        c = _seq_prior(_mono("mei", 60, seed=4))
    elif name == "mono_eucm_seq_prior_12":   # 12 poses: 72 pose rows, fewer than one row group
        c = _seq_prior(_mono("eucm", 12))
    elif name == "mono_eucm_seq_prior_400":  # 400 poses: 25 row groups
        c = _seq_prior(_mono("eucm", 400))
    elif name == "handeye_lam005":
        c = _handeye(12, 0.05)
    elif name == "handeye_lam1":
        c = _handeye(12, 1.0)
    elif name == "handeye_mid_anchor":     # anchor in the middle, frame 3 without an image
        c = _handeye(12, 0.05, anchor=6, no_image=(3,))
    elif name == "handeye_240":            # several hundred coupled poses
        c = _handeye(240, 0.05)
    elif name == "wheeled":
        c = _wheeled(10)
    elif name == "wheeled_const":
        c = _wheeled(10, constant_wheels=True)
    elif name == "rig4_seq_prior":         # G = 45: C = 46, dense Gram T = 3
        c = _seq_prior(G.case("rig"))
    elif name == "rig_g63_seq_prior":      # C = 64: T = 4
        c = _seq_prior(_rig(["mei", "ucm"], [0, 1, 0, 1, 0, 1, 0, 1, 0]))
    elif name == "rig_g64_seq_prior":      # C = 65: the pair kernel, T = 5
        c = _seq_prior(_rig(["mei"], [0] * 10))
    elif name == "rig_mei8_seq_prior":     # G = 122: the pair kernel, T = 8
        c = _seq_prior(_wide_rig(8))
    else:
        raise KeyError(name)
    c["name"] = name
    return c


def build_product_problem(vg, c):
    """the case on the HIP path (constant blocks, set_pose_constant, image_index, priors, odometry blocks and parameter
    blocks included)"""
    p = vg.CalibrationProblem(0)
    ccam, ctf = set(c.get("const_cameras", ())), set(c.get("const_transforms", ()))
    cams = [p.add_camera(m, i, constant=k in ccam) for k, (m, i) in enumerate(c["cameras"])]
    tfs = [p.add_transform(g, np.asarray(v).reshape(-1, 6) if not g else np.asarray(v).ravel(), constant=t in ctf)
           for t, (g, v) in enumerate(c["transforms"])]
    for ds in c["datasets"]:
        cam, chain, board, corners = ds[:4]
        index = ds[4] if len(ds) > 4 else None
        p.add_dataset(cams[cam], [(tfs[t], s) for t, s in chain], board, corners, image_index=index)
    for t, stiff, xi_prior in c.get("priors", ()):
        # the library's prior pulls towards the transform's initial value (element 0 of a sequence)
        assert np.array_equal(np.asarray(xi_prior, float), np.asarray(c["transforms"][t][1], float).reshape(-1, 6)[0])
        p.add_transformation_prior(tfs[t], stiff)
    for t, i, eV, eW, lam, xi1, xi2 in c.get("odometry_priors", ()):
        p.add_odometry_prior(tfs[t], i, eV, eW, lam, xi1, xi2)
    blocks = [p.add_parameter_block(v, constant=bool(k)) for v, k in c.get("parameter_blocks", ())]
    for t, i, eV, eW, lam, dq, b in c.get("odometry_costs", ()):
        p.add_odometry_cost(tfs[t], i, eV, eW, lam, dq, blocks[b])
    for t, idx in c.get("const_poses", {}).items():
        for i in idx:
            p.set_pose_constant(tfs[t], int(i))
    p.finalize()
    assert [p.parameter_block_offset(b) for b in blocks] == G.block_offsets(c)
    return p


def shard(c, cuts):
    """the case split over len(cuts) - 1 ranks by image: rank r holds the images of sequence elements cuts[r] .. cuts[r + 1]
    - 1.  A sequence without prior / odometry blocks is split with them (rank r holds those elements, re-indexed); a sequence
    coupled by odometry or carrying a prior is replicated on every rank with all of its blocks (the images keep their element
    through image_index), as the library requires.  Global blocks and priors on them are replicated.  -> [case dicts]"""
    seq = [t for t, (g, _) in enumerate(c["transforms"]) if not g]
    assert len(seq) == 1
    t = seq[0]
    coupled = any(b[0] == t for k in ("priors", "odometry_priors", "odometry_costs") for b in c.get(k, ()))
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        r = dict(c)
        r["datasets"] = []
        for ds in c["datasets"]:
            cam, chain, board, corners = ds[:4]
            index = np.asarray(ds[4] if len(ds) > 4 else np.arange(np.asarray(corners).shape[0]), dtype=np.int64)
            keep = (index >= lo) & (index < hi)
            r["datasets"].append((cam, chain, board, np.asarray(corners)[keep], index[keep] if coupled else index[keep] - lo))
        if not coupled:
            tr = list(c["transforms"])
            tr[t] = (False, np.asarray(c["transforms"][t][1]).reshape(-1, 6)[lo:hi])
            r["transforms"] = tr
            r["const_poses"] = {t: [i - lo for i in c.get("const_poses", {}).get(t, ()) if lo <= i < hi]}
        out.append(r)
    return out
