"""The calibration problems behind tests/golden/optimum_*.json, described once: tools/gen_golden.py solves them with
scipy's bounded trust-region least squares ON THE ORACLE (the optimum of a least-squares problem does not depend on the
solver: it stands in for "what Ceres would converge to"); tests/test_oracle_golden_optima.py checks on CPU
that every stored optimum is a stationary point of the oracle's cost; tests/test_gpu_golden.py holds the HIP solver to
them (intrinsics <= 1e-6, cost <= 1e-9).  BASELINE.json configs 2-5 at a reduced image count, inputs from the seeded
generator (visgeom_amd/synthetic.py) so only the answers are stored.

A case is a dict:
  cameras    [(model, initial intrinsics)]
  transforms [(is_global, initial values [count x 6])]
  datasets   [(camera index, chain [(transform index, status)], board, corners [n x N x 2])]
Parameter vector layout = the product's: [camera 0 | camera 1 | ... | transform 0 (count x 6) | ...].
"""
import numpy as np

BOUNDS = {  # eucm.h:228-246, ucm.h:199-215, mei.h:287-313
    "eucm": ([0, 0.1, 1, 1, 1, 1], [1, 10, 1e5, 1e5, 1e5, 1e5]),
    "ucm": ([0, 1, 1, 1, 1], [3, 1e5, 1e5, 1e5, 1e5]),
    "mei": ([0] + [-10] * 5 + [1] * 4, [3] + [10] * 5 + [1e5] * 4),
}


def case(name):
    from visgeom_amd import synthetic as S

    if name.startswith("mono_"):  # configs 2 / 4: one camera, chain [xiCamBoard DIRECT]
        model = name.split("_")[1]
        d = S.make_mono(model, 48, {"eucm": 2, "ucm": 2, "mei": 4}[model])
        return {"name": name, "cameras": [(model, d["init_intrinsics"])], "transforms": [(False, d["init_poses"])],
                "datasets": [(0, [(0, 0)], d["board"], d["corners"])]}
    if name == "stereo":  # config 3
        s = S.make_stereo(40)
        return {"name": name, "cameras": [("eucm", s["init_intrinsics1"]), ("eucm", s["init_intrinsics2"])],
                "transforms": [(True, s["init_xi12"][None, :]), (False, s["init_poses"])],
                "datasets": [(0, [(1, 0)], s["board"], s["corners1"]), (1, [(0, 1), (1, 0)], s["board"], s["corners2"])]}
    if name == "rig":  # config 5
        r = S.make_rig(24)
        return {"name": name, "cameras": list(zip(r["models"], r["init_intrinsics"])),
                "transforms": [(True, x[None, :]) for x in r["init_xi1k"]] + [(False, r["init_poses"])],
                "datasets": [(0, [(3, 0)], r["board"], r["corners"][0])] +
                            [(k + 1, [(k, 1), (3, 0)], r["board"], r["corners"][k + 1]) for k in range(3)]}
    raise KeyError(name)


NAMES = ["mono_eucm", "mono_ucm", "mono_mei", "stereo", "rig"]


def layout(c):
    """offsets of every camera / transform in the parameter vector, the initial vector, the box bounds (free-standing
    parameter blocks, the optional case key "parameter_blocks" of tests/oracle_lm.py, follow the transforms, unbounded)"""
    from oracle import vgo

    off, cam_off, tf_off = 0, [], []
    for model, intr in c["cameras"]:
        cam_off.append(off)
        off += vgo.NUM_INTRINSICS[vgo.MODELS[model]]
    for _, vals in c["transforms"]:
        tf_off.append(off)
        off += np.asarray(vals).size
    blocks = [np.asarray(v, float).ravel() for v, _ in c.get("parameter_blocks", ())]
    off += sum(b.size for b in blocks)
    x0 = np.concatenate([np.asarray(i, float).ravel() for _, i in c["cameras"]] +
                        [np.asarray(v, float).ravel() for _, v in c["transforms"]] + blocks)
    lb, ub = np.full(off, -np.inf), np.full(off, np.inf)
    for (model, _), o in zip(c["cameras"], cam_off):
        lo, hi = BOUNDS[model]
        lb[o:o + len(lo)], ub[o:o + len(hi)] = lo, hi
    return cam_off, tf_off, x0, lb, ub


def block_offsets(c):
    """offset of every free-standing parameter block (case key "parameter_blocks") in the parameter vector"""
    cam_off, tf_off, x0, _, _ = layout(c)
    off = x0.size - sum(np.asarray(v).size for v, _ in c.get("parameter_blocks", ()))
    out = []
    for v, _ in c.get("parameter_blocks", ()):
        out.append(off)
        off += np.asarray(v).size
    return out


def oracle_rows(c, x, want_jac=True):
    """stacked residual vector and dense Jacobian of the whole problem at x, from the oracle (one eval_dataset call
    per dataset, scattered into the problem's columns)"""
    from oracle import vgo

    cam_off, tf_off, _, _, _ = layout(c)
    rs, Js = [], []
    for cam, chain, board, corners in c["datasets"]:
        model = vgo.MODELS[c["cameras"][cam][0]]
        K = vgo.NUM_INTRINSICS[model]
        n, N = corners.shape[0], board.shape[0]
        status = [s for _, s in chain]
        bases = [tf_off[t] for t, _ in chain]
        strides = [0 if c["transforms"][t][0] else 6 for t, _ in chain]
        r, ji, jm = vgo.eval_dataset(model, status, board, corners, x, cam_off[cam], bases, strides, np.arange(n),
                                     want_jac=want_jac, threads=4)
        rs.append(r.ravel())
        if want_jac:
            J = np.zeros((n * 2 * N, x.size))
            J[:, cam_off[cam]:cam_off[cam] + K] = ji.reshape(-1, K)
            for l, (t, _) in enumerate(chain):
                if c["transforms"][t][0]:
                    J[:, tf_off[t]:tf_off[t] + 6] += jm[l].reshape(-1, 6)
                else:
                    for b in range(n):
                        J[b * 2 * N:(b + 1) * 2 * N, tf_off[t] + 6 * b:tf_off[t] + 6 * b + 6] = jm[l][b]
            Js.append(J)
    return np.concatenate(rs), (np.concatenate(Js) if want_jac else None)


def input_digest(c):
    """a number that changes when the seeded generator's output does (the fixtures only store answers)"""
    return float(sum(np.sum(np.asarray(corners) * np.arange(1, np.asarray(corners).size + 1).reshape(np.asarray(corners).shape) % 7)
                     for _, _, _, corners in c["datasets"]))


def build_product_problem(vg, c):
    """the same case on the HIP path"""
    p = vg.CalibrationProblem(0)
    cams = [p.add_camera(m, i) for m, i in c["cameras"]]
    tfs = [p.add_transform(g, np.asarray(v).reshape(-1, 6) if not g else np.asarray(v).ravel()) for g, v in c["transforms"]]
    for cam, chain, board, corners in c["datasets"]:
        p.add_dataset(cams[cam], [(tfs[t], s) for t, s in chain], board, corners)
    p.finalize()
    return p
