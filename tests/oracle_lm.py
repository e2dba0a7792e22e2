"""A plain restatement of ONE Levenberg-Marquardt step of the library, and of short chains of them, built from the ORACLE's
rows: the reference the solver's GPU routes are held to (tests/test_gpu_lm_steps.py).  Test infrastructure only: numpy and
oracle/vgo.py, nothing from the product.

The rule restated is the library's documented one (vg_lm_host_loop.hpp reduced_solve / step_and_evaluate / accept_or_shrink,
the header of vg_solver.hpp), not Ceres' internals:
  * damped normal equations  (J^T J + mu D) delta = -J^T r,  mu = 1 / radius,  D = clamp(diag J^T J, min_lm_diagonal,
    max_lm_diagonal) on the global AND on the pose blocks (no Jacobi scaling: the library clamps the unscaled diagonal);
  * arrow (Schur) form: every observed, non-constant pose is eliminated, S = U + mu D_g - sum W_i V_i'^-1 W_i^T,
    rhs = -gg + sum W_i V_i'^-1 gp_i;
  * constant blocks are frozen; a global column ON its box bound whose step points outwards is held (active set, repeated
    until no column leaves); the candidate is clamp(x + delta);
  * model change 1/2 delta^T (mu D delta - g), gain ratio rho = cost change / model change (-1 when the model change is
    not positive), success when rho > min_relative_decrease: radius / max(1/3, 1 - (2 rho - 1)^3) capped at the maximum
    radius, else radius / 2, / 4, ... (decrease_factor doubles until the next success);
  * SoftLOne(a) per grid block (one image): rows and residuals scaled by sqrt(rho'(s)) (Ceres' corrector, rho'' < 0),
    cost sum 1/2 rho(s).

A case is the dict of tests/golden_cases.py, with optional extensions:
  datasets        a fifth element image_index [n]: image b of the dataset uses element image_index[b] of its sequence
  const_cameras   camera indices whose intrinsics are constant
  const_transforms  transform indices that are constant (global or sequence)
  const_poses     {transform index: [element indices]} constant pose elements (set_pose_constant)
  priors          [(transform, stiffness[6], xi_prior[6])] TransformationPrior blocks (vg_problem_add_transformation_prior:
                  xi_prior is the transform's initial value); on a sequence the block acts on element 0
  odometry_priors [(transform, i, errV, errW, lam, xi1[6], xi2[6])] OdometryPrior blocks between elements i and i + 1
  parameter_blocks  [(values, constant)] free-standing global parameter blocks, placed after the transforms, unbounded
  odometry_costs  [(transform, i, errV, errW, lam, delta_q [n, 2], block)] OdometryCost blocks between elements i and i + 1
                  and parameter block `block` (its initial values are the cost's intrinsics prior)
A case with any of the last four keys is held to the FULL system (full_system, dense over all G + 6P columns): the grid rows
as in arrow_system, the prior and odometry rows uncorrected (the library adds them without a loss), with the oracle's own
Jacobians (vgo.transformation_prior, vgo.OdometryPrior, vgo.OdometryCost; not exact derivatives, so finite differences are
the wrong reference).  A pose is free when it is not constant and some residual block touches it.  Cases without them keep
the arrow path.
"""
import os

import numpy as np

from tests import golden_cases as G

BAR = 1e-11          # bar of the GPU tests on the backward error of a step (above the rounding floor of x, see backward_error)
RHO_MARGIN = 0.05    # |rho - min_relative_decrease| of every accept / reject decision a GPU test compares exactly

DEFAULTS = {"min_lm_diagonal": 1e-6, "max_lm_diagonal": 1e32, "max_trust_region_radius": 1e16, "min_relative_decrease": 1e-3,
            "initial_trust_region_radius": 1e4, "use_bounds": True, "soft_l1_scale": 0.0, "function_tolerance": 1e-15}


def _threads(threads):
    return threads if threads is not None else max(1, min(16, os.cpu_count() or 1))


def _dataset(c, d):
    ds = c["datasets"][d]
    cam, chain, board, corners = ds[:4]
    n = np.asarray(corners).shape[0]
    index = np.asarray(ds[4], dtype=np.int64) if len(ds) > 4 and ds[4] is not None else np.arange(n, dtype=np.int64)
    return cam, chain, np.asarray(board, float), np.asarray(corners, float), index


def _rows(c, x, d, tf_off, cam_off, want_jac, threads):
    from oracle import vgo

    cam, chain, board, corners, index = _dataset(c, d)
    model = vgo.MODELS[c["cameras"][cam][0]]
    status = [s for _, s in chain]
    bases = [tf_off[t] for t, _ in chain]
    strides = [0 if c["transforms"][t][0] else 6 for t, _ in chain]
    return vgo.eval_dataset(model, status, board, corners, x, cam_off[cam], bases, strides, index, want_jac=want_jac,
                            threads=_threads(threads))


def soft_l1(s, a):
    """SoftLOneLoss(a) of the squared norms s -> (rho(s), rho'(s)); a = 0: no loss (rho = s, rho' = 1)"""
    s = np.asarray(s, float)
    if not a:
        return s, np.ones_like(s)
    q = np.sqrt(1.0 + s / (a * a))
    return 2.0 * a * a * (q - 1.0), 1.0 / q


def cost_floor(r, corners, soft_l1_scale=0.0):
    """rounding floor of the cost of one or more images (r, corners [n, 2N]): every residual u - c is known to a few ulps of
    the corner coordinate c, so the cost 1/2 sum rho(|r_b|^2) is known to 4 eps sum_b rho'(s_b) sum_i |r_i| |c_i|.  Next to the
    relative bar, it matters where the cost is nearly zero (noise-free data close to the optimum)."""
    r, corners = np.atleast_2d(r), np.atleast_2d(corners)
    w = soft_l1(np.sum(r * r, axis=1), soft_l1_scale)[1]
    return 4.0 * np.finfo(float).eps * float(np.sum(w * np.sum(np.abs(r) * np.abs(corners), axis=1)))


def cost(c, x, soft_l1_scale=0.0, threads=None, floor=False):
    """sum over images of 1/2 rho(|r_b|^2) at x (plain 1/2 |r|^2 without a loss), plus 1/2 |r|^2 of the prior and odometry
    blocks; floor: also its rounding floor"""
    cam_off, tf_off, _, _, _ = G.layout(c)
    x = np.asarray(x, float)
    total, fl = 0.0, 0.0
    for d in range(len(c["datasets"])):
        if np.asarray(c["datasets"][d][3]).shape[0] == 0:
            continue
        r, _, _ = _rows(c, x, d, tf_off, cam_off, False, threads)
        total += float(np.sum(soft_l1(np.sum(r * r, axis=1), soft_l1_scale)[0])) if soft_l1_scale else float(np.sum(r * r))
        if floor:
            fl += cost_floor(r, np.asarray(c["datasets"][d][3], float).reshape(r.shape), soft_l1_scale)
    if has_extras(c):      # prior and odometry blocks, without a loss
        e, efl = extra_cost(c, x, floor=True)
        return (0.5 * total + e, fl + efl) if floor else 0.5 * total + e
    return (0.5 * total, fl) if floor else 0.5 * total


def arrow_system(c, x, soft_l1_scale=0.0, threads=None):
    """the normal equations of the (corrected) rows at x in arrow form:
    U [G, G], gg [G], V [P, 6, 6], W [P, G, 6], gp [P, 6] -- G global columns (every camera, every global transform, constant
    ones included: `frozen` marks them), P pose blocks (every element of every sequence transform; `pose_free` marks the
    observed, non-constant ones) -- and the cost, gcols / pose_param (parameter index of every global column / pose block),
    lb / ub (box of every global column)."""
    from oracle import vgo

    x = np.asarray(x, float)
    cam_off, tf_off, _, lb, ub = G.layout(c)
    const_cams = set(c.get("const_cameras", ()))
    const_tfs = set(c.get("const_transforms", ()))
    gcols, frozen, cam_g, tf_g, pb_g = [], [], [], {}, []
    for k, ((model, _), o) in enumerate(zip(c["cameras"], cam_off)):
        K = vgo.NUM_INTRINSICS[vgo.MODELS[model]]
        cam_g.append(np.arange(len(gcols), len(gcols) + K))
        gcols += list(range(o, o + K))
        frozen += [k in const_cams] * K
    pose_base, pose_param, pose_const = {}, [], []
    for t, (is_global, vals) in enumerate(c["transforms"]):
        if is_global:
            tf_g[t] = np.arange(len(gcols), len(gcols) + 6)
            gcols += list(range(tf_off[t], tf_off[t] + 6))
            frozen += [t in const_tfs] * 6
        else:
            m = np.asarray(vals).reshape(-1, 6).shape[0]
            pose_base[t] = len(pose_param)
            pose_param += [tf_off[t] + 6 * i for i in range(m)]
            cp = set(c.get("const_poses", {}).get(t, ()))
            pose_const += [t in const_tfs or i in cp for i in range(m)]
    for (vals, const), o in zip(c.get("parameter_blocks", ()), G.block_offsets(c)):
        k = np.asarray(vals).size
        pb_g.append(np.arange(len(gcols), len(gcols) + k))
        gcols += list(range(o, o + k))
        frozen += [bool(const)] * k
    gcols, pose_param = np.array(gcols, dtype=np.int64), np.array(pose_param, dtype=np.int64)
    Gn, P = gcols.size, pose_param.size
    U, gg = np.zeros((Gn, Gn)), np.zeros(Gn)
    V, W, gp = np.zeros((P, 6, 6)), np.zeros((P, Gn, 6)), np.zeros((P, 6))
    cost2 = 0.0
    for d in range(len(c["datasets"])):
        cam, chain, board, corners, index = _dataset(c, d)
        n = corners.shape[0]
        if n == 0:
            continue
        r, ji, jm = _rows(c, x, d, tf_off, cam_off, True, threads)
        if soft_l1_scale:                                         # Ceres' corrector: rows and residuals times sqrt(rho')
            rho, w = soft_l1(np.sum(r * r, axis=1), soft_l1_scale)
            cost2 += float(np.sum(rho))
            sw = np.sqrt(w)
            r, ji, jm = r * sw[:, None], ji * sw[:, None, None], [j * sw[:, None, None] for j in jm]
        else:
            cost2 += float(np.sum(r * r))
        cols, blocks, B, pb = [cam_g[cam]], [ji], None, None
        for l, (t, _) in enumerate(chain):
            if c["transforms"][t][0]:
                cols.append(tf_g[t])
                blocks.append(jm[l])
            else:
                assert B is None, "one sequence member per chain"
                B, pb = jm[l], pose_base[t] + index
        cols = np.concatenate(cols)
        A = np.concatenate(blocks, axis=2)                       # [n, 2N, G_local]
        A2 = A.reshape(-1, A.shape[2])
        U[np.ix_(cols, cols)] += A2.T @ A2
        gg[cols] += A2.T @ r.ravel()
        if B is not None:
            np.add.at(V, pb, np.einsum("bri,brj->bij", B, B))
            Wl = np.zeros((n, Gn, 6))
            Wl[:, cols, :] = np.einsum("bri,brj->bij", A, B)
            np.add.at(W, pb, Wl)
            np.add.at(gp, pb, np.einsum("bri,br->bi", B, r))
    seen = np.einsum("pii->p", V) > 0                            # poses without observations do not move
    return {"U": U, "gg": gg, "V": V, "W": W, "gp": gp, "cost": 0.5 * cost2, "gcols": gcols, "pose_param": pose_param,
            "frozen": np.array(frozen, dtype=bool), "pose_free": seen & ~np.array(pose_const, dtype=bool),
            "lb": lb[gcols], "ub": ub[gcols], "x": x, "tf_g": tf_g, "pb_g": pb_g, "pose_base": pose_base,
            "pose_const": np.array(pose_const, dtype=bool), "seen": seen}


EXTRA_KEYS = ("priors", "odometry_priors", "parameter_blocks", "odometry_costs")


def has_extras(c):
    """does the case carry prior / odometry / parameter-block keys (-> the full system)"""
    return any(c.get(k) for k in EXTRA_KEYS)


def _pose_cols(sy, t, i):
    Gn = sy["gcols"].size
    p = sy["pose_base"][t] + i
    return np.arange(Gn + 6 * p, Gn + 6 * p + 6), p


def extra_blocks(c, x, sy):
    """the prior and odometry residual blocks at x, from the oracle: [dict(kind, r [6], cols [system columns], J [6, cols],
    poses [pose blocks touched])]; system columns: global column g -> g, element k of pose block p -> G + 6 p + k"""
    from oracle import vgo

    x = np.asarray(x, float)
    _, tf_off, _, _, _ = G.layout(c)
    out = []
    for t, stiff, xi_prior in c.get("priors", ()):
        if c["transforms"][t][0]:
            cols, poses = sy["tf_g"][t], []
        else:
            cols, p = _pose_cols(sy, t, 0)
            poses = [p]
        r, J = vgo.transformation_prior(stiff, xi_prior, x[sy["x_cols"][cols]])
        out.append({"kind": "prior", "r": r, "cols": cols, "J": J, "poses": poses})
    for t, i, eV, eW, lam, xi1, xi2 in c.get("odometry_priors", ()):
        c1, p1 = _pose_cols(sy, t, i)
        c2, p2 = _pose_cols(sy, t, i + 1)
        r, J1, J2 = vgo.OdometryPrior(eV, eW, lam, xi1, xi2).evaluate(x[sy["x_cols"][c1]], x[sy["x_cols"][c2]])
        out.append({"kind": "odometry_prior", "r": r, "cols": np.concatenate([c1, c2]), "J": np.hstack([J1, J2]),
                    "poses": [p1, p2]})
    for t, i, eV, eW, lam, dq, b in c.get("odometry_costs", ()):
        c1, p1 = _pose_cols(sy, t, i)
        c2, p2 = _pose_cols(sy, t, i + 1)
        c3 = sy["pb_g"][b]
        blk = vgo.OdometryCost(eV, eW, lam, dq, np.asarray(c["parameter_blocks"][b][0], float))
        r, J1, J2, J3 = blk.evaluate(x[sy["x_cols"][c1]], x[sy["x_cols"][c2]], x[sy["x_cols"][c3]])
        out.append({"kind": "odometry_cost", "r": r, "cols": np.concatenate([c1, c2, c3]), "J": np.hstack([J1, J2, J3]),
                    "poses": [p1, p2], "n_pose_cols": 12})
    return out


def _x_cols(sy):
    """parameter index of every system column"""
    return np.concatenate([sy["gcols"], (sy["pose_param"][:, None] + np.arange(6)[None, :]).ravel()])


def extra_cost(c, x, floor=False):
    """sum of 1/2 |r|^2 over the prior and odometry blocks (no loss); floor: also its rounding floor, 4 eps sum_k |r_k|
    sum_j |J_kj| |x_j| (what rounding x, relative eps, moves the cost by)"""
    if not has_extras(c):
        return (0.0, 0.0) if floor else 0.0
    x = np.asarray(x, float)
    sy = _skeleton(c, x)
    tot, fl = 0.0, 0.0
    for b in extra_blocks(c, x, sy):
        tot += float(b["r"] @ b["r"])
        fl += 4.0 * np.finfo(float).eps * float(np.abs(b["r"]) @ (np.abs(b["J"]) @ np.abs(x[sy["x_cols"][b["cols"]]])))
    return (0.5 * tot, fl) if floor else 0.5 * tot


def _skeleton(c, x):
    """the column bookkeeping of arrow_system without its rows"""
    sy = arrow_system(dict(c, datasets=[]), x)
    sy["x_cols"] = _x_cols(sy)
    return sy


def full_system(c, x, soft_l1_scale=0.0, threads=None):
    """the damped step's system of a case with prior / odometry blocks, dense over all G + 6P columns (globals first, then
    the pose blocks): H [n, n], g [n], the cost, the arrow system's bookkeeping (gcols, pose_param, frozen, pose_free, lb,
    ub, gg, gp) and the pieces the planted errors of tests/test_oracle_lm.py take apart (diag_grid: diag H of the grid
    rows alone; blocks: the extra residual blocks)"""
    sy = arrow_system(c, x, soft_l1_scale, threads)
    Gn, P = sy["gcols"].size, sy["pose_param"].size
    n = Gn + 6 * P
    H, g = np.zeros((n, n)), np.zeros(n)
    H[:Gn, :Gn] = sy["U"]
    g[:Gn] = sy["gg"]
    Wf = np.transpose(sy["W"], (1, 0, 2)).reshape(Gn, 6 * P)
    H[:Gn, Gn:], H[Gn:, :Gn] = Wf, Wf.T
    for p in range(P):
        H[Gn + 6 * p:Gn + 6 * p + 6, Gn + 6 * p:Gn + 6 * p + 6] = sy["V"][p]
    g[Gn:] = sy["gp"].ravel()
    diag_grid = np.diag(H).copy()
    sy["x_cols"] = _x_cols(sy)
    blocks = extra_blocks(c, x, sy)
    touched = sy["seen"].copy()
    cost2 = 2.0 * sy["cost"]
    for b in blocks:
        cols, J, r = b["cols"], b["J"], b["r"]
        H[np.ix_(cols, cols)] += J.T @ J
        g[cols] += J.T @ r
        cost2 += float(r @ r)
        touched[b["poses"]] = True
    sy.update({"dense": True, "H": H, "g": g, "cost": 0.5 * cost2, "diag_grid": diag_grid, "blocks": blocks,
               "pose_free": touched & ~sy["pose_const"], "gg": g[:Gn], "gp": g[Gn:].reshape(P, 6)})
    return sy


def system(c, x, soft_l1_scale=0.0, threads=None):
    """the step's system: the full (dense) one for a case with prior / odometry blocks, else the arrow one"""
    return full_system(c, x, soft_l1_scale, threads) if has_extras(c) else arrow_system(c, x, soft_l1_scale, threads)


def _dense_free(sy, held):
    return np.concatenate([~held, np.repeat(sy["pose_free"], 6)])


def dense_step(sy, mu, opt=None, plant=None):
    """(H + mu D) delta = -g on the full system, D = clamp(diag H) over the free columns, the active set of damped_step.
    plant: deliberate errors for the tests of the step metric ("image_only_diag": pose damping clamped from the grid rows'
    diagonal; {"drop_e": k}: the pose-pose coupling of odometry block k dropped; "drop_wodo": the pose-global coupling of
    every OdometryCost block dropped; "prior_twice": every TransformationPrior block counted twice; {"keep_frozen": p}:
    constant pose p eliminated as a unit block with its couplings kept).  -> the dict of damped_step"""
    plant = plant or {}
    o = dict(DEFAULTS, **(opt or {}))
    H, g = sy["H"], sy["g"]
    Gn, P = sy["gcols"].size, sy["pose_param"].size
    if plant:
        H, g = H.copy(), g.copy()
    for k, b in enumerate(sy["blocks"]):
        cols, J, r = b["cols"], b["J"], b["r"]
        if b["kind"] == "prior" and "prior_twice" in plant:
            H[np.ix_(cols, cols)] += J.T @ J
            g[cols] += J.T @ r
        if b["kind"] != "prior" and plant.get("drop_e") == k:
            a, c2 = cols[:6], cols[6:12]
            E = J[:, :6].T @ J[:, 6:12]
            H[np.ix_(a, c2)] -= E
            H[np.ix_(c2, a)] -= E.T
        if b["kind"] == "odometry_cost" and "drop_wodo" in plant:
            pc, gc = cols[:12], cols[12:]
            Wo = J[:, :12].T @ J[:, 12:]
            H[np.ix_(pc, gc)] -= Wo
            H[np.ix_(gc, pc)] -= Wo.T
    D = clamp_diag(np.diag(H), o)
    if "image_only_diag" in plant:
        D[Gn:] = clamp_diag(sy["diag_grid"][Gn:], o)
    pose_free = sy["pose_free"].copy()
    if "keep_frozen" in plant:
        q = plant["keep_frozen"]
        pose_free[q] = True
        qc = np.arange(Gn + 6 * q, Gn + 6 * q + 6)
        H[np.ix_(qc, qc)] = np.eye(6)
        D[qc] = 0.0
        g[qc] = 0.0
    held = sy["frozen"].copy()
    xg = sy["x"][sy["gcols"]]
    for _ in range(Gn + 1):
        f = np.concatenate([~held, np.repeat(pose_free, 6)])
        A = H[np.ix_(f, f)]
        if mu:
            A = A + np.diag(mu * D[f])
        d = np.zeros(H.shape[0])
        if f.any():
            d[f] = np.linalg.solve(A, -g[f])
        dg = d[:Gn]
        if not o["use_bounds"]:
            break
        out = ~held & (((xg <= sy["lb"]) & (dg < 0)) | ((xg >= sy["ub"]) & (dg > 0)))
        if not out.any():
            break
        held |= out
    dp = d[Gn:].reshape(P, 6).copy()
    dp[~sy["pose_free"]] = 0.0
    return {"dg": dg.copy(), "dp": dp, "held": held, "Dg": D[:Gn], "Dp": D[Gn:].reshape(P, 6)}


def dense_backward_error(sy, mu, dg, dp, opt=None, x_next=None):
    """backward_error on the full system: the same Jacobi-scaled, blockwise normwise value, where the rows of a pose block
    touch every global column, its own columns and those of the poses it is coupled to (odometry neighbours)"""
    o = dict(DEFAULTS, **(opt or {}))
    held = damped_step(sy, mu, o)["held"]
    Gn, P = sy["gcols"].size, sy["pose_param"].size
    pf = sy["pose_free"]
    f = _dense_free(sy, held)
    H = sy["H"]
    A = H + np.diag(mu * clamp_diag(np.diag(H), o))
    d = np.concatenate([np.asarray(dg, float), np.asarray(dp, float).ravel()])
    s = np.zeros(H.shape[0])
    s[f] = 1.0 / np.sqrt(np.diag(A)[f])
    As = A * s[:, None] * s[None, :]
    gs, ds = sy["g"] * s, np.where(f, d / np.where(s > 0, s, 1.0), 0.0)
    res = As @ ds + gs
    eps = np.finfo(float).eps
    e = None
    if x_next is not None:
        e = np.where(f, eps * np.abs(np.asarray(x_next, float)[sy["x_cols"]]) / np.where(s > 0, s, 1.0), 0.0)
    gsel = np.zeros_like(f)
    gsel[:Gn] = f[:Gn]

    def block(rows, touch):
        nd = np.linalg.norm(ds[touch])
        v = np.linalg.norm(res[rows]) / (np.linalg.norm(As[np.ix_(rows, touch)]) * nd + np.linalg.norm(gs[rows]))
        return v, (np.linalg.norm(e[touch]) / nd if e is not None else 0.0)

    be_g, fl_g = block(gsel, f) if gsel.any() else (0.0, 0.0)
    be_p, fl_p = np.zeros(P), np.zeros(P)
    Hp = np.abs(H[Gn:, Gn:]).reshape(P, 6, P, 6).sum(axis=(1, 3)) > 0     # pose-pose coupling pattern
    for p in np.nonzero(pf)[0]:
        rows = np.arange(Gn + 6 * p, Gn + 6 * p + 6)
        touch = gsel.copy()
        for q in np.nonzero(Hp[p] & pf)[0]:
            touch[Gn + 6 * q:Gn + 6 * q + 6] = True
        be_p[p], fl_p[p] = block(rows, touch)
    if x_next is None:
        return float(be_g), be_p
    return float(be_g), be_p, float(fl_g), fl_p


def clamp_diag(d, opt=None):
    o = dict(DEFAULTS, **(opt or {}))
    return np.clip(d, o["min_lm_diagonal"], o["max_lm_diagonal"])


def damped_step(sy, mu, opt=None, plant=None):
    """(J^T J + mu D) delta = -J^T r in arrow form on the system of arrow_system, with the active set of the box bounds.
    mu = 0 without an option dict: D never enters (the Gauss-Newton step).  plant: deliberate errors for the tests of
    the step metric ({"mu_scale": s} the damping times s, "no_pose_damping", {"drop_w": i} pose i's coupling dropped,
    {"drop_rhs": i} pose i's term of the reduced right-hand side dropped).
    -> dict(dg [G], dp [P, 6], held [G], Dg [G], Dp [P, 6])  (the full system of a case with prior / odometry blocks:
    dense_step)"""
    if sy.get("dense"):
        return dense_step(sy, mu, opt, plant)
    plant = plant or {}
    o = dict(DEFAULTS, **(opt or {}))
    U, gg, V, W, gp = sy["U"], sy["gg"], sy["V"], sy["W"].copy(), sy["gp"]
    free = sy["pose_free"]
    Gn = gg.size
    mu_s = mu * plant.get("mu_scale", 1.0)
    Dg = clamp_diag(np.diag(U), o)
    Dp = clamp_diag(np.einsum("pii->pi", V), o)
    Vd = V.copy()
    if mu and "no_pose_damping" not in plant:
        Vd[:, np.arange(6), np.arange(6)] += mu_s * Dp
    if "drop_w" in plant:
        W[plant["drop_w"]] = 0.0
    Vd[~free] = np.eye(6)
    rhs_p = np.concatenate([np.swapaxes(W, 1, 2), gp[:, :, None]], axis=2)   # [P, 6, G + 1]
    rhs_p[~free] = 0.0
    X = np.linalg.solve(Vd, rhs_p)                               # V'^-1 [W^T | g_p]
    S = U - np.einsum("pgi,pih->gh", W, X[:, :, :Gn])
    if mu:
        S[np.arange(Gn), np.arange(Gn)] += mu_s * Dg
    y = X[:, :, Gn]
    if "drop_rhs" in plant:
        y = y.copy()
        y[plant["drop_rhs"]] = 0.0
    rhs = -gg + np.einsum("pgi,pi->g", W, y)
    held = sy["frozen"].copy()
    xg = sy["x"][sy["gcols"]]
    for _ in range(Gn + 1):
        f = ~held
        dg = np.zeros(Gn)
        if f.any():
            dg[f] = np.linalg.solve(S[np.ix_(f, f)], rhs[f])
        if not o["use_bounds"]:
            break
        out = f & (((xg <= sy["lb"]) & (dg < 0)) | ((xg >= sy["ub"]) & (dg > 0)))
        if not out.any():
            break
        held |= out
    dp = -(X[:, :, Gn] + np.einsum("pig,g->pi", X[:, :, :Gn], dg))
    dp[~free] = 0.0
    return {"dg": dg, "dp": dp, "held": held, "Dg": Dg, "Dp": Dp}


def apply_step(sy, dg, dp):
    """the candidate: clamp(x + delta) on the global columns (poses are unbounded)"""
    x = sy["x"].copy()
    x[sy["gcols"]] = np.clip(x[sy["gcols"]] + dg, sy["lb"], sy["ub"])
    idx = sy["pose_param"][:, None] + np.arange(6)[None, :]
    x[idx] += dp
    return x


def model_change(sy, st, mu):
    """1/2 delta^T (mu D delta - g) over the free columns (the library's model decrease of the exact LM step)"""
    f, pf = ~sy["frozen"], sy["pose_free"]
    dg, dp = st["dg"][f], st["dp"][pf]
    ddd = np.sum(st["Dg"][f] * dg * dg) + np.sum(st["Dp"][pf] * dp * dp)
    gd = np.dot(sy["gg"][f], dg) + np.sum(sy["gp"][pf] * dp)
    return 0.5 * (mu * ddd - gd)


def lm_step(c, x, radius, decrease_factor=2.0, opt=None, threads=None, sy=None):
    """one iteration at x with trust-region radius `radius` -> dict(delta (dg, dp, held), mu, model_change, cost,
    cand_cost, rho, success, x_next, radius, decrease_factor)"""
    o = dict(DEFAULTS, **(opt or {}))
    a = o["soft_l1_scale"]
    if sy is None:
        sy = system(c, x, a, threads)
    mu = 1.0 / radius
    st = damped_step(sy, mu, o)
    mc = model_change(sy, st, mu)
    xc = apply_step(sy, st["dg"], st["dp"])
    cc = cost(c, xc, a, threads)
    rho = (sy["cost"] - cc) / mc if mc > 0 else -1.0
    success = bool(np.isfinite(cc) and rho > o["min_relative_decrease"])
    # the function tolerance test (ends a solve at the current point) must not fire in a compared chain
    assert not (mc > 0 and np.isfinite(cc) and abs(sy["cost"] - cc) <= o["function_tolerance"] * sy["cost"]), "function tolerance"
    if success:
        f = 1.0 - (2.0 * rho - 1.0) ** 3
        radius_n, df = min(radius / max(f, 1.0 / 3.0), o["max_trust_region_radius"]), 2.0
    else:
        radius_n, df = radius / decrease_factor, decrease_factor * 2.0
    return {"step": st, "sy": sy, "mu": mu, "model_change": mc, "cost": sy["cost"], "cand_cost": cc, "rho": rho,
            "success": success, "x_next": xc if success else sy["x"], "radius": radius_n, "decrease_factor": df}


def lm_chain(c, x0, k, opt=None, threads=None):
    """k iterations from x0 -> list of k dicts: x, cost, radius, n_success after the iteration, rho / success / held /
    mu of the iteration"""
    o = dict(DEFAULTS, **(opt or {}))
    x, radius, df, ns = np.asarray(x0, float), o["initial_trust_region_radius"], 2.0, 0
    out = []
    for _ in range(k):
        s = lm_step(c, x, radius, df, o, threads)
        ns += s["success"]
        x, radius, df = s["x_next"], s["radius"], s["decrease_factor"]
        out.append({"x": x, "cost": s["cand_cost"] if s["success"] else s["cost"], "radius": radius, "n_success": ns,
                    "rho": s["rho"], "success": s["success"], "held": s["step"]["held"], "mu": s["mu"]})
    return out


def split_step(sy, x_next):
    """the step x_next - x of the system's point, in the system's columns -> (dg [G], dp [P, 6])"""
    d = np.asarray(x_next, float) - sy["x"]
    return d[sy["gcols"]], d[sy["pose_param"][:, None] + np.arange(6)[None, :]]


def backward_error(sy, mu, dg, dp, opt=None, x_next=None):
    """normwise backward error of a step in the damped system (H + mu D) delta = -g of arrow_system, blockwise, after a
    symmetric Jacobi scaling (columns scaled to a unit damped diagonal, so that no column's units hide an error):
        ||(H + mu D) delta + g||_B / (||(H + mu D)_B|| ||delta_B|| + ||g_B||)
    for the free global rows (one value, its rows touch every column) and for every free pose block (its rows touch the
    global columns and its own).  Frobenius norms.  Held / frozen columns and constant poses are left out (their step is
    zero by construction; a caller checks that separately).
    x_next: the point the step was recovered from (delta = x_next - x): then also the rounding floor of every block,
    ||e_B|| / ||delta_B|| with e = eps |x_next| in the same scaling -- what the rounding of x alone can add to the value.
    -> (global value, [P] per pose (0 for fixed poses)), and with x_next also (global floor, [P] floors)
    (the full system of a case with prior / odometry blocks: dense_backward_error)"""
    if sy.get("dense"):
        return dense_backward_error(sy, mu, dg, dp, opt, x_next)
    o = dict(DEFAULTS, **(opt or {}))
    held = damped_step(sy, mu, o)["held"]
    f, pf = ~held, sy["pose_free"]
    U, gg, V, W, gp = sy["U"][np.ix_(f, f)], sy["gg"][f], sy["V"][pf], sy["W"][pf][:, f, :], sy["gp"][pf]
    dg, dp = np.asarray(dg, float)[f], np.asarray(dp, float)[pf]
    Ud = U + np.diag(mu * clamp_diag(np.diag(U), o))
    Vd = V.copy()
    Vd[:, np.arange(6), np.arange(6)] += mu * clamp_diag(np.einsum("pii->pi", V), o)
    sg = 1.0 / np.sqrt(np.diag(Ud))                              # Jacobi scaling of the damped system
    sp = 1.0 / np.sqrt(np.einsum("pii->pi", Vd))
    Ud = Ud * sg[:, None] * sg[None, :]
    Vd = Vd * sp[:, :, None] * sp[:, None, :]
    W = W * sg[None, :, None] * sp[:, None, :]
    gg, gp = gg * sg, gp * sp
    dg, dp = dg / sg, dp / sp
    res_g = Ud @ dg + np.einsum("pgi,pi->g", W, dp) + gg
    res_p = np.einsum("pgi,g->pi", W, dg) + np.einsum("pij,pj->pi", Vd, dp) + gp
    nd_all = np.sqrt(dg @ dg + np.sum(dp * dp))
    a_g = np.sqrt(np.sum(Ud * Ud) + np.sum(W * W))
    be_g = np.linalg.norm(res_g) / (a_g * nd_all + np.linalg.norm(gg)) if f.any() else 0.0
    a_p = np.sqrt(np.sum(W * W, axis=(1, 2)) + np.sum(Vd * Vd, axis=(1, 2)))
    nd_p = np.sqrt(dg @ dg + np.sum(dp * dp, axis=1))
    be_p = np.zeros(sy["pose_free"].size)
    be_p[pf] = np.linalg.norm(res_p, axis=1) / (a_p * nd_p + np.linalg.norm(gp, axis=1))
    if x_next is None:
        return float(be_g), be_p
    xn = np.abs(np.asarray(x_next, float))
    eg = np.finfo(float).eps * xn[sy["gcols"]][f] / sg
    ep = np.finfo(float).eps * xn[sy["pose_param"][:, None] + np.arange(6)[None, :]][pf] / sp
    fl_g = np.sqrt(eg @ eg + np.sum(ep * ep)) / nd_all if f.any() else 0.0
    fl_p = np.zeros(sy["pose_free"].size)
    fl_p[pf] = np.sqrt(eg @ eg + np.sum(ep * ep, axis=1)) / nd_p
    return float(be_g), be_p, float(fl_g), fl_p


def step_backward_error(sy, mu, dg, dp, opt=None):
    """max over the blocks of backward_error"""
    g, p = backward_error(sy, mu, dg, dp, opt)
    return max(g, float(np.max(p)) if p.size else 0.0)


def recovered_step_error(sy, mu, x_next, opt=None):
    """for the step x_next - x recovered from two points: (max over the blocks of backward error minus rounding floor,
    max backward error, max floor)"""
    dg, dp = split_step(sy, x_next)
    g, p, fg, fp = backward_error(sy, mu, dg, dp, opt, x_next)
    return max(g - fg, float(np.max(p - fp)) if p.size else 0.0), max(g, float(np.max(p, initial=0.0))), max(fg, float(np.max(fp, initial=0.0)))


# ---- the per-image pose refinement (vg_refine_poses / vg_pose_lm.hpp): one 6-DOF problem per image, intrinsics constant ----
POSE_LM_DEFAULTS = dict(DEFAULTS, max_num_iterations=500, function_tolerance=1e-6, gradient_tolerance=1e-10,
                        parameter_tolerance=1e-8, soft_l1_scale=25.0, min_trust_region_radius=1e-32)
TERM = {"FUNCTION": 0, "GRADIENT": 1, "PARAMETER": 2, "NO_CONVERGENCE": 3, "RADIUS_TOO_SMALL": 4}


def _pose_rows(model, intr, board, corners, x):
    from oracle import vgo

    r, jac = vgo.eval_block(vgo.MODELS[model], [vgo.DIRECT], board, corners, [intr, x], jac_mask=[False, True])
    return r, jac[1]


def pose_lm(model, intr, board, corners, x0, opt=None):
    """the library's LM on ONE image: (w J^T J + mu D) delta = -w J^T r with w = rho'(s) of the current point (Ceres'
    corrector on the one block), D = clamp(diag(w J^T J)); the gradient and parameter tests before the decision, the
    function tolerance after an accepted step; the radius rule of lm_step.  -> dict(x, iterations, cost, termination, and
    per iteration: x, cost, radius, gain, accepted, and how close each convergence test came to firing)"""
    o = dict(POSE_LM_DEFAULTS, **(opt or {}))
    a = o["soft_l1_scale"]
    x = np.asarray(x0, float).copy()
    r, J = _pose_rows(model, intr, board, corners, x)
    rho, w = soft_l1(r @ r, a)
    cost, radius, df, it, term = 0.5 * float(rho), o["initial_trust_region_radius"], 2.0, 0, TERM["NO_CONVERGENCE"]
    trace = []
    while it < o["max_num_iterations"]:
        it += 1
        A, g = w * (J.T @ J), w * (J.T @ r)
        D = clamp_diag(np.diag(A), o)
        mu = 1.0 / radius
        dx = -np.linalg.solve(A + mu * np.diag(D), g)
        xc = x + dx
        rc, Jc = _pose_rows(model, intr, board, corners, xc)
        rho_c, w_c = soft_l1(rc @ rc, a)
        cost_c = 0.5 * float(rho_c)
        mc = 0.5 * (mu * np.sum(D * dx * dx) - g @ dx)
        gain = (cost - cost_c) / mc if mc > 0 else -1.0
        step = {"mu": mu, "gain": gain, "x_prev": x.copy(), "grad": np.max(np.abs(g)) / o["gradient_tolerance"],
                "param": np.linalg.norm(dx) / (o["parameter_tolerance"] * (np.linalg.norm(x) + o["parameter_tolerance"]))}
        if np.max(np.abs(g)) <= o["gradient_tolerance"]:
            term = TERM["GRADIENT"]
        elif np.linalg.norm(dx) <= o["parameter_tolerance"] * (np.linalg.norm(x) + o["parameter_tolerance"]):
            term = TERM["PARAMETER"]
        elif np.isfinite(cost_c) and gain > o["min_relative_decrease"]:
            prev, x, r, J, w, cost = cost, xc, rc, Jc, w_c, cost_c
            f = 1.0 - (2.0 * gain - 1.0) ** 3
            radius, df = min(radius / max(f, 1.0 / 3.0), o["max_trust_region_radius"]), 2.0
            step["func"] = abs(prev - cost) / (o["function_tolerance"] * prev)
            if abs(prev - cost) <= o["function_tolerance"] * prev:
                term = TERM["FUNCTION"]
        else:
            radius, df = radius / df, df * 2.0
            if radius < o["min_trust_region_radius"]:
                term = TERM["RADIUS_TOO_SMALL"]
        step.update(x=x.copy(), cost=cost, radius=radius, accepted=bool(np.array_equal(x, xc)))
        trace.append(step)
        if term != TERM["NO_CONVERGENCE"]:
            break
    return {"x": x, "iterations": it, "cost": cost, "termination": term, "trace": trace}


def pose_step_error(model, intr, board, corners, x_prev, x_next, mu, soft_l1_scale, opt=None):
    """backward error (Jacobi-scaled, as backward_error) of the step x_next - x_prev in one image's damped 6 x 6 system at
    x_prev, and its rounding floor -> (value, floor)"""
    o = dict(POSE_LM_DEFAULTS, **(opt or {}))
    r, J = _pose_rows(model, intr, board, corners, x_prev)
    w = soft_l1(r @ r, soft_l1_scale)[1]
    A, g = w * (J.T @ J), w * (J.T @ r)
    A = A + mu * np.diag(clamp_diag(np.diag(A), o))
    s = 1.0 / np.sqrt(np.diag(A))
    As, gs = A * s[:, None] * s[None, :], g * s
    d = (np.asarray(x_next, float) - x_prev) / s
    e = np.finfo(float).eps * np.abs(x_next) / s
    nd = np.linalg.norm(d)
    return float(np.linalg.norm(As @ d + gs) / (np.linalg.norm(As) * nd + np.linalg.norm(gs))), float(np.linalg.norm(e) / nd)
