"""Single Levenberg-Marquardt steps, and chains of two and three, of the solver's routes that tests/test_gpu_lm_steps.py cannot
reach: TransformationPrior blocks, sequences coupled by OdometryPrior / OdometryCost blocks, and solves over several ranks.
They are held to the full (dense) damped-normal-equation reference of tests/oracle_lm.py with the assertions of
tests/lm_check.py: the step's blockwise backward error at most BAR above its rounding floor, the exact success count, the cost
to 1e-12 beyond its floor, the radius to 1e-8, every compared decision far from min_relative_decrease, held / frozen columns
and constant poses still.

What is reached (vg_lm_host_loop.hpp, vg_solver_coupled.hpp, vg_comm.hpp):
  * a prior on a global transform: the host loop with the fused Schur rows, the prior added once after the sum (add_priors);
  * a prior on a sequence or odometry blocks: the coupled route -- vg_schur_rows_kernel for every pose, the host's
    block-tridiagonal elimination of the coupled elements (CoupledSeq::eliminate / backsub, the pose damping clamped from the
    diagonal with the odometry and prior terms, frozen elements, the OdometryCost pose-global coupling), and the Schur Gram
    of launch_dense_gram: vg_dense_gram_kernel<T> for T = ceil((G + 1) / 16) = 1 .. 4, vg_dense_gram_pair_kernel beyond;
  * several ranks in one process (the in-process communicator: vg_local_sum_slots_kernel / vg_scale_in_place_kernel), and
    the host all-reduce callback: the single-problem chain is the reference, every rank's global columns and replicated
    sequences are bitwise equal, the ranks' own poses assembled into one vector pass the step bar."""
import threading

import numpy as np
import pytest

from tests import golden_cases as G
from tests import lm_cases as C
from tests import lm_check as K
from tests import oracle_lm as L

pytestmark = pytest.mark.gpu

# (route, case, initial radii, SoftLOne scale, route the sizes select); a route named *_rejected must meet a rejected step
ROUTES = [
    ("prior_global_stereo", "stereo_prior", (1e4, 1.0, 1e16), 0.0, "host fused"),
    ("seq_prior_eucm", "mono_eucm_seq_prior", (1e4, 1.0, 1e16), 0.0, "coupled T=1"),
    ("seq_prior_mei_rejected", "mono_mei_seq_prior", (1e4, 1.0), 0.0, "coupled T=1"),
    ("seq_prior_12_poses", "mono_eucm_seq_prior_12", (1e4, 1e16), 0.0, "coupled T=1"),
    ("seq_prior_400_poses", "mono_eucm_seq_prior_400", (1e4,), 0.0, "coupled T=1"),
    ("handeye_lam005", "handeye_lam005", (1e4, 1.0, 1e16), 0.0, "coupled T=2"),
    ("handeye_lam1", "handeye_lam1", (1e4, 1e16), 0.0, "coupled T=2"),
    ("handeye_mid_anchor_unobserved", "handeye_mid_anchor", (1e4, 1.0), 0.0, "coupled T=2"),
    ("handeye_soft_l1", "handeye_lam005", (1e4, 1.0), 2.0, "coupled T=2"),
    ("handeye_240_poses", "handeye_240", (1e4,), 0.0, "coupled T=2"),
    ("wheeled_free_block", "wheeled", (1e4, 1.0), 0.0, "coupled T=2"),
    ("wheeled_constant_block", "wheeled_const", (1e4, 1.0), 0.0, "coupled T=2"),
    ("rig4_seq_prior_rejected", "rig4_seq_prior", (1e4, 1e16), 0.0, "coupled T=3"),
    ("rig_g63_seq_prior_rejected", "rig_g63_seq_prior", (1e4, 1e16), 0.0, "coupled T=4"),
    ("rig_g64_seq_prior_rejected", "rig_g64_seq_prior", (1e4, 1e16), 0.0, "coupled pair"),
    ("rig_mei8_seq_prior", "rig_mei8_seq_prior", (1e4,), 0.0, "coupled pair"),
]
# pose rows in one row group (vg_lm_solve.hpp rows_per_group): (route, fewest, most) row groups of 96 pose rows
GROUPS = {"seq_prior_12_poses": (1, 1), "seq_prior_400_poses": (16, None), "handeye_240_poses": (15, None)}


# the library's route rule, restated (vg_lm_solve.hpp setup_coupled, vg_solver_impl.hpp launch_dense_gram): a sequence with
# odometry blocks or a prior is eliminated on the host (the coupled route, unfused rows + dense Gram of T = ceil((G + 1) / 16)
# tiles, the pair kernel when G + 1 > 64); any prior or coupled sequence keeps the solve on the host loop
def expected_route(c, G_):
    seq_blocks = any(not c["transforms"][b[0]][0] for k in ("priors", "odometry_priors", "odometry_costs") for b in c.get(k, ()))
    if not seq_blocks:
        return "host fused" if c.get("priors") else "not host"
    return "coupled pair" if G_ + 1 > 64 else "coupled T=%d" % -(-(G_ + 1) // 16)


_WORST = {}


@pytest.fixture(scope="module")
def vg():
    import torch

    assert torch.cuda.is_available()
    import visgeom_amd

    return visgeom_amd


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for route, v in sorted(_WORST.items()):
        print("lm coupled steps %-34s worst backward error %.2e (rounding floor %.2e)  cost %.2e  radius %.2e" % ((route,) + tuple(v)))


@pytest.mark.parametrize("route,name,radii,a,kernel", ROUTES, ids=[r[0] for r in ROUTES])
def test_coupled_lm_steps_equal_the_full_damped_normal_equations(vg, route, name, radii, a, kernel):
    c = C.case(name)
    assert L.has_extras(c)

    def route_ok(what, s):
        assert expected_route(c, s["num_global_columns"]) == kernel, (what, s["num_global_columns"])
        if route in GROUPS:
            lo, hi = GROUPS[route]
            groups = -(-6 * s["num_pose_blocks"] // 96)
            assert groups >= lo and (hi is None or groups <= hi), (what, s["num_pose_blocks"])

    refs = []
    p = C.build_product_problem(vg, c)
    try:
        for R in radii:
            refs.append(K.check_chain(p, route, c, R, a, _WORST.setdefault(route, [0.0, 0.0, 0.0, 0.0]), route_ok))
    finally:
        p.close()
    if route.endswith("_rejected"):
        assert any(not it["success"] for ref in refs for it in ref), route


def test_wheeled_solves_do_not_fail(vg):
    """the planar wheeled set has a gauge direction (tests/test_gpu_solve.py): with the radii of the chains above (<= 1e4)
    the damped system stays regular, and a longer solve from the same start ends in neither FAILURE nor a bad pose block"""
    for name in ("wheeled", "wheeled_const"):
        c = C.case(name)
        p = C.build_product_problem(vg, c)
        try:
            for R in (1e4, 1.0):
                p.set_parameters(G.layout(c)[2])
                s = p.solve(max_num_iterations=20, initial_trust_region_radius=R)
                assert s["termination"] != "FAILURE" and "not positive definite" not in s["message"], (name, R, s["message"])
        finally:
            p.close()


# ---- several ranks: the single-problem chain is the reference
def _run_ranks(vg, cases, k, R, a, mode):
    """solve(max_num_iterations=k) of every rank's problem, each in its own thread and stream; mode "comm": the in-process
    communicator (Comm.local_group), "callback": the host all-reduce callback, summing in rank order behind a barrier.
    -> [(summary, parameters)]"""
    import torch

    from visgeom_amd import distributed as D

    n = len(cases)
    comms = D.Comm.local_group(n) if mode == "comm" else None
    barrier = threading.Barrier(n, timeout=300)
    slots = [None] * n
    out, err = [None] * n, [None] * n

    def make_allreduce(rank):
        def allreduce(buf):
            slots[rank] = buf.copy()
            barrier.wait()
            total = slots[0].copy()
            for q in slots[1:]:
                total += q
            barrier.wait()
            buf[:] = total
        return allreduce

    def worker(r):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                q = C.build_product_problem(vg, cases[r])
                try:
                    q.set_parameters(G.layout(cases[r])[2])
                    kw = {"comm": comms[r]} if mode == "comm" else {"allreduce": make_allreduce(r)}
                    s = q.solve(max_num_iterations=k, initial_trust_region_radius=R, soft_l1_scale=a, **kw)
                    out[r] = (s, q.get_parameters())
                finally:
                    q.close()
        except Exception as e:  # noqa: BLE001 -- reported by the main thread
            err[r] = e
            if mode != "comm":
                barrier.abort()
        finally:
            if comms is not None:
                comms[r].close()   # a rank that leaves breaks the group instead of leaving the others waiting

    th = [threading.Thread(target=worker, args=(r,)) for r in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not any(t.is_alive() for t in th), "a rank hangs"
    assert all(e is None for e in err), err
    return out


def _assemble(c, shards, res):
    """the full parameter vector from the ranks' vectors: the global columns from rank 0 (asserted bitwise equal on every
    rank), a replicated sequence from rank 0 (asserted bitwise equal on every rank), a split one from each rank's own
    elements"""
    _, tf_off, x0, _, _ = G.layout(c)
    t = next(t for t, (g, _) in enumerate(c["transforms"]) if not g)
    n_seq = np.asarray(c["transforms"][t][1]).size
    x_r0 = res[0][1]
    m0 = np.asarray(shards[0]["transforms"][t][1]).size
    glob0 = np.concatenate([x_r0[:tf_off[t]], x_r0[tf_off[t] + m0:]])
    parts = []
    for sc, (_, x) in zip(shards, res):
        m = np.asarray(sc["transforms"][t][1]).size
        assert np.array_equal(np.concatenate([x[:tf_off[t]], x[tf_off[t] + m:]]), glob0), "global columns differ between ranks"
        parts.append(x[tf_off[t]:tf_off[t] + m])
    replicated = all(q.size == n_seq for q in parts) and len(parts) > 1
    if replicated:
        assert all(np.array_equal(q, parts[0]) for q in parts), "a replicated sequence differs between ranks"
    x = x0.copy()
    x[:tf_off[t]] = glob0[:tf_off[t]]
    x[tf_off[t]:tf_off[t] + n_seq] = parts[0] if replicated else np.concatenate(parts)
    x[tf_off[t] + n_seq:] = glob0[tf_off[t]:]
    return x


def _stereo_tail(n=30, cut=18):
    """stereo, camera 2 sees frames 0 .. cut - 1 only: the second dataset is empty on a rank holding frames cut .."""
    c = C._stereo(n, missing=set(range(cut, n)))
    c["name"] = "stereo_tail"
    return c


MULTI = [   # (route, case, rank cuts (image ranges), radii, SoftLOne scale, all-reduce, loop the full case selects)
    ("device_fold_2_unequal", "mono_eucm", (0, 70, 300), (1e4, 1e16), 0.0, "comm", "device"),
    ("device_fold_3_unequal", "mono_eucm", (0, 40, 230, 300), (1e4,), 0.0, "comm", "device"),
    ("host_rig4_3_empty_rank_rejected", "rig4", (0, 13, 13, 24), (1e4, 1e16), 0.0, "comm", "host"),
    ("dataset_empty_on_one_rank", "stereo_tail", (0, 18, 30), (1e4, 1.0), 0.0, "comm", "device"),
    ("coupled_handeye_2", "handeye_lam005", (0, 7, 12), (1e4, 1.0), 0.0, "comm", "coupled"),
    ("coupled_handeye_3_no_images", "handeye_lam1", (0, 5, 5, 12), (1e4, 1e16), 0.0, "comm", "coupled"),
    ("callback_mono_2", "mono_eucm", (0, 120, 300), (1e4, 1.0), 0.0, "callback", "host"),
    ("callback_rig4_3", "rig4", (0, 9, 17, 24), (1e4, 1e16), 0.0, "callback", "host"),
    ("callback_prior_stereo_2", "stereo_prior", (0, 25, 60), (1e4,), 0.0, "callback", "host"),
]


def _multi_case(name):
    return _stereo_tail() if name == "stereo_tail" else C.case(name)


@pytest.mark.parametrize("route,name,cuts,radii,a,mode,loop", MULTI, ids=[m[0] for m in MULTI])
def test_multi_rank_lm_steps_equal_the_single_problem_chain(vg, route, name, cuts, radii, a, mode, loop):
    c = _multi_case(name)
    shards = C.shard(c, list(cuts))
    Gn = L.arrow_system(dict(c, datasets=[]), G.layout(c)[2])["gcols"].size
    # the loop the sizes select on one rank (test_gpu_lm_steps.expected_route, setup_coupled); the callback always takes
    # the host loop
    coupled = expected_route(c, Gn).startswith("coupled")
    want = "coupled" if coupled else ("device" if Gn <= 32 and not c.get("priors") and mode == "comm" else "host")
    assert want == loop, (route, want)
    opt_worst = _WORST.setdefault("ranks " + route, [0.0, 0.0, 0.0, 0.0])
    rejected = False
    for R in radii:
        ref = K.reference_chain(route, c, R, a)
        rejected |= any(not it["success"] for it in ref)
        opt = {"initial_trust_region_radius": R, "soft_l1_scale": a}
        x_prev, radius_prev = G.layout(c)[2], R
        for k in (1, 2, 3):
            res = _run_ranks(vg, shards, k, R, a, mode)
            what = (route, R, k)
            s0 = res[0][0]
            for s, _ in res:
                assert s["termination"] == "NO_CONVERGENCE", (what, s["message"])
                assert s["num_successful_steps"] == s0["num_successful_steps"] and s["final_radius"] == s0["final_radius"], what
                assert s["final_cost"] == s0["final_cost"], what
            x = _assemble(c, shards, res)
            for s, _ in res:
                K.check_iteration(what, c, a, opt, ref[k - 1], s, x, x_prev, radius_prev, opt_worst)
            x_prev, radius_prev = x, s0["final_radius"]
    if route.endswith("_rejected"):
        assert rejected, route
