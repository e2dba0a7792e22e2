"""Photometric bundle adjustment on the GPU (vg_dense_ba_*, visgeom_amd.dense_ba) against the restatement (tests/dense_ba_ref.py)
on the inputs of tests/dense_ba_scene.py: the pack in order, the rows, the per-frame sums and the reduced system to 1e-10 with
their determinism, the launch shapes, the reference's own settings, the back-substitution, the solve against the restatement's
own solve, the output maps and the refusals.

The solve is not compared iterate by iterate: the cost is C1 only (the bicubic sampler) and has many shallow minima under 3 %
depth noise, so two correct solvers may walk differently.  The restatement alone, from start_poses(F, 0.1) and from 0.9 x and
1.1 x that offset, at the default function tolerance 1e-6:
  F = 2  49 / 49 / 38 iterations, all ended by the function tolerance
         final cost 6970.0866 / 6970.0086 / 6969.3573                     spread 1.05e-4 relative
         pose error 0.2977 / 0.2993 / 0.2766 mm, 0.1411 / 0.1409 / 0.1182 mrad   spread 7.6 % / 16.2 %
         median relative depth error 1.11331 / 1.11225 / 1.11399 %        spread 1.6e-3 relative   (start: 2.8 mm, 0.88 mrad, 2.008 %)
  F = 3  46 / 44 / 38 iterations, function tolerance
         final cost 8607.4469 / 8607.4777 / 8608.5079                     spread 1.23e-4
         pose error 0.2293 / 0.2347 / 0.2543 mm, 0.1066 / 0.1094 / 0.1226 mrad   spread 10.7 % / 14.6 %
         median relative depth error 0.87964 / 0.88014 / 0.87972 %        spread 5.7e-4
A function tolerance of 1e-10 was tried and does not narrow this: every start then runs into the cap of 150 iterations and the
three final costs still differ by 4e-5 relative, the pose errors by 7 % -- the spread is the landscape's, not the stopping
rule's.  So the test runs at the default tolerance and the margins are ten spreads of the wider of the two cases."""
import numpy as np
import pytest

from tests import dense_ba_ref as br
from tests import dense_ba_scene as bs
from tests import photometric_scene as ps

pytestmark = pytest.mark.gpu
PARITY = 1e-10   # the project's parity bar, relative to max |.| per array
COST_MARGIN, TRANS_MARGIN, ROT_MARGIN, DEPTH_MARGIN, POSE_FLOOR = 1.23e-3, 1.07, 1.62, 1.6e-2, 1e-6
LD = np.longdouble


@pytest.fixture(scope="module")
def torch():
    import torch

    from visgeom_amd import _build

    _build.build()
    return torch


def params(prm):
    from visgeom_amd import stereo

    return stereo.make_params(equal_margins=0, **prm)


def make(torch, problem, F, prm=ps.PRM, **options):
    """a handle on the restatement's inputs"""
    from visgeom_amd import dense_ba

    opt = dense_ba.make_options(**options) if options else None
    h = dense_ba.DenseBA(ps.CAM, params(prm), ps.XI_BASE_CAM, ps.W, ps.H, opt)
    sigma = torch.from_numpy(problem.sigma_map).cuda() if problem.sigma_map is not None else None
    h.set_base(torch.from_numpy(ps.scene()["base"]).cuda(), torch.from_numpy(problem.depth_map).cuda(), sigma)
    h.set_frames(torch.from_numpy(bs.frames(F)).cuda())
    return h


@pytest.fixture(scope="module")
def handles(torch):
    """the solve case with F = 1, 2, 3 and 8 frames, made on first use"""
    made = {}

    def get(F):
        if F not in made:
            made[F] = make(torch, bs.problem(F), F)
        return made[F]

    yield get
    for h in made.values():
        h.close()


def close(got, want, what, scale=None):
    got, want = np.asarray(got, float), np.asarray(want, float)
    scale = float(np.abs(want).max()) if scale is None else float(scale)
    err = float(np.abs(got - want).max())
    print(what, "max error", err, "scale", scale)
    assert err <= PARITY * scale, what


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def check_rows(out, r):
    """every point: the three row arrays, zero rows exactly where the restatement's projection fails"""
    res, jp, jd = (out[k].cpu().numpy() for k in ("residuals", "jac_pose", "jac_depth"))
    fail = ~r["ok"]
    assert (res[fail] == 0.).all() and (jp[fail] == 0.).all() and (jd[fail] == 0.).all()
    assert ((jp != 0.).any(-1) == (r["jp"] != 0.).any(-1)).all()
    close(res, r["res"], "residuals")
    close(jp, r["jp"], "pose rows")
    close(jd, r["jd"], "depth entries")
    close(out["a"].cpu().numpy(), r["a"], "a")
    close(out["g_depth"].cpu().numpy(), r["gd"], "g_d")


def check_reduce(h, r, mus=(1e-4, 1.)):
    """S and rhs against longdouble sums of the restatement's rows.  S is relative to the largest entry of H_pp; rhs = g_p - sum
    is a difference of two sums of the size of g_p, so it is relative to the largest entry of g_p."""
    H, g, _ = br.Problem.normal(r, LD)
    for mu in mus:
        S, rhs = h.reduce(mu)
        Sr, rr, _, _ = br.Problem.reduce(r, mu, LD)
        close(S, Sr.astype(float), "S mu=%g" % mu, np.abs(H).max())
        close(rhs, rr.astype(float), "rhs mu=%g" % mu, np.abs(g).max())
        assert (S == S.T).all()
        S2, rhs2 = h.reduce(mu)
        assert same_bits(S, S2) and same_bits(rhs, rhs2)


def test_pack(torch):
    """photometric_scene's depth map: holes, far values (kept: there is no distance limit here), values below MIN_DEPTH; a sigma
    map with entries that are 0, negative and NaN"""
    p = bs.problem(2, which="pack")
    depth, sigma = bs.pack_maps()
    assert (depth == 0.).any() and (depth == 60.).any() and (depth == 0.1).any()
    assert (sigma == 0.).any() and (sigma < 0.).any() and np.isnan(sigma).any()
    h = make(torch, p, 2)
    idx, val, dirs, d0, s0 = [t.cpu().numpy() for t in h.pack()]
    h.close()
    want = p.pack
    assert 1000 < len(want["idx"]) == len(idx) and idx.tolist() == want["idx"].tolist()
    assert (d0 == 60.).any()
    for got, key in ((val, "val"), (dirs, "dir"), (d0, "d0"), (s0, "s0")):
        assert np.abs(got - want[key]).max() <= 1e-12 * np.abs(want[key]).max(), key
    assert np.abs(np.linalg.norm(dirs, axis=1) - 1.).max() <= 1e-14


def test_rows(torch, handles):
    """F = 3 at the start poses.  The five pack points nearest the principal point get the depth -1: behind the camera, where
    projectPoint passes its first test (eta about 0.2 against 1e-3) and fails its second (z / eta about -5 against (alpha - 1) /
    (2 alpha - 1) = -2), far from both thresholds, so the restatement alone decides that they fail."""
    p, h = bs.problem(3), handles(3)
    cell = p.pack["idx"]
    u, v = (cell % ps.PRM["x_max"]) * ps.PRM["scale"] + ps.PRM["u0"], (cell // ps.PRM["x_max"]) * ps.PRM["scale"] + ps.PRM["v0"]
    near = np.argsort((u - ps.CAM[4]) ** 2 + (v - ps.CAM[5]) ** 2, kind="stable")[:5]
    d = p.pack["d0"].copy()
    d[near] = -1.
    r = p.rows(bs.start_poses(3), d)
    for f in r["frames"]:
        assert not f["ok"][near].any() and (f["eta"][near] > 0.1).all() and (f["zn"][near] < -3.).all()
        others = np.delete(np.arange(len(d)), near)
        assert f["ok"][others].all()
        assert (np.abs(f["eta"][others] - 1e-3) > 1e-2).all() and (np.abs(f["zn"][others] + 2.) > 1e-2).all()
    out = h.evaluate(bs.start_poses(3), torch.from_numpy(d).cuda())
    check_rows(out, r)
    again = h.evaluate(bs.start_poses(3), torch.from_numpy(d).cuda())
    for k in ("residuals", "jac_pose", "jac_depth", "a", "g_depth"):
        assert same_bits(out[k].cpu().numpy(), again[k].cpu().numpy()), k


@pytest.mark.parametrize("F", [1, 2, 3, 8])
def test_sums_and_reduce(torch, handles, F):
    """F = 8 uses the three targets cyclically at different poses"""
    p, h = bs.problem(F), handles(F)
    xi = bs.start_poses(F)
    assert len({tuple(x) for x in xi}) == F
    r = p.rows(xi)
    out = h.evaluate(xi)
    check_rows(out, r)
    H, g, _ = br.Problem.normal(r, LD)
    cost = 0.5 * float((r["res"].astype(LD) ** 2).sum() + (r["p"].astype(LD) ** 2).sum())
    print("cost", out["cost"], cost)
    assert abs(out["cost"] - cost) <= PARITY * cost
    for f in range(F):
        blk = H[6 * f:6 * f + 6, 6 * f:6 * f + 6].astype(float)
        close(out["sums"][f, :21], blk[np.triu_indices(6)], "J^T J frame %d" % f)
        close(out["sums"][f, 21:27], g[6 * f:6 * f + 6].astype(float), "J^T r frame %d" % f)
    check_reduce(h, r)
    again = h.evaluate(xi, rows=False)
    assert again["cost"] == out["cost"] and same_bits(again["sums"], out["sums"])


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 1024])
def test_launch_shapes(torch, m):
    """packs of exactly m points, F = 2: below, at and above a wave and a workgroup"""
    p = bs.exact(m)
    h = make(torch, p, 2)
    assert h.count == m
    xi = bs.start_poses(2)
    r = p.rows(xi)
    check_rows(h.evaluate(xi), r)
    check_reduce(h, r)
    h.close()


def test_launch_shape_of_the_whole_image(torch):
    """the scale-1 grid with grad_thresh 0: 49 152 points, 192 workgroups of 256 for the rows.  The reduce gives a workgroup 256 C
    points, C the smallest that keeps it at 128 workgroups or fewer: up to 32 768 points C is 1 (the packs above), here C is 2 --
    96 workgroups of 512 points, 384 partial tile sets in the final pass."""
    p = bs.problem(2, bs.PRM1, grad_thresh=0.)
    h = make(torch, p, 2, bs.PRM1, grad_thresh=0.)
    assert h.count == 49152 == len(p.pack["idx"]) > 128 * 256
    xi = bs.start_poses(2)
    r = p.rows(xi)
    check_rows(h.evaluate(xi), r)
    check_reduce(h, r)
    h.close()


def test_the_references_settings(torch):
    """dense_ba_test's own problem on the scale-1 grid: no prior, every cell, greys over 255 -- rows and reduce only (its solve
    diverges).  Textureless cells have a below the 1e-6 clamp of D."""
    p = bs.problem(2, bs.PRM1, **br.REFERENCE)
    h = make(torch, p, 2, bs.PRM1, **br.REFERENCE)
    assert h.count == 49152
    xi = bs.start_poses(2)
    r = p.rows(xi)
    assert (r["a"] < 1e-6).any() and (r["p"] == 0.).all()
    check_rows(h.evaluate(xi), r)
    check_reduce(h, r)
    h.close()


def test_back_substitution(torch, handles):
    """from the library's S, rhs and mu a numpy pose step; the candidate depths and the depth block's share of the rule's sums.
    g . dd is a sum of terms of either sign: relative to sum |g dd|."""
    p, h = bs.problem(3), handles(3)
    xi = bs.start_poses(3)
    r = p.rows(xi)
    h.evaluate(xi, rows=False)
    for mu in (1e-4, 1.):
        S, rhs = h.reduce(mu)
        dp = -np.linalg.solve(S, rhs)
        cand, tail = h.back_substitute(mu, dp)
        dd, want = br.Problem.back_substitute(r, mu, dp, LD)
        close(cand.cpu().numpy(), (r["depths"].astype(LD) + dd).astype(float), "candidate depths mu=%g" % mu)
        close(cand.cpu().numpy() - r["depths"], dd.astype(float), "depth step mu=%g" % mu)
        scales = [want[0], np.abs(r["gd"].astype(LD) * dd).sum(), want[2], want[3], want[4]]
        for k in range(5):
            close(tail[k], float(want[k]), "tail %d mu=%g" % (k, mu), float(scales[k]))
        cand2, tail2 = h.back_substitute(mu, dp)
        assert same_bits(tail, tail2) and same_bits(cand.cpu().numpy(), cand2.cpu().numpy())


@pytest.fixture(scope="module")
def solved(torch, handles):
    made = {}

    def get(F):
        if F not in made:
            made[F] = handles(F).solve(bs.start_poses(F))
        return made[F]

    return get


@pytest.mark.parametrize("F", [2, 3])
def test_solve_against_the_restatement(torch, handles, solved, F):
    """see the module's header: the restatement's cost at the library's result within 1.23e-3 of the restatement's own final cost,
    the pose errors within 107 % / 162 % plus 1e-6, the median relative depth error within 1.6 % of the restatement's"""
    p, h = bs.problem(F), handles(F)
    ref_x, ref_d, _, ref_rep = bs.reference_solve(F)
    x, depth, sigma, rep = solved(F)
    d = depth.cpu().numpy().ravel()[p.pack["idx"]]
    cost_at = p.cost(x, d)
    (et, er, ed), (rt, rr, rd) = bs.errors(x, d, p.pack), bs.errors(ref_x, ref_d, p.pack)
    print("library", rep.tolist(), "cost by the restatement", cost_at, "errors", et, er, ed)
    print("restatement", ref_rep, "errors", rt, rr, rd)
    assert cost_at <= ref_rep["final_cost"] * (1. + COST_MARGIN)
    assert et <= rt * (1. + TRANS_MARGIN) + POSE_FLOOR and er <= rr * (1. + ROT_MARGIN) + POSE_FLOOR
    assert ed <= rd * (1. + DEPTH_MARGIN)
    assert 1 <= rep[0] <= br.DEFAULTS["max_iterations"] and rep[2] < rep[1] and rep[3] in (0, 1, 2)
    assert abs(rep[1] - ref_rep["initial_cost"]) <= PARITY * rep[1] and abs(rep[2] - cost_at) <= PARITY * cost_at
    x2, depth2, sigma2, rep2 = h.solve(bs.start_poses(F))
    assert same_bits(x, x2) and same_bits(rep, rep2)
    assert same_bits(depth.cpu().numpy(), depth2.cpu().numpy()) and same_bits(sigma.cpu().numpy(), sigma2.cpu().numpy())


def test_outputs(torch, handles, solved):
    """the maps keep the input's bits outside the pack; inside they hold the final depths -- an evaluation there has the
    report's final cost, bit for bit -- and 1 / sqrt(a) at the solution"""
    p, h = bs.problem(2), handles(2)
    x, depth, sigma, rep = solved(2)
    depth, sigma = depth.cpu().numpy(), sigma.cpu().numpy()
    outside = np.ones(depth.size, bool)
    outside[p.pack["idx"]] = False
    assert outside.sum() > 1000
    assert same_bits(depth.ravel()[outside], p.depth_map.ravel()[outside]) and same_bits(sigma.ravel()[outside], p.sigma_map.ravel()[outside])
    d = depth.ravel()[p.pack["idx"]]
    assert np.isfinite(d).all() and (d != p.pack["d0"]).mean() > 0.99
    out = h.evaluate(x, torch.from_numpy(np.ascontiguousarray(d)).cuda())
    assert out["cost"] == rep[2]
    a = out["a"].cpu().numpy()
    assert np.abs(sigma.ravel()[p.pack["idx"]] - 1. / np.sqrt(a)).max() <= 1e-14 * (1. / np.sqrt(a)).max()
    close(a, p.rows(x, d)["a"], "a at the solution")


def test_refusals(torch, handles):
    from visgeom_amd import capi, dense_ba

    def refused(fn, code):
        with pytest.raises(capi.VisgeomError) as e:
            fn()
        assert e.value.code == code, e.value

    p = bs.problem(2)
    xi = bs.start_poses(2)
    fresh = dense_ba.DenseBA(ps.CAM, params(ps.PRM), ps.XI_BASE_CAM, ps.W, ps.H)
    refused(lambda: fresh.solve(xi), capi.ERR_STATE)                       # before set_base
    refused(lambda: fresh.pack(), capi.ERR_STATE)
    base = torch.from_numpy(ps.scene()["base"]).cuda()
    refused(lambda: fresh.set_base(base, torch.from_numpy(p.depth_map).cuda()), capi.ERR_INVALID_ARGUMENT)   # a prior without a sigma map
    fresh.set_base(base, torch.from_numpy(p.depth_map).cuda(), torch.from_numpy(p.sigma_map).cuda())
    refused(lambda: fresh.solve(xi), capi.ERR_STATE)                       # before set_frames
    refused(lambda: fresh.evaluate(xi, rows=False), capi.ERR_STATE)
    with pytest.raises(capi.VisgeomError):
        fresh.set_frames(torch.from_numpy(bs.frames(9)).cuda())            # nine frames
    fresh.set_frames(torch.from_numpy(bs.frames(2)).cuda())
    refused(lambda: fresh.reduce(1.), capi.ERR_STATE)                      # before evaluate
    refused(lambda: fresh.back_substitute(1., np.zeros(12)), capi.ERR_STATE)
    fresh.evaluate(xi, rows=False)
    refused(lambda: fresh.reduce(0.), capi.ERR_INVALID_ARGUMENT)
    refused(lambda: fresh.evaluate(np.full((2, 6), np.nan), rows=False), capi.ERR_INVALID_ARGUMENT)
    fresh.close()
    refused(lambda: fresh.solve(xi), capi.ERR_INVALID_ARGUMENT)            # a handle used after close
    refused(lambda: fresh.reduce(1.), capi.ERR_INVALID_ARGUMENT)
