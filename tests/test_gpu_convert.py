"""Conversion between camera models on the GPU (include/visgeom_amd.h section 20): the batched unprojection, the model-to-model maps
and the intrinsic fit against tests/convert_ref.py (numpy FP64 in the header's order, itself held to 50 digits by
tests/test_convert_cpu.py) and against scipy's Levenberg-Marquardt.

The cameras are synthetic.GT moved a little (intr_of), at 1280 x 800.  Bars: 1e-10 for rays (the project's parity bar), 1e-9 px for
the round trip through the reference's projection, one float32 spacing for map entries (an FP64 disagreement can only flip a
rounding), 1e-6 for converged values.

Shapes: pixel counts 1, 63, 64, 65, 257 (a lane, one less / exactly / one more than a wave, more than a workgroup); maps of 67 x 35
(narrower than a tile, odd width: element stores) and 260 x 5 (float4 stores, crosses the 256-pixel tile, a row count that is no
multiple of 4); fit grids of 63, 65, 256, 258 and 2560 samples.  Maps of 67 x 35 and 260 x 5 use the destination camera resampled to
that size (small_camera), so that the small map spans the camera's whole field of view."""
import numpy as np
import pytest

from tests import convert_ref as ref

pytestmark = pytest.mark.gpu

MODELS = ["eucm", "ucm", "mei", "kb", "ds"]
W, H = 1280, 800
TOL = 1e-10
MOVE = {"eucm": [0.01, -0.01, 3.0, -2.0, 1.5, -1.0],
        "ucm": [0.02, 3.0, -2.0, 1.5, -1.0],
        "mei": [0.02, 0.004, -0.002, 0.0007, -0.0001, 0.0003, 3.0, -2.0, 1.5, -1.0],
        "kb": [0.004, -0.002, 0.0007, -0.0001, 3.0, -2.0, 1.5, -1.0],
        "ds": [0.03, -0.02, 3.0, -2.0, 1.5, -1.0]}
SHOULDER = np.array([0.3, 2.2, -0.1])   # the rotation of test_rectify_map_against_the_reference_rounded_to_float32
GRIDS = [(9, 7), (13, 5), (16, 16), (43, 6), (64, 40)]
FIT_PAIRS = [("kb", "eucm"), ("ds", "eucm"), ("eucm", "kb")]
TIGHT = dict(function_tolerance=1e-15, gradient_tolerance=1e-15, parameter_tolerance=1e-15, max_iterations=500)


@pytest.fixture(scope="module")
def convert():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    from visgeom_amd import convert

    return convert


@pytest.fixture(scope="module")
def S():
    from visgeom_amd import synthetic

    return synthetic


def intr_of(S, model):
    """evaluation point: the ground truth moved a little (all distortion terms non-zero)"""
    return np.asarray(S.GT[model], float) + np.array(MOVE[model])


def small_camera(p, w, h):
    """the camera p of the 1280 x 800 image resampled to w x h: the whole field of view in a small map"""
    q = np.array(p, float)
    q[-4], q[-2] = q[-4] * w / W, q[-2] * w / W
    q[-3], q[-1] = q[-3] * h / H, q[-1] * h / H
    return q


# ------------------------------------------------------------------------------------------ unprojection
def pixel_list(p, n):
    """n pixels: the principal point, the image corners, pixels far outside every model's domain, NaN and infinite ones, padded
    with random pixels of the image"""
    rng = np.random.default_rng(17 + n)
    special = [[p[-2], p[-1]], [0, 0], [W - 1, H - 1], [W - 1, 0], [0, H - 1], [1e5, 1e5], [np.nan, 10.0], [-3e4, 7e4], [np.inf, 5.0],
               [6e3, 400.0], [3.0, -np.inf], [640.0, -5e3], [np.nan, np.nan], [640.25, 399.75]]
    special = np.array(special[:n], float)
    pad = np.column_stack([rng.uniform(0, W - 1, n - len(special)), rng.uniform(0, H - 1, n - len(special))])
    return np.concatenate([special, pad])


def assert_off_the_boundary(model, p, uv):
    """no finite pixel within 1e-6 px of the boundary of the model's domain: the reference's discriminant keeps its sign, and stays
    away from zero, when the pixel moves 1e-6 px towards the centre or away from it"""
    fin = np.isfinite(uv).all(-1)
    q = uv[fin]
    d = q - p[-2:]
    nrm = np.hypot(d[:, 0], d[:, 1])
    d = np.where(nrm[:, None] > 0, d / np.where(nrm > 0, nrm, 1.)[:, None], [1.0, 0.0])
    m0 = ref.domain_margin(model, p, q)
    for s in (-1e-6, 1e-6):
        m1 = ref.domain_margin(model, p, q + s * d)
        assert np.all(m0 != 0) and np.all(np.sign(m1) == np.sign(m0)), (model, q[np.sign(m1) != np.sign(m0)])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("model", MODELS)
def test_unproject_against_the_reference(convert, S, model, n):
    p = intr_of(S, model)
    uv = pixel_list(p, n)
    assert_off_the_boundary(model, p, uv)
    want, ok = ref.unproject_unit(model, p, uv)
    assert 2 * ok.sum() >= n
    rays, got_ok = convert.unproject(model, p, uv)
    assert rays.shape == (n, 3) and got_ok.shape == (n,)
    rays, got_ok = rays.cpu().numpy(), got_ok.cpu().numpy().astype(bool)
    assert np.array_equal(got_ok, ok), (model, uv[got_ok != ok])
    assert np.all(rays[~ok] == 0)
    err = np.max(np.abs(rays - want))
    back, okp = ref.project(model, p, rays[ok])
    assert okp.all()
    trip = np.max(np.abs(back - uv[ok]))
    print(model, n, "valid %d, worst |ray - reference| %.3e, round trip %.3e px" % (int(ok.sum()), err, trip))
    assert err <= TOL
    assert np.max(np.abs(np.linalg.norm(rays[ok], axis=1) - 1.0)) <= 1e-14
    assert trip <= 1e-9


def test_unproject_takes_a_device_tensor_and_an_empty_batch(convert, S):
    import torch

    p = intr_of(S, "mei")
    uv = pixel_list(p, 65)
    a, oka = convert.unproject("mei", p, uv)
    b, okb = convert.unproject("mei", p, torch.from_numpy(uv).cuda())
    assert torch.equal(a, b) and torch.equal(oka, okb)
    r, ok = convert.unproject("mei", p, np.zeros((0, 2)))
    assert r.shape == (0, 3) and ok.shape == (0,)


# ------------------------------------------------------------------------------------------ maps
def check_map(convert, S, dst, src, w, h, rotvec):
    from oracle import vgo

    pd, ps = small_camera(intr_of(S, dst), w, h), intr_of(S, src)
    mx, my = convert.convert_maps(dst, pd, src, ps, (w, h), rotvec=rotvec)
    assert mx.shape == (h, w) and my.shape == (h, w)
    mx, my = mx.cpu().numpy(), my.cpu().numpy()
    assert mx.dtype == np.float32
    R = None if rotvec is None else vgo.rotation_matrix(np.asarray(rotvec, float)).reshape(3, 3)
    wx, wy, ok, _ = ref.convert_maps(dst, pd, src, ps, (w, h), R)
    for got, want in ((mx, wx), (my, wy)):
        assert np.all(got[~ok] == -1.0), (dst, src)
        assert np.all(np.abs(got[ok] - want[ok]) <= np.spacing(np.abs(want[ok]))), (dst, src)
    return ok


@pytest.mark.parametrize("src", MODELS)
@pytest.mark.parametrize("dst", MODELS)
def test_map_of_every_pair_against_the_reference(convert, S, dst, src):
    """67 x 35, the destination looks over a shoulder: an EUCM or double-sphere source does not see part of the map (UCM and Mei
    never report a failed projection, Kannala-Brandt sees everything but the ray pointing exactly backwards); a UCM, Mei or
    double-sphere destination has pixels outside its own domain"""
    ok = check_map(convert, S, dst, src, 67, 35, SHOULDER)
    print(dst, "<-", src, "valid %d of %d" % (int(ok.sum()), ok.size))
    assert ok.sum() > ok.size // 2
    if src in ("eucm", "ds") or dst in ("ucm", "mei", "ds"):
        assert (~ok).sum() > 50


@pytest.mark.parametrize("dst,src", [("eucm", "kb"), ("kb", "eucm"), ("ds", "mei"), ("mei", "ds"), ("ucm", "ucm")])
def test_map_on_the_float4_path(convert, S, dst, src):
    ok = check_map(convert, S, dst, src, 260, 5, np.array([0.02, -0.3, 0.01]))
    assert ok.sum() > ok.size // 2


@pytest.mark.parametrize("model", MODELS)
def test_map_of_a_camera_onto_itself_is_the_pixel_grid(convert, S, model):
    """no rotation, the same intrinsics: wherever the reference says valid the map is the pixel itself.  The FP64 round trip is
    good to 1e-9 px (the bar of the unprojection tests); rounded to float32 that is one spacing of the pixel coordinate, and 1e-9 px
    where the coordinate is 0"""
    w, h = 67, 35
    p = small_camera(intr_of(S, model), w, h)
    mx, my = convert.convert_maps(model, p, model, p, (w, h))
    _, _, ok, _ = ref.convert_maps(model, p, model, p, (w, h))
    j, i = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    assert ok.sum() > ok.size // 2
    for got, want in ((mx.cpu().numpy(), j), (my.cpu().numpy(), i)):
        assert np.all(got[~ok] == -1.0)
        assert np.all(np.abs(got[ok] - want[ok]) <= np.maximum(np.spacing(want[ok]), 1e-9))


def test_maps_feed_remap_unchanged(convert, S):
    """a Kannala-Brandt image resampled into the EUCM fitted to it, then back.  The two maps are inverse to each other whatever the
    fit's residual, so away from the border the image returns up to two bilinear interpolations: each is off by at most
    h^2 / 8 (|f_xx| + |f_yy|) = (50 / 81 + 50 / 49) / 8 = 0.2 grey levels at unit magnification"""
    import torch

    from visgeom_amd.rectify import remap

    w, h = 160, 100
    kb = small_camera(intr_of(S, "kb"), w, h)
    eucm, s = convert.fit("kb", kb, (w, h), "eucm")
    j, i = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    img = torch.from_numpy((100 + 50 * np.sin(j / 9) * np.cos(i / 7)).astype(np.float32)).cuda()
    there = remap(img, *convert.convert_maps("eucm", eucm, "kb", kb, (w, h)), fill=-1)
    back = remap(there, *convert.convert_maps("kb", kb, "eucm", eucm, (w, h)), fill=-1)
    err = (back - img).abs()[10:-10, 10:-10].max().item()
    print("fit rms %.3f px, there-and-back error %.3f grey levels" % (s["rms"], err))
    assert err < 2.0   # 2 x 0.2, with room for the magnification between the two cameras (below 2 in the cropped region)


# ------------------------------------------------------------------------------------------ fit
def reference_problem(S, src, grid, max_angle=np.pi):
    rays, uv, dropped = ref.fit_samples(src, intr_of(S, src), (W, H), grid, max_angle)
    return rays, uv, dropped


def fun_jac(dst, rays, uv):
    def fun(p):
        r, _, ok = ref.fit_residual_jacobian(dst, p, rays, uv, want_jac=False)
        return np.where(np.repeat(ok, 2), r, 1e3)

    def jac(p):
        return ref.fit_residual_jacobian(dst, p, rays, uv)[1]

    return fun, jac


@pytest.mark.parametrize("grid", GRIDS)
def test_fit_ucm_to_eucm_reaches_the_closed_form(convert, S, grid):
    """EUCM holds UCM exactly: alpha = xi / (1 + xi), beta = 1, f / (1 + xi)"""
    p = intr_of(S, "ucm")
    xi, fu, fv, u0, v0 = p
    truth = np.array([xi / (1 + xi), 1.0, fu / (1 + xi), fv / (1 + xi), u0, v0])
    x, s = convert.fit("ucm", p, (W, H), "eucm", grid_w=grid[0], grid_h=grid[1], **TIGHT)
    rays, uv, dropped = reference_problem(S, "ucm", grid)
    err = np.max(np.abs(x - truth) / np.maximum(1.0, np.abs(truth)))
    print(grid, s, "error %.3e" % err)
    assert (s["kept"], s["dropped"]) == (len(rays), dropped)
    assert err <= 1e-6


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("src,dst", FIT_PAIRS)
def test_fit_against_the_reference_and_scipy(convert, S, src, dst, grid):
    from scipy.optimize import least_squares

    p = intr_of(S, src)
    x, s = convert.fit(src, p, (W, H), dst, grid_w=grid[0], grid_h=grid[1], **TIGHT)
    rays, uv, dropped = reference_problem(S, src, grid)
    n = grid[0] * grid[1]
    assert (s["kept"], s["dropped"]) == (len(rays), dropped)
    assert 4 * s["kept"] >= 3 * n
    x0 = ref.default_start(src, p, dst)
    assert np.array_equal(x0, convert.default_start(src, p, dst))
    cost0, g0, ok0 = ref.fit_cost_gradient(dst, x0, rays, uv)
    cost, g, ok = ref.fit_cost_gradient(dst, x, rays, uv)
    assert ok0.all() and ok.all()
    fun, jac = fun_jac(dst, rays, uv)
    r = least_squares(fun, x0, jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=4000)
    res = fun(x).reshape(-1, 2)
    print(src, "->", dst, grid, s, "reference cost %.12e scipy %.12e  |g| %.3e of %.3e" % (cost, r.cost, np.max(np.abs(g)), np.max(np.abs(g0))))
    assert abs(s["initial_cost"] - cost0) <= 1e-9 * cost0
    assert abs(s["final_cost"] - cost) <= 1e-9 * cost
    assert np.max(np.abs(g)) <= 1e-6 * np.max(np.abs(g0))
    assert s["final_cost"] <= r.cost * (1 + 1e-6)
    assert abs(s["rms"] - np.sqrt(np.mean(np.sum(res ** 2, 1)))) <= 1e-9 * max(1.0, s["rms"])
    assert abs(s["max_residual"] - np.max(np.hypot(res[:, 0], res[:, 1]))) <= 1e-9 * max(1.0, s["max_residual"])
    assert s["iterations"] >= 1


def test_fit_max_angle_drops_what_the_reference_drops(convert, S):
    p = intr_of(S, "kb")
    limit = np.radians(95.0)
    rays, uv, dropped = reference_problem(S, "kb", (64, 40), limit)
    _, _, dropped_all = reference_problem(S, "kb", (64, 40))
    x, s = convert.fit("kb", p, (W, H), "eucm", max_angle=limit)
    print("95 degrees:", s)
    assert dropped > dropped_all and (s["kept"], s["dropped"]) == (len(rays), dropped)
    xa, sa = convert.fit("kb", p, (W, H), "eucm")
    assert sa["dropped"] == dropped_all and s["rms"] < sa["rms"]   # the rim is what EUCM cannot follow


def test_fit_twice_gives_the_same_bits(convert, S):
    p = intr_of(S, "ds")
    a, sa = convert.fit("ds", p, (W, H), "eucm", **TIGHT)
    b, sb = convert.fit("ds", p, (W, H), "eucm", **TIGHT)
    assert a.tobytes() == b.tobytes()
    assert all(np.array(sa[k]).tobytes() == np.array(sb[k]).tobytes() for k in sa)
    c, sc = convert.fit("ds", p, (W, H), "eucm", start=convert.default_start("ds", p, "eucm"), **TIGHT)
    assert a.tobytes() == c.tobytes()   # no start = the default start


def test_fit_refuses_a_start_that_cannot_see_a_sample(convert, S):
    from visgeom_amd import capi

    p = intr_of(S, "kb")
    start = convert.default_start("kb", p, "eucm")
    start[:2] = [0.9, 4.0]   # a narrow cone: Kannala-Brandt's rays beyond it do not project
    rays, uv, _ = reference_problem(S, "kb", (64, 40))
    _, ok = ref.project("eucm", start, rays)
    assert not ok.all()
    with pytest.raises(capi.VisgeomError) as e:
        convert.fit("kb", p, (W, H), "eucm", start=start)
    assert e.value.code == capi.ERR_NUMERIC
    assert "sample %d " % int(np.nonzero(~ok)[0][0]) in str(e.value), str(e.value)


@pytest.mark.parametrize("dst,grid", [("eucm", (2, 1)), ("eucm", (1, 1)), ("mei", (2, 2)), ("ucm", (1, 2))])
def test_fit_refuses_fewer_residuals_than_parameters(convert, S, dst, grid):
    from visgeom_amd import capi

    with pytest.raises(capi.VisgeomError) as e:
        convert.fit("kb", intr_of(S, "kb"), (W, H), dst, grid_w=grid[0], grid_h=grid[1])
    assert e.value.code == capi.ERR_INVALID_ARGUMENT and "samples kept" in str(e.value)


def test_fit_with_exactly_enough_samples_runs(convert, S):
    x, s = convert.fit("kb", intr_of(S, "kb"), (W, H), "eucm", grid_w=3, grid_h=1)   # 6 residuals, 6 parameters
    assert s["kept"] == 3 and np.isfinite(x).all()
