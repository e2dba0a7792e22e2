"""Rectification on the GPU (vg_rectify_map, vg_remap, visgeom_amd.rectify, the `rectify` program): the maps against the
oracle's projectPoint and a vectorised restatement, the remap against its float32 restatement (tests/rectify_ref.py), batch
equivalence, identity, an end-to-end checkerboard and a launch past 2^31 bytes."""
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

from tests import rectify_ref

pytestmark = pytest.mark.gpu

EUCM, UCM, MEI = 0, 1, 2
# (model, intrinsics, pinhole [w, h, u0, v0, f], xi): for every model 2-3 sets; EUCM with alpha > 0.5 and a pinhole wide enough
# that part of its field fails to project
CASES = [
    (EUCM, [0.6, 1.1, 250., 252., 320.5, 240.25], [160, 120, 79.5, 59.5, 60.], [0.01, -0.02, 0.005, 0.02, -0.03, 0.01]),
    (EUCM, [0.85, 1.3, 180., 181., 300., 200.], [160, 120, 80., 60., 12.], [0., 0., 0., 0.3, 0.6, 0.]),
    (EUCM, [0.3, 0.9, 400., 398., 640., 480.], [160, 120, 81., 58., 90.], [0., 0., 0., 0., 0., 0.]),
    (UCM, [0.9, 280., 281., 320., 240.], [160, 120, 80., 60., 40.], [0.02, 0.01, -0.01, -0.1, 0.05, 0.02]),
    (UCM, [1.4, 300., 300., 330., 250.], [160, 120, 80., 60., 10.], [0., 0., 0., 0., 0., 0.]),
    (MEI, [0.8, -0.2, 0.05, -0.01, 0.001, -0.002, 260., 261., 320., 240.], [160, 120, 80., 60., 50.],
     [0.01, 0.02, 0.0, 0.05, -0.02, 0.1]),
    (MEI, [1.1, 0.1, -0.02, 0.0, 0.0, 0.0, 300., 300., 640., 360.], [160, 120, 79., 61., 80.], [0., 0., 0., 0., 0., 0.]),
]


@pytest.fixture(scope="module")
def torch():
    import torch

    from visgeom_amd import _build

    _build.build()
    return torch


def _rot(xi):
    from oracle import vgo

    return vgo.rotation_matrix(np.asarray(xi[3:], np.float64)), np.asarray(xi[:3], np.float64)


def _ulp_diff(a, b):
    """distance in float32 units in the last place (same-sign finite values)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def _check_maps(gx, gy, rx, ry):
    fail_g, fail_r = (gx == -1) & (gy == -1), (rx == -1) & (ry == -1)
    assert np.array_equal(fail_g, fail_r), "failed projections differ at %d pixels" % (fail_g != fail_r).sum()
    ok = ~fail_r
    for g, r in ((gx, rx), (gy, ry)):
        g, r = g[ok], r[ok]
        fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(g), fin)
        d = _ulp_diff(g[fin], r[fin])
        assert d.max(initial=0) <= 1, d.max()
        assert (d == 0).mean() >= 0.999 if d.size else True
    return fail_r.sum()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_map_parity_vs_oracle(torch, case):
    from oracle import vgo
    from visgeom_amd import rectify

    model, intr, pin, xi = CASES[case]
    gx, gy = (t.cpu().numpy() for t in rectify.rectify_maps(model, intr, pin, xi))
    assert gx.shape == (pin[1], pin[0])
    R, t = _rot(xi)
    X0, X1 = rectify_ref.pinhole_rays(pin)
    x, y, z = rectify_ref.transform(R, t, X0, X1)
    rx, ry = np.empty(gx.shape, np.float32), np.empty(gx.shape, np.float32)
    for i in range(gx.shape[0]):
        for j in range(gx.shape[1]):
            ok, uv = vgo.project_point(model, intr, [x[i, j], y[i, j], z[i, j]])
            rx[i, j], ry[i, j] = (np.float32(uv[0]), np.float32(uv[1])) if ok else (-1., -1.)
    n_fail = _check_maps(gx, gy, rx, ry)
    if case == 1:
        assert 0 < n_fail < gx.size, "the wide pinhole of case 1 must have pixels the camera cannot see"


@pytest.mark.parametrize("case", [0, 1, 3, 5])
def test_map_parity_full_hd(torch, case):
    from visgeom_amd import rectify

    model, intr, _, xi = CASES[case]
    pin = [1920, 1080, 959.5, 539.5, 600. if case != 1 else 150.]
    gx, gy = (t.cpu().numpy() for t in rectify.rectify_maps(model, intr, pin, xi))
    rx, ry = rectify_ref.rectify_maps(model, intr, pin, *_rot(xi))
    _check_maps(gx, gy, rx, ry)


def _random_maps(rng, mh, mw, sw, sh):
    """map entries over and past the source: fractional, integer, on the border, (-1, -1), NaN, huge"""
    mx = rng.uniform(-2.5, sw + 1.5, (mh, mw)).astype(np.float32)
    my = rng.uniform(-2.5, sh + 1.5, (mh, mw)).astype(np.float32)
    k = mx.size
    sel = rng.integers(0, k, k // 10)
    mx.flat[sel], my.flat[sel] = np.floor(mx.flat[sel]), np.floor(my.flat[sel])
    specials = [(-1., -1.), (np.nan, 3.), (3., np.nan), (1e30, 2.), (-1e30, 1e30), (0., 0.), (sw - 1., sh - 1.),
                (sw - 0.5, 1.), (-0.5, sh - 0.5), (-0.999, -0.999), (float(sw), 1.), (1., float(sh))]
    for q, (a, b) in enumerate(specials):
        mx.flat[q * 7], my.flat[q * 7] = a, b
    return mx, my


REMAP_CASES = [(dt, c, n) for dt, c in (("u8", 1), ("u8", 3), ("u8", 4), ("f32", 1)) for n in (1, 3, 17)]


@pytest.mark.parametrize("dt,c,n", REMAP_CASES)
@pytest.mark.parametrize("shape", [(37, 23, 51, 29), (64, 48, 40, 30)])   # src_w, src_h, map_w, map_h
def test_remap_parity(torch, dt, c, n, shape):
    from visgeom_amd import rectify

    sw, sh, mw, mh = shape
    rng = np.random.default_rng(zlib.crc32(repr((dt, c, n, shape)).encode()))
    if dt == "u8":
        imgs = rng.integers(0, 256, (n, sh, sw, c), dtype=np.uint8)
        fills = (0., 255.)
    else:
        imgs = rng.uniform(-3., 5., (n, sh, sw, c)).astype(np.float32)
        fills = (0., 0.5)
    mx, my = _random_maps(rng, mh, mw, sw, sh)
    dev = torch.device("cuda", 0)
    ti = torch.from_numpy(imgs).to(dev)
    tx, ty = torch.from_numpy(mx).to(dev), torch.from_numpy(my).to(dev)
    for fill in fills:
        got = rectify.remap(ti if c > 1 else ti[..., 0], tx, ty, fill).cpu().numpy().reshape(n, mh, mw, c)
        want = rectify_ref.remap(imgs, mx, my, fill)
        if dt == "u8":
            d = np.abs(got.astype(np.int32) - want.astype(np.int32))
            assert d.max() <= 1 and (d == 0).mean() >= 0.999, (d.max(), (d == 0).mean())
        else:
            scale = float(imgs.max() - imgs.min())
            assert np.allclose(got, want, rtol=0, atol=1e-5 * scale), np.abs(got - want).max()


@pytest.mark.parametrize("dt,c", [("u8", 1), ("u8", 3), ("f32", 1), ("f32", 4)])
def test_batch_equals_single_frames(torch, dt, c):
    from visgeom_amd import rectify

    rng = np.random.default_rng(5)
    n, sh, sw, mh, mw = 6, 50, 70, 44, 64
    imgs = rng.integers(0, 256, (n, sh, sw, c), dtype=np.uint8) if dt == "u8" else rng.uniform(0, 1, (n, sh, sw, c)).astype(np.float32)
    mx, my = _random_maps(rng, mh, mw, sw, sh)
    dev = torch.device("cuda", 0)
    ti = torch.from_numpy(imgs).to(dev)
    tx, ty = torch.from_numpy(mx).to(dev), torch.from_numpy(my).to(dev)
    batch = rectify.remap(ti, tx, ty, 3.).cpu().numpy()
    for k in range(n):
        one = rectify.remap(ti[k:k + 1].contiguous(), tx, ty, 3.).cpu().numpy()
        assert np.array_equal(batch[k:k + 1].view(np.uint8), one.view(np.uint8)), k


@pytest.mark.parametrize("w", [64, 61])
def test_identity_map(torch, w):
    from visgeom_amd import rectify

    rng = np.random.default_rng(w)
    h = 37
    dev = torch.device("cuda", 0)
    j, i = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    tx, ty = torch.from_numpy(j).to(dev), torch.from_numpy(i).to(dev)
    for imgs in (rng.integers(0, 256, (4, h, w, 3), dtype=np.uint8), rng.standard_normal((3, h, w)).astype(np.float32)):
        got = rectify.remap(torch.from_numpy(imgs).to(dev), tx, ty, 17.).cpu().numpy()
        assert np.array_equal(got.view(np.uint8), imgs.view(np.uint8))


def test_wrapper_validation(torch):
    from visgeom_amd import rectify

    dev = torch.device("cuda", 0)
    m = torch.zeros((4, 4), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        rectify.remap(torch.zeros((2, 4, 4), dtype=torch.int16, device=dev), m, m)
    with pytest.raises(ValueError):
        rectify.remap(torch.zeros((4, 4), dtype=torch.uint8), m.cpu(), m.cpu())
    with pytest.raises(ValueError):
        rectify.remap(torch.zeros((8, 8), dtype=torch.uint8, device=dev)[:, ::2], m, m)
    with pytest.raises(ValueError):
        rectify.remap(torch.zeros((4, 4), dtype=torch.uint8, device=dev), m.double(), m.double())
    from visgeom_amd import capi

    with pytest.raises(capi.VisgeomError) as ei:   # two channels: the library refuses
        rectify.remap(torch.zeros((1, 4, 4, 2), dtype=torch.uint8, device=dev), m, m)
    assert ei.value.code == capi.ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------------- end to end
CAM = [0.62, 1.05, 330., 331., 399.5, 299.5]   # EUCM of an 800 x 600 fisheye
PIN = [640, 480, 319.5, 239.5, 300.]
SQ, NX, NY, DEPTH = 0.1, 9, 7, 1.0          # board: NX x NY squares of SQ m at DEPTH m, centred on the optical axis


def _eucm_unproject(p, u, v):
    """EnhancedCamera::reconstructPoint (eucm.h:85-106), vectorised: the ray of a fisheye pixel, z normalised to 1"""
    alpha, beta, fu, fv, u0, v0 = p
    mx, my = (u - u0) / fu, (v - v0) / fv
    r2 = mx * mx + my * my
    mz = (1. - beta * alpha * alpha * r2) / (alpha * np.sqrt(1. - (2. * alpha - 1.) * beta * r2) + (1. - alpha))
    return mx / mz, my / mz


def _fisheye_board(w=800, h=600):
    """the board seen by the EUCM camera: a checkerboard on the plane z = DEPTH, 40 / 220 grey, 128 elsewhere"""
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x, y = _eucm_unproject(CAM, u, v)
    X, Y = x * DEPTH, y * DEPTH
    cx, cy = np.floor(X / SQ + NX / 2.), np.floor(Y / SQ + NY / 2.)
    on = (cx >= 0) & (cx < NX) & (cy >= 0) & (cy < NY)
    return np.where(on, np.where((cx + cy) % 2 == 0, 40, 220), 128).astype(np.uint8)


def _invert_map(mx, my, u, v):
    """the pinhole pixel (j, i) whose map entry is (u, v): nearest entry, then Newton steps on the bilinear map"""
    d = (mx - u) ** 2 + (my - v) ** 2
    i, j = np.unravel_index(np.argmin(d), d.shape)
    p = np.array([j, i], np.float64)

    def at(q):
        j0, i0 = int(np.floor(q[0])), int(np.floor(q[1]))
        a, b = q[0] - j0, q[1] - i0
        f = lambda m: ((1 - b) * ((1 - a) * m[i0, j0] + a * m[i0, j0 + 1]) + b * ((1 - a) * m[i0 + 1, j0] + a * m[i0 + 1, j0 + 1]))
        return np.array([f(mx.astype(np.float64)), f(my.astype(np.float64))])

    for _ in range(4):
        e = 0.25
        J = np.column_stack([(at(p + [e, 0]) - at(p - [e, 0])) / (2 * e), (at(p + [0, e]) - at(p - [0, e])) / (2 * e)])
        p = p - np.linalg.solve(J, at(p) - [u, v])
    return p


def test_end_to_end_checkerboard(torch, tmp_path):
    from visgeom_amd import _build, rectify

    img = _fisheye_board()
    map_x, map_y = rectify.rectify_maps("eucm", CAM, PIN, np.zeros(6))
    mx, my = map_x.cpu().numpy(), map_y.cpu().numpy()
    # straight board lines stay straight: the corners' projections, found in the pinhole image through the map
    from oracle import vgo

    gx, gy = np.meshgrid(np.arange(NX + 1) - NX / 2., np.arange(NY + 1) - NY / 2.)
    pts = np.empty(gx.shape + (2,))
    for a in range(gx.shape[0]):
        for b in range(gx.shape[1]):
            ok, uv = vgo.project_point(0, CAM, [gx[a, b] * SQ, gy[a, b] * SQ, DEPTH])
            assert ok
            pts[a, b] = _invert_map(mx, my, uv[0], uv[1])
    for line in list(pts) + list(pts.transpose(1, 0, 2)):   # rows and columns of corners
        c = line - line.mean(0)
        n = np.linalg.svd(c)[2][-1]   # unit normal of the total-least-squares line
        res = c @ n
        assert np.abs(res).max() <= 0.05, np.abs(res).max()
    # ... and land where a pinhole with the same axis puts them (f X / Z + c)
    want = np.stack([PIN[4] * gx * SQ / DEPTH + PIN[2], PIN[4] * gy * SQ / DEPTH + PIN[3]], -1)
    assert np.abs(pts - want).max() <= 0.05
    # the rectified board: the pinhole rendering of the same board, away from the square edges
    dev = torch.device("cuda", 0)
    out = rectify.remap(torch.from_numpy(img).to(dev), map_x, map_y).cpu().numpy()
    jj, ii = np.meshgrid(np.arange(PIN[0]), np.arange(PIN[1]))
    X, Y = (jj - PIN[2]) / PIN[4] * DEPTH, (ii - PIN[3]) / PIN[4] * DEPTH
    fx, fy = X / SQ + NX / 2., Y / SQ + NY / 2.
    on = (fx >= 0) & (fx < NX) & (fy >= 0) & (fy < NY)
    ref = np.where(on, np.where((np.floor(fx) + np.floor(fy)) % 2 == 0, 40, 220), 128)
    far = (np.abs(fx - np.round(fx)) > 0.1) & (np.abs(fy - np.round(fy)) > 0.1)
    assert (out[far] == ref[far]).mean() >= 0.995
    # the `rectify` program on two PGMs gives the bytes of the Python remap
    noise = np.random.default_rng(1).integers(0, 256, img.shape, dtype=np.uint8)
    for k, im in enumerate((img, noise)):
        (tmp_path / ("in%d.pgm" % k)).write_bytes(b"P5\n%d %d\n255\n" % (im.shape[1], im.shape[0]) + im.tobytes())
    cfg = {"camera_params": CAM, "pinhole_params": PIN, "xi_eucm_pinhole": [0, 0, 0, 0, 0, 0], "image_names": ["in0.pgm", "in1.pgm"]}
    (tmp_path / "r.json").write_text(json.dumps(cfg))
    r = subprocess.run(["timeout", "-k", "10", "120", _build.RECTIFY_CLI, "r.json"], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    both = rectify.remap(torch.from_numpy(np.stack([img, noise])).to(dev), map_x, map_y).cpu().numpy()
    for k in range(2):
        data = (tmp_path / ("img_%d.pgm" % k)).read_bytes()
        head = b"P5\n%d %d\n255\n" % (PIN[0], PIN[1])
        assert data[:len(head)] == head
        assert data[len(head):] == both[k].tobytes(), k


def test_large_launch_past_2_31_bytes(torch):
    """one u8 C = 3 remap of 96 frames of 3840 x 2160 (2.39 GB in, 2.39 GB out): the batch loop's offsets are 64-bit"""
    from visgeom_amd import rectify

    n, h, w, c = 96, 2160, 3840, 3
    assert n * h * w * c > 2 ** 31
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    imgs = torch.randint(0, 256, (n, h, w, c), dtype=torch.uint8, device=dev, generator=g)
    map_x, map_y = rectify.rectify_maps("eucm", CASES[0][1], [w, h, 1919.5, 1079.5, 700.], CASES[0][3])
    # a remap of the full-size maps: a source as large as the output
    out = rectify.remap(imgs, map_x, map_y, 0.)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    sel = rng.integers(0, h * w, 200_000)
    mx, my = map_x.cpu().numpy().ravel()[sel], map_y.cpu().numpy().ravel()[sel]
    for k in (0, n // 2, n - 1):
        want = rectify_ref.remap(imgs[k:k + 1].cpu().numpy(), mx, my, 0.)[0]
        got = out[k].reshape(h * w, c).cpu().numpy()[sel]
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        assert d.max() <= 1 and (d == 0).mean() >= 0.999, (k, d.max())
    del imgs, out
    torch.cuda.empty_cache()
