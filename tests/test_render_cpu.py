"""The scene renderer without a GPU: section 14 of the C ABI is declared, exported and bound and refuses bad arguments before HIP
is touched; the host arithmetic of the anti-aliasing kernels against the restatement (tests/render_ref.py); the cases the test
scene (tests/render_scene.py) must contain for the GPU comparison to mean something, asserted on the restatement's own output;
and how little the restatement's image moves when its float32 texture coordinates move by one step -- the measure the GPU test's
cap on differing pixels is twice of."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import render_ref as rr
from tests import render_scene as sc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "visgeom_amd.h")
ENTRIES = ("vg_render_create", "vg_render_destroy", "vg_render_size", "vg_render_set_camera", "vg_render_views", "vg_render_filter_kernel")
dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def lib():
    from visgeom_amd import _build, capi

    _build.build()
    return capi.load()


def test_section_14_is_declared_exported_and_bound(lib):
    from visgeom_amd import _build, capi

    declared = set(re.findall(r"\b(vg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)))
    for path in (_build.LIB, _build.build_production()):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = set(re.findall(r" T (vg_[a-z0-9_]+)", out))
        for name in ENTRIES:
            assert name in declared and name in exported and name in capi.SIGNATURES, (name, path)
    assert sorted(s for s in declared if s.startswith("vg_render_")) == sorted(ENTRIES)


def _objects(n_planes=2, first_kind=None, cols=None, pose=None, size=None):
    from visgeom_amd import capi

    tex = sc.textures()
    objs = (capi.RenderObject * (1 + n_planes))()
    keep = []
    for k in range(1 + n_planes):
        t = tex[min(k, 2)]
        keep.append(t)
        o = objs[k]
        o.kind = capi.RENDER_BACKGROUND if k == 0 else capi.RENDER_PLANE
        o.texture = t.ctypes.data
        o.rows, o.cols = t.shape
        if k:
            p = sc.PLANES[min(k, 2) - 1]
            o.pose[:] = p["pose"]
            o.width, o.height = p["width"], p["height"]
    if first_kind is not None:
        objs[0].kind = first_kind
    if cols is not None:
        objs[1].cols = cols
    if pose is not None:
        objs[1].pose[:] = pose
    if size is not None:
        objs[2].width = size
    return objs, keep


def _create(lib, objs, cam=sc.CAM, width=sc.W, height=sc.H, n=None):
    h = ctypes.c_void_p()
    c = np.array(cam, dtype=np.float64)
    rc = lib.vg_render_create(ctypes.byref(h), 0, None, c.ctypes.data_as(dp), width, height, len(objs) if n is None else n, ctypes.byref(objs))
    return rc, h, lib.vg_last_error().decode()


def test_create_refuses_bad_worlds_before_hip_is_touched(lib):
    """... and a good world gets VG_ERR_NO_DEVICE on a machine without a GPU.  vg_render_create is the only entry of the section
    that can return it there: vg_render_views, vg_render_set_camera and vg_render_size need the handle that creation did not
    give, and vg_render_filter_kernel is host only."""
    from visgeom_amd import capi

    def refused(*words, **kw):
        objs, keep = _objects(**{k: v for k, v in kw.items() if k in ("n_planes", "first_kind", "cols", "pose", "size")})
        rc, h, msg = _create(lib, objs, **{k: v for k, v in kw.items() if k in ("cam", "width", "height", "n")})
        assert rc == capi.ERR_INVALID_ARGUMENT and not h.value, (kw, rc, msg)
        for w in words:
            assert w in msg, (kw, msg)

    refused("object 0 must be the background", first_kind=capi.RENDER_PLANE)
    refused("at most 64 planes", n_planes=65)
    refused("at most 64 planes", n=0)
    refused("[2, 16384]", width=1)
    refused("[2, 16384]", height=16385)
    refused("texture", "[2, 16384]", cols=1)
    refused("texture", "[2, 16384]", cols=16385)
    refused("finite", pose=[0., 0., float("nan"), 0., 0., 0.])
    refused("finite", pose=[0., 0., 1., float("inf"), 0., 0.])
    refused("positive", size=0.)
    refused("camera", "finite", cam=[0.75, float("nan"), 40., 39., 39.5, 29.5])
    refused("non-zero", cam=[0.75, 1.6, 0., 39., 39.5, 29.5])
    objs, keep = _objects()
    objs[2].texture = None
    rc, h, msg = _create(lib, objs)
    assert rc == capi.ERR_INVALID_ARGUMENT and "texture" in msg
    assert lib.vg_render_create(None, 0, None, None, sc.W, sc.H, 1, None) == capi.ERR_INVALID_ARGUMENT
    # 64 planes are a world: only the device is missing then
    import torch

    if not torch.cuda.is_available():
        for n_planes in (2, 64):
            objs, keep = _objects(n_planes=n_planes)
            rc, h, msg = _create(lib, objs)
            assert rc == capi.ERR_NO_DEVICE and not h.value, (rc, msg)


def test_calls_refuse_bad_arguments_before_hip_is_touched(lib):
    from visgeom_amd import capi

    xi = np.zeros((3, 6))
    img = ctypes.c_void_p(64)   # never dereferenced: every call below is refused first
    views = lambda n, poses, image: (lib.vg_render_views(None, n, poses.ctypes.data_as(dp) if poses is not None else None, image, None, None, None,  # noqa: E731
                                                         None, None), lib.vg_last_error().decode())
    for n in (-1, 65536):
        rc, msg = views(n, xi, img)
        assert rc == capi.ERR_INVALID_ARGUMENT and "view count must be in [0, 65535]" in msg
    rc, msg = views(3, xi, None)
    assert rc == capi.ERR_INVALID_ARGUMENT and "image is NULL" in msg
    rc, msg = views(3, None, img)
    assert rc == capi.ERR_INVALID_ARGUMENT and "poses are NULL" in msg
    bad = xi.copy()
    bad[2, 4] = np.inf
    rc, msg = views(3, bad, img)
    assert rc == capi.ERR_INVALID_ARGUMENT and "finite" in msg
    rc, msg = views(3, xi, img)
    assert rc == capi.ERR_INVALID_ARGUMENT and "handle is NULL" in msg
    w = ctypes.c_int()
    assert lib.vg_render_size(None, ctypes.byref(w), ctypes.byref(w)) == capi.ERR_INVALID_ARGUMENT
    assert lib.vg_render_set_camera(None, xi.ctypes.data_as(dp)) == capi.ERR_INVALID_ARGUMENT
    lib.vg_render_destroy(None)


def test_filter_kernels_match_the_restatement(lib):
    from visgeom_amd import capi

    for length in range(1, rr.MAX_KERNEL + 1):
        out = np.full(length + 1, -7.)
        assert lib.vg_render_filter_kernel(length, out.ctypes.data_as(dp)) == capi.OK
        assert out[length] == -7.
        k = out[:length]
        assert np.abs(k - rr.KERNELS[length]).max() <= 1e-12, length
        assert abs(k.sum() - 1.) <= 1e-12 and (k > 0).all(), length
        assert np.abs(k - k[::-1]).max() <= 1e-12   # the filter is even
    one, two = np.zeros(1), np.zeros(2)
    lib.vg_render_filter_kernel(1, one.ctypes.data_as(dp))
    lib.vg_render_filter_kernel(2, two.ctypes.data_as(dp))
    assert one.tolist() == [1.] and two.tolist() == [0.5, 0.5]
    for length in (0, 25, -1):
        assert lib.vg_render_filter_kernel(length, two.ctypes.data_as(dp)) == capi.ERR_INVALID_ARGUMENT
        assert b"[1, 24]" in lib.vg_last_error()
    assert lib.vg_render_filter_kernel(3, None) == capi.ERR_INVALID_ARGUMENT


def test_bilinear_keeps_the_reference_s_quirks():
    tex = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90], [100, 110, 120]], np.uint8)   # 3 cols, 4 rows
    at = lambda x, y: float(rr.bilinear(tex, np.array([x]), np.array([y]))[0])   # noqa: E731
    assert at(0.5, 0.5) == (50 * 0.5 + 40 * 0.5) * 0.5 + (20 * 0.5 + 10 * 0.5) * 0.5
    assert at(-0.5, 0.) == 20 * -0.5 + 10 * 1.5          # int() truncates towards zero: cell 0, extrapolated
    assert at(0., -0.5) == (40 * 1.) * -0.5 + (10 * 1.) * 1.5
    assert at(-1., 2.) == 10.                            # u fails: column 0 and, `fail` being set, row 0
    assert at(2., 2.) == 30.                             # u > cols - 2: the last column, and row 0 again
    assert at(0.5, 3.) == 100.                           # v > rows - 2 alone: the last row, u as truncated
    assert at(0.5, -1.5) == 10.
    assert at(1., 1.) == 50.


def test_the_scene_contains_every_case_the_gpu_comparison_relies_on():
    lengths, hidden = set(), 0
    for k in range(len(sc.VIEWS)):
        r = sc.reference(k)
        cov = r["index"] >= 0
        assert r["counts"].sum() - r["counts"][4] == sc.W * sc.H and r["counts"][0] == (~r["ok"]).sum() > 100
        assert (r["image"][~cov] == 0).all() and (r["depth"][~cov] == rr.DEPTH_INIT).all()
        assert (r["index"] == 0).sum() > 1000 and (r["index"] == 1).sum() > 1000 and (r["index"] == 2).sum() > 200
        assert r["counts"][4] >= 100                                   # nu = nv = 1
        assert r["nu"][cov].max() == 24 or r["nv"][cov].max() == 24
        lengths |= set(r["nu"][cov].tolist()) | set(r["nv"][cov].tolist())
        assert 150 <= (r["ucount"][cov] == 1).sum() <= 400             # one same-object neighbour along the row
        assert (r["left"] > 0).all()                                   # taps leave the textures on each of the four sides
        assert r["close"].sum() <= 5
        # plane 2 beats plane 1 on depth: where plane 2 is seen, the floor behind it is hit too
        xi = [float(v) for v in sc.VIEWS[k]]
        behind = rr.fill_buffers(sc.CAM, sc.W, sc.H, sc.objects()[:2], xi)
        won = (r["index"] == 2) & (behind["index"] == 1)
        assert (r["depth"][won] < behind["depth"][won]).all()
        hidden += int(won.sum())
        assert r["image"][cov].min() > 0 and r["image"][cov].max() < 255   # no value sits on the clamp
    assert lengths == set(range(1, 25)) and hidden > 100
    assert sum(int((sc.reference(k)["ucount"] == 0).sum()) for k in range(len(sc.VIEWS))) >= 1   # no neighbour at all
    assert sc.W % 64 != 0 and len(sc.VIEWS) == 3


@pytest.mark.parametrize("k", range(len(sc.VIEWS)))
def test_one_float32_step_of_the_texture_coordinates_moves_almost_no_pixel(k):
    """the restatement against itself: a random half of the float32 u and v entries moved one step, once up and once down.  At
    most 0.1 % of the covered pixels may change, and by one grey level: the reference's image hangs on the last bit of its
    buffers that rarely, so a device whose atan2 differs from libm's in the last place stays far inside the GPU test's 0.2 %."""
    r = sc.reference(k)
    cov = r["index"] >= 0
    rng = np.random.default_rng(100 + k)
    for direction in (np.float32(np.inf), np.float32(-np.inf)):
        buf = dict(index=r["index"])
        for name in ("u", "v"):
            moved = np.nextafter(r[name], direction)
            buf[name] = np.where(rng.random(r[name].shape) < 0.5, moved, r[name]).astype(np.float32)
            assert (buf[name] != r[name])[cov].sum() > cov.sum() // 3
        img = rr.fill_image(sc.W, sc.H, sc.objects(), buf)["image"]
        diff = np.abs(img.astype(int) - r["image"].astype(int))
        print("view %d: %d of %d covered pixels differ, by at most %d" % (k, (diff[cov] > 0).sum(), cov.sum(), diff.max()))
        assert (diff[~cov] == 0).all()
        assert (diff[cov] > 0).sum() <= 0.001 * cov.sum() and diff.max() <= 1
