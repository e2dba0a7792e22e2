"""The scene renderer on the GPU (include/visgeom_amd.h section 14) against the restatement of the reference's RenderDevice
(tests/render_ref.py) on the scene of tests/render_scene.py: the hit buffers, the image, the counters, the `render` program and the
production library.

What may differ, and why.  A plane's hit is +, -, *, / and sqrt in FP64 in one order on both sides: index equal, u, v and depth
bit-equal.  The background's texture coordinates go through atan2, where the device's may differ from libm's in the last place of
the double, which moves the float32 u or v by at most one step.  The grey value of such a pixel hangs on that last bit only when
its filtered value lies within about 1e-4 of an integer: tests/test_render_cpu.py moves half of all coordinates by a whole
float32 step and allows the restatement 0.1 % of the covered pixels against itself; twice that, 0.2 %, is allowed here, by at
most one grey level.  Pixels whose two nearest hits are less than one float32 step apart (the float32 depth test then hangs on
the last bit of a depth) are left out of the buffer comparison; there are at most 5 per view (none in this scene)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import render_ref as rr
from tests import render_scene as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NAMES = ("image", "depth", "index", "u", "v")


@pytest.fixture(scope="module")
def renderer():
    from visgeom_amd import render

    r = render.Renderer(sc.CAM, sc.W, sc.H, sc.textures()[0], sc.planes())
    yield r
    r.close()


@pytest.fixture(scope="module")
def batch(renderer):
    """the three views rendered in one call: dict of numpy arrays [3, H, W] and counts [3, 5]"""
    out = {k: t.cpu().numpy() for k, t in zip(NAMES, renderer.render(sc.VIEWS, buffers=True))}
    out["counts"] = renderer.counts.copy()
    return out


def _steps(a, b):
    """float32 steps between two arrays of non-negative floats"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_buffers(got, ref, what):
    """got: dict of [H, W] arrays of one view; ref: the restatement's render of it"""
    keep = ~ref["close"]
    print("%s: %d pixels left out (two hits within one float32 step)" % (what, (~keep).sum()))
    assert (~keep).sum() <= 5
    assert (got["index"][keep] == ref["index"][keep]).all(), what
    none, bg, pl = keep & (ref["index"] < 0), keep & (ref["index"] == 0), keep & (ref["index"] > 0)
    assert (got["depth"][none] == rr.DEPTH_INIT).all() and (got["u"][none] == 0).all() and (got["v"][none] == 0).all(), what
    for name in ("u", "v", "depth"):
        assert got[name].dtype == np.float32
        assert (got[name][pl].view(np.int32) == ref[name][pl].view(np.int32)).all(), (what, name)
    assert (got["depth"][bg] == np.float32(rr.BACKGROUND_DEPTH)).all(), what
    for name in ("u", "v"):
        steps = _steps(got[name][bg], ref[name][bg])
        print("%s: background %s differs on %d of %d pixels, by at most %d float32 steps" % (what, name, (steps > 0).sum(), bg.sum(), steps.max()))
        assert steps.max() <= 1, (what, name)


def check_image(got, ref, what):
    cov = ref["index"] >= 0
    assert got["image"].dtype == np.uint8
    same = cov & (got["index"] == ref["index"]) & (got["u"].view(np.int32) == ref["u"].view(np.int32)) & \
        (got["v"].view(np.int32) == ref["v"].view(np.int32))
    diff = np.abs(got["image"].astype(int) - ref["image"].astype(int))
    print("%s: %d of %d covered pixels differ, by at most %d; %d of them with equal index, u and v" % (
        what, (diff[cov] > 0).sum(), cov.sum(), diff[cov].max(), (diff[same] > 0).sum()))
    assert (got["image"][~cov] == 0).all(), what
    assert (diff[same] == 0).all(), what
    assert (diff[cov] > 0).sum() <= 0.002 * cov.sum() and diff[cov].max() <= 1, what


def check_counts(counts, ref, what):
    slack = int(ref["close"].sum())   # a left-out pixel may be counted on the other side
    print("%s: counts %s, restatement %s" % (what, counts.tolist(), ref["counts"].tolist()))
    assert np.abs(counts - ref["counts"]).max() <= slack, what
    assert counts[:4].sum() == sc.W * sc.H


def test_buffers_match_the_restatement(batch):
    for k in range(len(sc.VIEWS)):
        check_buffers({n: batch[n][k] for n in NAMES}, sc.reference(k), "view %d" % k)


def test_image_matches_the_restatement(batch):
    for k in range(len(sc.VIEWS)):
        check_image({n: batch[n][k] for n in NAMES}, sc.reference(k), "view %d" % k)


def test_counts_match_the_restatement(batch):
    for k in range(len(sc.VIEWS)):
        check_counts(batch["counts"][k], sc.reference(k), "view %d" % k)


def test_a_view_alone_has_the_bits_it_has_in_the_batch(renderer, batch):
    for k in range(len(sc.VIEWS)):
        alone = renderer.render(sc.VIEWS[k], buffers=True)
        for name, t in zip(NAMES, alone):
            assert tuple(t.shape) == (sc.H, sc.W)
            assert t.cpu().numpy().tobytes() == batch[name][k].tobytes(), (k, name)
        assert (renderer.counts[0] == batch["counts"][k]).all()


def test_two_runs_have_the_same_bits(renderer, batch):
    again = renderer.render(sc.VIEWS, buffers=True)
    for name, t in zip(NAMES, again):
        assert t.cpu().numpy().tobytes() == batch[name].tobytes(), name
    assert (renderer.counts == batch["counts"]).all()


def test_the_image_does_not_depend_on_the_optional_outputs(renderer, batch):
    import torch

    image = renderer.render(sc.VIEWS)
    assert image.dtype == torch.uint8 and tuple(image.shape) == (3, sc.H, sc.W) and image.is_cuda
    assert image.cpu().numpy().tobytes() == batch["image"].tobytes()
    one = renderer.render(sc.VIEWS[1])
    assert tuple(one.shape) == (sc.H, sc.W) and one.cpu().numpy().tobytes() == batch["image"][1].tobytes()


def test_set_camera_changes_the_views(renderer, batch):
    from visgeom_amd import capi

    renderer.set_camera(sc.CAM2)
    try:
        got = {n: t.cpu().numpy() for n, t in zip(NAMES, renderer.render(sc.VIEWS[1], buffers=True))}
        counts = renderer.counts[0].copy()
        with pytest.raises(capi.VisgeomError):
            renderer.set_camera([0.6, 1.2, 0., 44., 40.5, 30.5])
    finally:
        renderer.set_camera(sc.CAM)
    ref = sc.reference(1, sc.CAM2)
    assert (got["image"] != batch["image"][1]).mean() > 0.5
    check_buffers(got, ref, "view 1, second camera")
    check_image(got, ref, "view 1, second camera")
    check_counts(counts, ref, "view 1, second camera")
    back = renderer.render(sc.VIEWS[1])
    assert back.cpu().numpy().tobytes() == batch["image"][1].tobytes()


def test_argument_refusals(renderer):
    import torch

    from visgeom_amd import capi, render

    tex = sc.textures()
    make = lambda background=tex[0], planes=None, **kw: render.Renderer(  # noqa: E731
        kw.get("cam", sc.CAM), kw.get("width", sc.W), kw.get("height", sc.H), background, sc.planes() if planes is None else planes)
    plane = lambda **kw: [(kw.get("texture", tex[1]), kw.get("pose", sc.PLANES[0]["pose"]), kw.get("width", 6.), kw.get("height", 4.))]  # noqa: E731
    for bad in (tex[0].astype(np.float32), tex[0][None], torch.from_numpy(tex[0]), tex[0][:1], None):
        with pytest.raises(ValueError):
            make(background=bad)
        with pytest.raises(ValueError):
            make(planes=plane(texture=bad))
    for bad in ([0.] * 5, np.zeros((2, 6)), torch.zeros(6, dtype=torch.float64), np.zeros(6, complex), [0., 0., 1., float("nan"), 0., 0.]):
        with pytest.raises(ValueError):
            make(planes=plane(pose=bad))
        with pytest.raises(ValueError):
            renderer.render(bad if not (isinstance(bad, np.ndarray) and bad.shape == (2, 6)) else np.zeros((2, 5)))
    with pytest.raises(ValueError):
        make(planes=plane(width=0.))
    with pytest.raises(ValueError):
        make(planes=sc.planes() * 33)
    with pytest.raises(ValueError):
        make(width=1)
    with pytest.raises(ValueError):
        make(cam=sc.CAM[:5])
    with pytest.raises(ValueError):
        renderer.render(np.zeros((0, 6)))
    # what only the library sees: the NULL image and the view count, with a live handle
    L = capi.load()
    xi = np.zeros(6)
    dp = xi.ctypes.data_as(render._dp)
    assert L.vg_render_views(renderer._h, 1, dp, None, None, None, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert L.vg_render_views(renderer._h, 65536, dp, None, None, None, None, None, None) == capi.ERR_INVALID_ARGUMENT
    assert L.vg_render_views(renderer._h, 0, None, None, None, None, None, None, None) == capi.OK


# ---- the `render` program

def _pfm(path):
    data = open(path, "rb").read()
    head, dims, scale, body = data.split(b"\n", 3)
    w, h = (int(x) for x in dims.split())
    assert head == b"Pf" and float(scale) == -1.0 and len(body) == 4 * w * h
    return np.frombuffer(body, "<f4").reshape(h, w)[::-1]


def test_the_render_program_writes_what_the_python_api_returns(tmp_path, batch):
    from visgeom_amd import _build

    path = sc.write_world(str(tmp_path))
    r = subprocess.run([_build.RENDER_CLI, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for k in range(len(sc.VIEWS)):
        img = open(os.path.join(str(tmp_path), "img_%d.pgm" % k), "rb").read()
        assert img == b"P5\n%d %d\n255\n" % (sc.W, sc.H) + batch["image"][k].tobytes(), k
        assert _pfm(os.path.join(str(tmp_path), "depth_%d.pfm" % k)).tobytes() == batch["depth"][k].tobytes(), k
    assert not os.path.exists(os.path.join(str(tmp_path), "img_3.pgm"))


def test_the_render_program_refuses_a_broken_world(tmp_path):
    from visgeom_amd import _build

    for words, override in ((("background",), dict(background=None)), (("nope.pgm",), dict(background=dict(image_name="nope.pgm"))),
                            (("views",), dict(views=[]))):
        path = sc.write_world(str(tmp_path), **override)
        r = subprocess.run([_build.RENDER_CLI, path], capture_output=True, text=True, timeout=60)
        assert r.returncode not in (0, 2) and r.returncode > 0, (override, r.returncode)
        lines = r.stderr.strip().splitlines()
        assert len(lines) == 1 and lines[0].startswith("render: "), r.stderr
        for w in words:
            assert w in lines[0], lines[0]
        assert not [n for n in os.listdir(str(tmp_path)) if n.startswith("img_") or n.startswith("depth_")]


# ---- the library that ships

def test_production_library_holds_the_same_parity(tmp_path, batch):
    from visgeom_amd import _build

    assert os.path.exists(_build.PRODUCTION_LIB), "python -m visgeom_amd._build --production (or __graft_entry__.build())"
    path = str(tmp_path / "production.npz")
    env = dict(os.environ, VISGEOM_AMD_LIBRARY="production")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "render_dump.py"), path], env=env, cwd=ROOT, timeout=300)
    got = np.load(path)
    assert int(got["has_hooks"][0]) == 0 and "production" in str(got["library"][0])
    for k in range(len(sc.VIEWS)):
        view = {n: got[n][k] for n in NAMES}
        check_buffers(view, sc.reference(k), "production, view %d" % k)
        check_image(view, sc.reference(k), "production, view %d" % k)
        check_counts(got["counts"][k], sc.reference(k), "production, view %d" % k)
    for n in NAMES:   # one source, two builds: the same bits
        assert got[n].tobytes() == batch[n].tobytes(), n
