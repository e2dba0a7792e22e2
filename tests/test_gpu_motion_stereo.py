"""Motion stereo on the GPU (vg_motion_stereo_*, visgeom_amd.motion_stereo) against the restatement (tests/motion_ref.py): the
mask, the per-pixel stage record, compute without a prior and over a sequence with an SGM prior, the too-certain path, the
in-place call, a batch against single calls, ground truth on three synthetic rigs and the production library."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import motion_ref as mr
from tests import motion_scene as ms
from tests import stereo_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIGS = ["sideways", "vertical", "forward"]
SCALE2 = dict(scale=2, u0=11, v0=7, equal_margins=0, x_max=50, y_max=38)
# What the restatement alone reaches on these scenes (96 x 64 depth pixels, tests/motion_scene.py), measured on the CPU: median
# relative range error at the share of depth pixels with a depth (their number)
#   without a prior   sideways 0.0568 at 0.812 (4 988),  vertical 0.0529 at 0.715 (4 394),  forward 0.0710 at 0.281 (1 729)
#   after the 4 steps sideways 0.0168 at 0.812,          vertical 0.0155 at 0.715,          forward 0.0266 at 0.281
#   first SGM map -> after the sequence, on the pixels both hold: sideways 0.0408 -> 0.0168, vertical 0.0401 -> 0.0155,
#                     forward 0.0530 -> 0.0266 (the restatement passes the "fusing must not make the map worse" rule on all rigs)
# Bars: 1.5 x the error, 0.85 x the share (the GPU must equal the restatement; the margin only keeps the bar from being a copy).
TRUTH_NO_PRIOR = {"sideways": (0.0852, 0.690), "vertical": (0.0794, 0.608), "forward": (0.1065, 0.239)}
TRUTH_SEQUENCE = {"sideways": (0.0253, 0.690), "vertical": (0.0233, 0.608), "forward": (0.0399, 0.239)}
SCENES = {}


@pytest.fixture(scope="module")
def torch():
    import torch

    from visgeom_amd import _build

    _build.build()
    return torch


def scene(rig):
    if rig not in SCENES:
        SCENES[rig] = stereo_scene.make_scene(rig)
    return SCENES[rig]


def cuda(torch, *a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def handle(p, torch):
    from visgeom_amd import motion_stereo

    return motion_stereo.MotionStereo(stereo_scene.CAM1, stereo_scene.CAM2, motion_stereo.make_params(**p))


def reference(p, img1):
    M = mr.MotionStereo(stereo_scene.CAM1, stereo_scene.CAM2, mr.params(**p))
    M.set_base(img1)
    return M


def sgm_prior(torch, rig, p):
    """(depth, sigma, cost) CUDA tensors of vg_stereo_compute on the rig's first pair"""
    from visgeom_amd import stereo

    img1, img2, _, xi = scene(rig)
    sp = {k: v for k, v in p.items() if k != "gradient_thresh"}
    s = stereo.Stereo(stereo_scene.CAM1, stereo_scene.CAM2, xi, stereo.make_params(**sp))
    dep, sig, cst, _ = s.compute(*cuda(torch, img1, img2))
    s.close()
    return dep, sig, cst


def assert_maps(got, want):
    """depth, sigma to 1e-12 relative with the same zeros, cost exactly"""
    for g, w in zip(got[:2], want[:2]):
        np.testing.assert_array_equal(g == 0, w == 0)
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(got[2], want[2])


def stat(dep, rng):
    m = (dep > 0) & (rng > 0)
    return float(np.median(np.abs(dep[m] - rng[m]) / rng[m])), float(m.mean()), int(m.sum())


def test_mask_equals_restatement(torch):
    from visgeom_amd import motion_stereo

    rnd = np.random.default_rng(11)
    flat = np.full((93, 125), 90, np.uint8)
    flat[40:60, 50:80] = 110   # one patch: the mask is set along its edge only
    imgs = np.stack([scene("sideways")[0], ms.view(ms.poses("forward")[2]), rnd.integers(0, 256, (93, 125), dtype=np.uint8), flat])
    for thresh in (2, 40):
        h = handle(ms.prm_of("sideways", gradient_thresh=thresh), torch)
        h.set_base(cuda(torch, imgs)[0])
        got = h.mask().cpu().numpy()
        h.close()
        for k in range(len(imgs)):
            want = mr.compute_mask(imgs[k], thresh)
            np.testing.assert_array_equal(got[k], want)
            assert set(np.unique(want)) <= {0, 128}
        assert thresh != 2 or 0 < (got[3] > 0).mean() < 0.5
    # a size that is no multiple of the tile, smaller than the blur's reach in one direction
    small = rnd.integers(0, 256, (5, 37), dtype=np.uint8)
    p = motion_stereo.make_params(u_max=37, v_max=5, x_max=4, y_max=2, disp_max=8)
    h = motion_stereo.MotionStereo(stereo_scene.CAM1, stereo_scene.CAM2, p)
    h.set_base(cuda(torch, small)[0])
    np.testing.assert_array_equal(h.mask().cpu().numpy()[0], mr.compute_mask(small, 2))
    h.close()


@pytest.mark.parametrize("rig", RIGS)
@pytest.mark.parametrize("with_prior", [False, True], ids=["noprior", "prior"])
@pytest.mark.parametrize("extra", [{}, SCALE2], ids=["scale1", "scale2"])
def test_select_record_bit_exact(torch, rig, with_prior, extra):
    img1, img2, _, xi = scene(rig)
    p = ms.prm_of(rig, **extra)
    pose = ms.poses(rig)[0] if with_prior else xi
    view = ms.view(pose) if with_prior else img2
    prior = sgm_prior(torch, rig, p) if with_prior else None
    h = handle(p, torch)
    h.set_base(cuda(torch, img1)[0])
    got = h.select(pose, cuda(torch, view)[0], prior).cpu().numpy()
    h.close()
    ref = reference(p, img1).compute(pose, view, None if prior is None else [t.cpu().numpy() for t in prior])
    np.testing.assert_array_equal(got, ref["record"])
    st = ref["record"][..., mr.STATUS]
    assert (st == mr.UPDATED).sum() > 200 and (st != mr.UPDATED).any()


@pytest.mark.parametrize("rig", RIGS)
def test_compute_without_prior(torch, rig):
    img1, img2, rng, xi = scene(rig)
    p = ms.prm_of(rig)
    h = handle(p, torch)
    h.set_base(cuda(torch, img1)[0])
    got = [t.cpu().numpy() for t in h.compute(xi, cuda(torch, img2)[0])]
    counts = h.counts.copy()
    h.close()
    ref = reference(p, img1).compute(xi, img2)
    assert_maps(got, (ref["depth"], ref["sigma"], ref["cost"]))
    np.testing.assert_array_equal(counts[0], ref["counts"])
    assert counts[0, :5].sum() == got[0].size and counts[0, 5] == (got[0] != 0).sum()
    err, share, n = stat(got[0], rng)
    print("without a prior, %s: median relative range error %.4f, share %.3f, %d pixels" % (rig, err, share, n))
    assert n >= 1000
    assert err <= TRUTH_NO_PRIOR[rig][0] and share >= TRUTH_NO_PRIOR[rig][1]
    if rig == "forward":   # the epipole paths ran: inverted sampling and pixels too close to the epipole of camera 1
        assert ref["record"][..., mr.INVERTED].any() and (ref["record"][..., mr.STATUS] == mr.REJ_SELECT).sum() > 100


@pytest.mark.parametrize("rig", RIGS)
def test_sequence_with_sgm_prior(torch, rig):
    """every step is compared against the restatement fed the same prior (the GPU's previous output)"""
    img1, _, rng, _ = scene(rig)
    p = ms.prm_of(rig)
    first = sgm_prior(torch, rig, p)
    h = handle(p, torch)
    h.set_base(cuda(torch, img1)[0])
    R = reference(p, img1)
    cur = first
    for pose in ms.poses(rig):
        view = ms.view(pose)
        ref = R.compute(pose, view, [t.cpu().numpy() for t in cur])
        cur = h.compute(pose, cuda(torch, view)[0], cur)
        assert_maps([t.cpu().numpy() for t in cur], (ref["depth"], ref["sigma"], ref["cost"]))
        np.testing.assert_array_equal(h.counts[0], ref["counts"])
        assert ref["counts"][5] > 300
    h.close()
    dep, sgm = cur[0].cpu().numpy(), first[0].cpu().numpy()
    err, share, n = stat(dep, rng)
    print("after the sequence, %s: median relative range error %.4f, share %.3f, %d pixels" % (rig, err, share, n))
    assert n >= 1000
    assert err <= TRUTH_SEQUENCE[rig][0] and share >= TRUTH_SEQUENCE[rig][1]
    both = (dep > 0) & (sgm > 0) & (rng > 0)
    e_seq = np.median(np.abs(dep[both] - rng[both]) / rng[both])
    e_sgm = np.median(np.abs(sgm[both] - rng[both]) / rng[both])
    print("  on the pixels both hold: SGM %.4f, after the sequence %.4f" % (e_sgm, e_seq))
    assert e_seq <= 1.1 * e_sgm   # fusing must not make the map worse


def test_too_certain_prior_leaves_the_map_untouched(torch):
    img1, img2, rng, xi = scene("sideways")
    p = ms.prm_of("sideways")
    dep = np.where(rng > 0, rng, 1.2)
    sig = np.full_like(dep, 1e-9)
    cst = np.full_like(dep, 17.25)
    h = handle(p, torch)
    h.set_base(cuda(torch, img1)[0])
    prior = cuda(torch, dep, sig, cst)
    got = [t.cpu().numpy() for t in h.compute(xi, cuda(torch, img2)[0], prior)]
    counts = h.counts[0].copy()
    h.close()
    for g, w in zip(got, (dep, sig, cst)):
        assert g.tobytes() == w.tobytes()
    ref = reference(p, img1).compute(xi, img2, (dep, sig, cst))
    np.testing.assert_array_equal(counts, ref["counts"])
    assert counts[2] > 3000 and counts[3] == 0 and counts[4] == 0 and counts[5] == 0


def test_in_place_equals_out_of_place(torch):
    rig = "vertical"
    img1, _, _, _ = scene(rig)
    p = ms.prm_of(rig)
    prior = sgm_prior(torch, rig, p)
    pose = ms.poses(rig)[1]
    view = cuda(torch, ms.view(pose))[0]
    h = handle(p, torch)
    h.set_base(cuda(torch, img1)[0])
    out = [t.cpu().numpy() for t in h.compute(pose, view, prior)]
    c_out = h.counts.copy()
    buf = [t.clone() for t in prior]
    h.compute(pose, view, buf, out=buf)
    np.testing.assert_array_equal(h.counts, c_out)
    h.close()
    assert c_out[0, 5] > 300
    for a, b in zip(out, buf):
        assert a.tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("with_prior", [False, True], ids=["noprior", "prior"])
def test_batch_of_8_equals_single_calls(torch, with_prior):
    img1, _, rng, _ = scene("sideways")
    noise = np.random.default_rng(3)
    base = np.stack([np.clip(img1.astype(int) + noise.integers(-4, 5, img1.shape), 0, 255).astype(np.uint8) for _ in range(8)])
    poses = [stereo_scene.RIGS["sideways"], stereo_scene.RIGS["vertical"], stereo_scene.RIGS["forward"]] + ms.poses("sideways") + \
        [ms.poses("vertical")[1]]
    views = np.stack([ms.view(list(q)) for q in poses])
    p = ms.prm_of("forward")
    prior = None
    if with_prior:
        dep = np.stack([np.where(rng > 0, rng * (1. + 0.02 * k), 0.) for k in range(8)])
        prior = cuda(torch, dep, np.full_like(dep, 0.15), np.full_like(dep, 60.))
    tb, tv = cuda(torch, base, views)
    h = handle(p, torch)
    h.set_base(tb)
    batch = [t.cpu().numpy() for t in h.compute(poses, tv, prior)]
    counts = h.counts.copy()
    h.close()
    one = handle(p, torch)
    for k in range(8):
        one.set_base(tb[k])
        got = one.compute(poses[k], tv[k], None if prior is None else [t[k] for t in prior])
        for g, w in zip(got, batch):
            assert g.cpu().numpy().tobytes() == w[k].tobytes()
        np.testing.assert_array_equal(one.counts[0], counts[k])
        assert counts[k, 5] > 100
    one.close()
    assert len({tuple(c) for c in counts}) == 8   # the items differ


def _dump(tmp_path, which):
    env = dict(os.environ)
    env.pop("VISGEOM_AMD_LIBRARY", None)
    if which == "production":
        env["VISGEOM_AMD_LIBRARY"] = "production"
    path = str(tmp_path / ("%s.npz" % which))
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "motion_dump.py"), path], env=env, cwd=ROOT)
    return np.load(path)


def test_production_library_gives_the_same_bits(tmp_path):
    from visgeom_amd import _build

    assert os.path.exists(_build.PRODUCTION_LIB), "python -m visgeom_amd._build --production (or __graft_entry__.build())"
    a, b = _dump(tmp_path, "hooks"), _dump(tmp_path, "production")
    assert int(a["has_hooks"][0]) == 1 and int(b["has_hooks"][0]) == 0
    keys = sorted(k for k in a.files if k != "has_hooks")
    assert keys == sorted(k for k in b.files if k != "has_hooks") and len(keys) >= 8
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert (a["depth_prior"] != 0).mean() > 0.2 and a["counts_prior"][0, 5] > 1000


def test_cli_on_a_sequence_equals_the_wrapper(torch, tmp_path):
    """SGM on the first two further images, motion stereo after: depth_<i>.pfm / sigma_<i>.pfm equal the wrapper's maps"""
    import json

    from visgeom_amd import _build, motion_stereo, stereo

    params = dict(stereo_scene.SCENE_JSON_PARAMS, motion_stereo_parameters={"gradient_thresh": 3})
    path, images, poses = ms.write_sequence(str(tmp_path), "sideways", params)
    r = subprocess.run([_build.MOTION_STEREO_CLI, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mp = motion_stereo.params_from_json(json.load(open(path))["stereo_parameters"])
    assert mp.gradient_thresh == 3
    h = motion_stereo.MotionStereo(stereo_scene.CAM1, stereo_scene.CAM2, mp)
    key = cuda(torch, images[0])[0]
    h.set_base(key)
    cur = None
    for i in range(1, len(images)):
        view = cuda(torch, images[i])[0]
        if i <= 2:
            cur = stereo.stereo(key, view, stereo_scene.CAM1, stereo_scene.CAM2, poses[i], mp.stereo)[:3]
        else:
            cur = h.compute(poses[i], view, cur)
            assert h.counts[0, 5] > 1000
        for name, want in (("depth_%d.pfm" % i, cur[0]), ("sigma_%d.pfm" % i, cur[1])):
            got = stereo_scene.read_pfm(str(tmp_path / name))
            np.testing.assert_array_equal(got, want.cpu().numpy().astype(np.float32))
    h.close()
    assert (cur[0] > 0).float().mean() > 0.5
