"""What the five image-pipeline handles share (csrc/vg_handle.hpp, visgeom_amd/_handle.py), on the GPU: the per-item counters
when one handle's buffers grow and are then reused with room to spare, and the stream hand-off of every wrapper."""
import numpy as np
import pytest

from tests import depth_scene as ds
from tests import motion_ref as mr
from tests import motion_scene as ms
from tests import photometric_scene as ps
from tests import sparse_odom_scene as ss
from tests import stereo_scene

pytestmark = pytest.mark.gpu
ORDER = (1, 3, 2)   # items per call on one handle: the capacity grows, then is reused with room to spare


@pytest.fixture(scope="module")
def torch():
    import torch

    from visgeom_amd import _build

    _build.build()
    return torch


def cuda(torch, *a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def stereo_params(p):
    from visgeom_amd import stereo

    return stereo.make_params(**{k: v for k, v in p.items() if k != "gradient_thresh"})


def fusion():
    from visgeom_amd import depth_fusion

    return depth_fusion.DepthFusion(ds.CAM, stereo_params(ms.prm_of("sideways")))


def depth_items():
    """three pairs of (depth, sigma) maps that differ: tests/depth_scene.py's two synthetic maps, each shifted sideways by its
    own step per item"""
    a, b = ds.synthetic_maps(mr.params(**ms.prm_of("sideways")))
    return [[[np.roll(m, shift * k, axis=1) for m in maps[:2]] for maps, shift in ((a, 7), (b, 3))] for k in range(3)]


def batch(torch, items, n, which):
    """the maps `which` of the first n items as a (depth, sigma) batch on the GPU"""
    return cuda(torch, *[np.stack([items[k][which][j] for k in range(n)]) for j in range(2)])


def test_merge_counters_when_the_items_grow_and_shrink(torch):
    items = depth_items()
    alone = []
    for one, two in items:
        h = fusion()
        t1 = cuda(torch, *one)
        h.merge(t1, cuda(torch, *two))
        alone.append((t1, h.counts[0].copy()))
        h.close()
    assert len({tuple(c) for _, c in alone}) == 3 and all((c > 20).all() for _, c in alone)   # the items differ; every outcome
    h = fusion()
    for n in ORDER:
        t1 = batch(torch, items, n, 0)
        h.merge(t1, batch(torch, items, n, 1))
        assert h.counts.shape == (n, 5)
        for k in range(n):
            assert torch.equal(t1[0][k], alone[k][0][0]) and torch.equal(t1[1][k], alone[k][0][1]), (n, k)
            assert np.array_equal(h.counts[k], alone[k][1]), (n, k)
    h.close()


def test_filter_noise_counters_when_the_items_grow_and_shrink(torch):
    items = depth_items()
    alone = []
    for one, _ in items:
        h = fusion()
        alone.append((h.filter_noise(cuda(torch, *one)), h.counts[0].copy()))
        h.close()
    assert len({tuple(c) for _, c in alone}) == 3 and all((c > 20).all() for _, c in alone)
    h = fusion()
    for n in ORDER:
        src = batch(torch, items, n, 0)
        got = h.filter_noise(src)
        c_out = h.counts.copy()
        h.filter_noise(src, out=src)   # in place: through the handle's copy, which grows and shrinks with n as well
        assert c_out.shape == (n, 3) and np.array_equal(h.counts, c_out)
        for k in range(n):
            for j in range(2):
                assert torch.equal(got[j][k], alone[k][0][j]) and torch.equal(src[j][k], alone[k][0][j]), (n, k, j)
            assert np.array_equal(c_out[k], alone[k][1]), (n, k)
    h.close()


@pytest.mark.parametrize("with_prior", [False, True], ids=["noprior", "prior"])
def test_motion_stereo_counters_when_the_items_grow_and_shrink(torch, with_prior):
    from visgeom_amd import motion_stereo

    p = ms.prm_of("forward")
    key = ds.view([0.] * 6)   # camera 1 at the origin
    noise = np.random.default_rng(3)
    base = np.stack([np.clip(key.astype(int) + noise.integers(-4, 5, key.shape), 0, 255).astype(np.uint8) for _ in range(3)])
    poses = [stereo_scene.RIGS["sideways"], stereo_scene.RIGS["vertical"], stereo_scene.RIGS["forward"]]
    tb, tv = cuda(torch, base, np.stack([ms.view(list(q)) for q in poses]))
    prior = None
    if with_prior:
        rng = ds.true_range([0.] * 6, mr.params(**p))
        dep = np.stack([np.where(rng > 0, rng * (1. + 0.02 * k), 0.) for k in range(3)])
        prior = cuda(torch, dep, np.full_like(dep, 0.15), np.full_like(dep, 60.))

    def handle():
        return motion_stereo.MotionStereo(stereo_scene.CAM1, stereo_scene.CAM2, motion_stereo.make_params(**p))

    alone = []
    for k in range(3):
        h = handle()
        h.set_base(tb[k])
        alone.append((h.compute(poses[k], tv[k], None if prior is None else [t[k] for t in prior]), h.counts[0].copy()))
        h.close()
    assert len({tuple(c) for _, c in alone}) == 3 and all(c[5] > 100 for _, c in alone)
    h = handle()
    h.set_base(tb)
    for n in ORDER:
        got = h.compute(poses[:n], tv[:n], None if prior is None else [t[:n] for t in prior])
        assert h.counts.shape == (n, 6)
        for k in range(n):
            for j in range(3):
                assert torch.equal(got[j][k], alone[k][0][j]), (n, k, j)
            assert np.array_equal(h.counts[k], alone[k][1]), (n, k)
    h.close()


# ---- the stream hand-off: (handle, call); call() makes its inputs on torch's current stream and returns every output

def _stereo(torch):
    from visgeom_amd import stereo

    images, poses = ds.sequence("sideways")
    h = stereo.Stereo(ds.CAM, ds.CAM, poses[1], stereo_params(ms.prm_of("sideways")))
    a, b = cuda(torch, images[0], images[1])
    return h, lambda: list(h.compute(a + 0, b + 0))


def _motion_stereo(torch):
    from visgeom_amd import motion_stereo

    images, poses = ds.sequence("sideways")
    h = motion_stereo.MotionStereo(ds.CAM, ds.CAM, motion_stereo.make_params(**ms.prm_of("sideways")))
    a, b = cuda(torch, images[0], images[1])

    def call():
        h.set_base(a + 0)
        return list(h.compute(poses[1], b + 0)) + [h.counts]

    return h, call


def _depth_fusion(torch):
    h = fusion()
    d, s = cuda(torch, *depth_items()[0][0])
    return h, lambda: list(h.filter_noise([d + 0, s + 0])) + [h.counts]


def _photometric(torch):
    from visgeom_amd import photometric, stereo

    s = ps.scene()
    h = photometric.Photometric(ps.CAM, stereo.make_params(equal_margins=0, **ps.PRM), ps.XI_BASE_CAM, ps.W, ps.H, ps.NUM_SCALES)
    img, depth = cuda(torch, s["base"], s["depth"])

    def call():
        h.set_base(img + 0, depth + 0)
        return list(h.level(0)) + list(h.pack(0))

    return h, call


def _sparse_odom(torch):
    from visgeom_amd import sparse_odom

    h = sparse_odom.SparseOdometry(ss.CAM, ss.XI_BASE_CAM, ss.W, ss.H)
    img = cuda(torch, ss.images()[0])[0]
    return h, lambda: [h.response(img + 0)]


@pytest.mark.parametrize("case", [_stereo, _motion_stereo, _depth_fusion, _photometric, _sparse_odom], ids=lambda f: f.__name__[1:])
def test_a_call_from_another_stream_gives_the_bits_of_a_call_from_the_handles_own(torch, case):
    h, call = case(torch)
    assert h._stream == torch.cuda.current_stream(h.device)
    side = torch.cuda.Stream(h.device)
    with torch.cuda.stream(side):
        other = call()
        side.synchronize()
    own = call()
    assert len(own) == len(other) >= 1
    for a, b in zip(own, other):
        if isinstance(a, np.ndarray):
            assert a.size and np.array_equal(a, b)
        else:
            assert a.numel() and torch.equal(a, b)
    h.close()
