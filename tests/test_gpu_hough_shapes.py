"""Line detection on the GPU against the numpy restatement (tests/hough_ref.py) on the cases of tests/hough_shapes.py: accumulators
that are not square, anisotropic cameras, every parameter at the ends of its range, a loaded compaction, both statuses, both
reasons for dropping a candidate maximum and the three threshold comparisons at equality.  tests/test_hough_shapes_cpu.py shows
that each case is live.

What may differ: nothing, for the reasons of tests/test_gpu_hough.py.  The accumulator, the six counters, the blurred accumulator
and every field of every line are compared for equal bits; no tolerance appears.

The mistakes each case is there to catch (vg_hough.hpp), by reading the kernels against the cases:
  acc_w for acc_h in vote_bin's bin or its bounds     aniso, aniso_tall: every vote with cv > 0 lands in another bin (test_accumulator)
  ... in the blur's row or column addressing          aniso, aniso_tall, blur15_min_side (8 x 40): other taps, other folds (test_blur)
  ... in maximum_at's border test or its row stride   blur3_search8 (19 x 50: the maximum's row 40 is refused), aniso* (test_detect)
  ... in pix % acc_w, pix / acc_w                     every non-square case: the bins are read transposed (test_detect)
  fu for fv, u0 for v0 of either camera               aniso, aniso_tall, no_end_points: all four differ in both cameras
  <= for < in the gradient test                       equal_grad: 3 selected pixels fewer, counter and accumulator
  <= for < in val < acc_thresh                        equal_acc: the lowest maximum is lost
  < for <= in val <= neighbour + delta                tie: two lines where there are none; tie_broken guards the other direction
  rec.n[2] < 0 or the failed reconstruction ignored   behind, behind_not_reconstructed, many_maxima (22 behind): lines too many
  the order of waves or lanes inside a block          many_maxima*: blocks with up to 5 and 8 maxima, compared in raster order
  the cut applied per block, or offsets not restarted test_max_lines_cuts_inside_a_block, the mixed batch
  the scan's runs of several blocks (above 256)       many_maxima*: 258 blocks, two to a thread, maxima in both of a run
  a halo that reads past a margin of 1                margin1_*, min_image: selected pixels beside the clamped halo
  reflect101 off by one on a side of r + 1            blur15_min_side
  the horizon test's direction or a missing antipode  horizon_all, horizon_none, horizon_negative"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hough_dump, hough_ref
from tests import hough_shapes as hs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    """every case through vote and detect, once"""
    return {name: hough_dump.run(name, hs, hs.MAX_LINES) for name in hs.NAMES}


def assert_lines_equal(lines, status, ref, k=None):
    """the first k lines of the restatement (all by default), field by field, for equal bits"""
    want, want_status = (ref["lines"], ref["status"]) if k is None else (ref["lines"][:k], ref["status"][:k])
    assert lines.shape == want.shape and status.shape == want_status.shape
    for field, sl in (("centroid", slice(0, 2)), ("value", slice(2, 3)), ("normal", slice(3, 6)), ("poly6", slice(6, 12))):
        assert lines[:, sl].tobytes() == want[:, sl].tobytes(), (field, lines[:, sl], want[:, sl])
    assert np.array_equal(lines[:, 12:], want[:, 12:], equal_nan=True)
    assert status.tolist() == want_status.tolist()


@pytest.mark.parametrize("name", hs.NAMES)
def test_accumulator_and_counters(gpu, name):
    ref, got = hs.reference(name), gpu[name]
    print(name, dict(zip(hough_ref.COUNTS, got["counts"].tolist())))
    assert got["acc"].dtype == np.int32 and got["acc"].shape == ref["acc"].shape
    assert np.array_equal(got["acc"], ref["acc"]), "%d bins differ" % int((got["acc"] != ref["acc"]).sum())
    assert got["counts"].tolist() == ref["counts"].tolist()


@pytest.mark.parametrize("name", hs.NAMES)
def test_blur(gpu, name):
    ref, got = hs.reference(name), gpu[name]
    assert got["blur"].dtype == np.float32 and got["blur"].shape == ref["blur"].shape
    assert got["blur"].tobytes() == ref["blur"].tobytes(), "%d bins differ" % int((got["blur"] != ref["blur"]).sum())


@pytest.mark.parametrize("name", hs.NAMES)
def test_detect(gpu, name):
    ref, got = hs.reference(name), gpu[name]
    print(name, "lines", int(got["count"][0]), "status", got["status"].tolist()[:8])
    assert int(got["count"][0]) == len(ref["lines"]) <= hs.MAX_LINES
    assert_lines_equal(got["lines"], got["status"], ref)
    if name == "no_end_points":   # the status comes out of vg_hough_detect, with NaN end points
        from visgeom_amd import capi

        assert set(got["status"].tolist()) == {capi.HOUGH_OK, capi.HOUGH_NO_END_POINTS}
        assert np.isnan(got["lines"][got["status"] == capi.HOUGH_NO_END_POINTS, 12:]).all()


def handle(name):
    import torch

    from visgeom_amd import hough

    img, cam, acc_cam, prm = hs.case(name)
    return hough.Hough(cam, acc_cam, img.shape[1], img.shape[0], hough.make_params(**prm)), torch.from_numpy(np.array(img)).cuda()


def test_max_lines_cuts_inside_a_block():
    """every max_lines around the count and one that falls between two maxima of one block of 256 bins: the restatement's first
    min(max_lines, count) lines in raster order, and the full count"""
    ref = hs.reference("many_maxima")
    count, inside = len(ref["lines"]), hs.cut_inside_a_block("many_maxima")
    h, dev = handle("many_maxima")
    for m in (0, 1, inside, count - 1, count, count + 1):
        lines, status, n = h.detect(dev, m)
        assert n == count and len(lines) == min(m, count), m
        assert_lines_equal(lines, status, ref, min(m, count))
    h.close()


def test_one_handle_across_max_lines():
    """the record stride follows max_lines while the buffers only grow: 200, then 3, then 200 again"""
    ref = hs.reference("many_maxima")
    h, dev = handle("many_maxima")
    first, small, third = h.detect(dev, 200), h.detect(dev, 3), h.detect(dev, 200)
    h.close()
    assert_lines_equal(first[0], first[1], ref, min(200, len(ref["lines"])))
    assert_lines_equal(small[0], small[1], ref, 3)
    assert first[2] == small[2] == third[2] == len(ref["lines"])
    assert first[0].tobytes() == third[0].tobytes() and first[1].tobytes() == third[1].tobytes()


@pytest.fixture(scope="module")
def batch():
    """the mixed batch through vote and detect on one handle, twice: [(acc, counts, blur, results)]"""
    import torch

    from visgeom_amd import hough

    img, cam, acc_cam, prm = hs.case("many_maxima")
    h = hough.Hough(cam, acc_cam, img.shape[1], img.shape[0], hough.make_params(**prm))
    dev = torch.from_numpy(np.stack([hs.batch_image(item) for item in hs.BATCH])).cuda()
    runs = []
    for _ in range(2):
        acc = h.vote(dev).cpu().numpy()
        counts = h.counts.copy()
        res, blur = h.detect(dev, hs.MAX_LINES, blur=True)
        runs.append((acc, counts, blur.cpu().numpy(), res))
    h.close()
    return runs


def test_a_mixed_batch_equals_the_restatement_item_by_item(batch):
    """items of 155, 0, some and 155 maxima: the scan offsets restart with every item"""
    for acc, counts, blur, res in batch:
        for k, item in enumerate(hs.BATCH):
            ref = hs.batch_reference(item)
            lines, status, count = res[k]
            assert count == len(ref["lines"]), (k, item)
            assert blur[k].tobytes() == ref["blur"].tobytes(), (k, item)
            assert_lines_equal(lines, status, ref)
        assert res[0][0].tobytes() == res[3][0].tobytes() and res[0][1].tobytes() == res[3][1].tobytes() and res[0][2] == res[3][2]
        assert blur[0].tobytes() == blur[3].tobytes()
        assert res[1][2] == 0 and res[1][0].shape == (0, 16)


def test_items_of_vote(batch):
    for acc, counts, _, _ in batch:
        assert acc.dtype == np.int32 and counts.shape == (len(hs.BATCH), 6)
        for k, item in enumerate(hs.BATCH):
            ref = hs.batch_reference(item)
            assert np.array_equal(acc[k], ref["acc"]), (k, item)
            assert counts[k].tolist() == ref["counts"].tolist(), (k, item)
        assert not acc[1].any() and counts[1].tolist() == [0] * 6   # the blank item


def test_production_library_gives_the_same_bytes(gpu, tmp_path):
    from visgeom_amd import _build

    assert os.path.exists(_build.PRODUCTION_LIB), "python -m visgeom_amd._build --production (or __graft_entry__.build())"
    path = str(tmp_path / "production.npz")
    env = dict(os.environ, VISGEOM_AMD_LIBRARY="production")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "hough_dump.py"), path, "shapes"], env=env, cwd=ROOT, timeout=300)
    got = np.load(path)
    assert int(got["has_hooks"][0]) == 0 and "production" in str(got["library"][0])
    for name in hs.NAMES:
        for k, v in gpu[name].items():
            assert got[name + "." + k].tobytes() == np.asarray(v).tobytes(), (name, k)
