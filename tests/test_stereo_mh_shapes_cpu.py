"""The conditions the inputs of tests/stereo_mh_shapes.py have to meet for tests/test_gpu_stereo_mh_shapes.py to test what it
says, asserted on the restatement alone (tests/stereo_mh_ref.py).  No GPU."""
import numpy as np
import pytest

from tests import stereo_mh_ref as smh
from tests import stereo_mh_shapes as ms
from tests import stereo_strip as strip


def assert_packs_equal(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert (ms.bits(x) == ms.bits(y)).all() if x.dtype == np.float64 else (x == y).all()


# ---- A ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", sorted(ms.SMALL))
def test_small_maps_and_the_vectorised_pack(P):
    """the vectorised pack is smh.pack_mh, bit for bit, on every small map; the random fill has entries and empty pixels, the
    other two exactly the planes of their one pixel; no pixel lies within 1e-9 of the camera's refusal"""
    for fill in ms.FILLS:
        prm, depth, sigma = ms.small(P, fill)
        assert depth.shape[1] * depth.shape[2] == P and len(np.unique(sigma)) == sigma.size
        want = smh.pack_mh(ms.CAM, prm, depth, sigma)
        assert_packs_equal(ms.pack_fast(ms.CAM, prm, depth, sigma), want)
        if fill == "random":
            assert len(want[0]) >= 1
            if P >= 63:
                assert (want[1] >= 1).sum() >= 10 and len(np.unique(want[0])) < P
                assert smh.holes(depth) >= 10   # filled planes above empty ones are emitted
        else:
            assert want[0].tolist() == [P - 1 if fill == "last" else 0] * 4 and want[1].tolist() == [0, 1, 2, 3]
        assert (np.abs(ms.directions(ms.CAM, prm)[2]) > 1e-9).all()
    if ms.SMALL[P][0] >= 255:   # one row of 255 pixels or more from u = 0 leaves the camera's field: both kinds of pixel
        seen = ms.directions(ms.CAM, ms.small(P, "random")[0])[1]
        assert seen.any() and not seen.all()


def test_hand_made_maps_and_the_vectorised_pack():
    for cam, (prm, depth, sigma) in ((ms.HAND_CAM, ms.hand_made()), (ms.CAM, ms.values()[:3]), (ms.CAM, ms.patterns()[:3]), (ms.CAM, ms.full())):
        assert_packs_equal(ms.pack_fast(cam, prm, depth, sigma), smh.pack_mh(cam, prm, depth, sigma))
        assert (np.abs(ms.directions(cam, prm)[2]) > 1e-9).all()
    idx, hyp, cloud, _ = smh.pack_mh(ms.HAND_CAM, *ms.hand_made())
    assert idx.tolist() == [0, 1, 1, 3, 3] and hyp.tolist() == [0, 0, 1, 0, 1] and (cloud[3:] == 0.).all() and (cloud[:3] != 0.).any(1).all()


@pytest.mark.parametrize("w,h", ms.BLOCK_SHAPES)
def test_block_maps(w, h):
    """256, 257 and 520 workgroups: scan runs of 1, 2 and 3; whole workgroups and whole waves without an entry between filled
    ones, workgroups near 2048 entries, a partly filled last run of the scan, refused and reconstructed pixels"""
    prm, depth, sigma = ms.blocks(w, h)
    P, nb = w * h, ms.blocks_of(w * h)
    run = (nb + ms.LANES - 1) // ms.LANES
    assert (nb, run) == {(256, 256): (256, 1), (257, 256): (257, 2), (416, 320): (520, 3)}[(w, h)]
    idx, hyp, cloud, sig = ms.pack_fast(ms.CAM, prm, depth, sigma)
    counts = ms.entries_per_block(idx, P)
    waves = np.bincount(idx // 64, minlength=nb * 4)
    inner = slice(1, nb - 1)
    print("%d x %d: entries %d, empty workgroups %d of %d, empty waves %d, largest workgroup %d" % (w, h, len(idx), (counts == 0).sum(), nb,
                                                                                                      (waves == 0).sum(), counts.max()))
    assert (counts[inner] == 0).sum() >= 20 and counts[0] + counts[-1] > 0 and counts.max() > 1024
    assert ((waves == 0) & (np.repeat(counts, 4) > 0)).sum() >= 20   # empty waves inside workgroups that have entries
    assert counts[ms.LANES:].sum() > 0 if nb > ms.LANES else True     # entries in the workgroups a scan run of 1 would not reach
    if run > 1:
        assert nb % run != 0   # the last thread of the scan in use holds a shorter run
    assert smh.holes(depth) >= 1000 and (hyp == 7).sum() >= 1000
    seen = ms.directions(ms.CAM, prm)[1][idx]
    print("    entries of reconstructed pixels %d, of refused pixels %d" % (seen.sum(), (~seen).sum()))
    assert seen.sum() >= 1000 and (~seen).sum() >= 1000
    assert (cloud[~seen] == 0.).all() and (cloud[seen] != 0.).any(1).all()
    assert (np.abs(ms.directions(ms.CAM, prm)[2]) > 1e-9).all()
    # the vectorised pack against the loop on the first and the last rows of the map
    rows = 4
    for part in (slice(0, rows), slice(h - rows, h)):
        sub = dict(prm, y_max=rows, v0=prm["v0"] + (part.start or 0))
        assert_packs_equal(ms.pack_fast(ms.CAM, sub, depth[:, part], sigma[:, part]), smh.pack_mh(ms.CAM, sub, depth[:, part], sigma[:, part]))


def test_full_map_and_patterns():
    prm, depth, sigma = ms.full()
    idx, hyp, _, _ = ms.pack_fast(ms.CAM, prm, depth, sigma)
    assert len(idx) == 8 * 257 * 3 and ms.entries_per_block(idx, 771).tolist() == [2048, 2048, 2048, 24]
    prm, depth, sigma, pat = ms.patterns()
    assert np.bincount(pat, minlength=256).min() >= 2
    idx, hyp, _, _ = ms.pack_fast(ms.CAM, prm, depth, sigma)
    for p in range(600):   # the entries of a pixel are its pattern's bits, or none when bit 0 is not set
        want = [h for h in range(8) if pat[p] >> h & 1] if pat[p] & 1 else []
        assert hyp[idx == p].tolist() == want
    assert pat[255] != pat[256] and pat[511] != pat[512]
    for K in range(1, 9):   # the first K planes alone: the patterns cut at K bits
        assert len(ms.pack_fast(ms.CAM, prm, depth[:K], sigma[:K])[0]) == sum(bin(q & (1 << K) - 1).count("1") for q in pat if q & 1)


def test_value_maps():
    prm, depth, sigma, entries = ms.values()
    idx, hyp, cloud, sig = smh.pack_mh(ms.CAM, prm, depth, sigma)
    assert list(zip(idx.tolist(), hyp.tolist())) == entries and len(entries) == 11
    assert np.isfinite(cloud).all() and (sig == sigma[hyp, 0, idx]).all()
    assert ms.BELOW < smh.MIN_DEPTH and ms.BELOW == np.nextafter(0.25, 0.)
    depth, sigma, cost, want = ms.regularize_values()
    got = smh.regularize(depth, sigma, cost)
    assert (ms.bits(got[0]) == ms.bits(want)).all()
    assert np.isnan(want).sum() == 3 and np.isnan(depth).sum() == 3


# ---- B ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", range(2, 9))
def test_exhaustive_maps(K):
    """3^K distinct pixels; a move of the wrong plane's sigma or cost would show: the values differ at every (plane, pixel)"""
    depth, sigma, cost = ms.exhaustive(K)
    P = 3 ** K
    assert depth.shape == (K, 1, P) and len(np.unique(depth.reshape(K, P).T, axis=0)) == P
    assert len(np.unique(sigma)) == sigma.size and len(np.unique(cost)) == cost.size
    d, s, c = smh.regularize(depth, sigma, cost)
    assert smh.holes(depth) > 0 and smh.holes(d) == 0
    filled = depth >= 0.25
    holed = int(((~filled) & (np.cumsum(filled[::-1], 0)[::-1] > 0)).any(0).sum())   # pixels with an empty plane under a filled one
    assert holed >= 2 and (ms.bits(d) != ms.bits(depth)).any(0).sum() == holed and (ms.bits(c) != ms.bits(cost)).any(0).sum() == holed
    # every filled depth is still there, once, on its own pixel and in the same order
    for p in (0, P // 2, P - 1, 5 % P, 7 % P):
        assert d[:, 0, p][d[:, 0, p] >= 0.25].tolist() == depth[:, 0, p][depth[:, 0, p] >= 0.25].tolist()


def test_random_maps_have_holes():
    for K in (3, 8):
        for P in sorted(ms.SMALL)[:-1]:
            depth, _, _ = ms.random_map(P, K)
            assert depth.shape[0] == K and (P < 63 or smh.holes(depth) >= 10)
    depth, _, _ = ms.random_map(259, 3, 3)
    assert depth.shape == (3, 3, 37, 7) and (3 * 259) % 64 != 0 and min(smh.holes(d) for d in depth) >= 10
    assert not (depth[0] == depth[1]).all() and not (depth[1] == depth[2]).all()


def test_chain_on_the_exhaustive_map():
    depth, sigma, cost = ms.exhaustive(8)
    d, s, _ = smh.regularize(depth, sigma, cost)
    prm = ms.grid(81, 81, -60, -60)
    idx, hyp, cloud, sig = ms.pack_fast(ms.CAM, prm, d.reshape(8, 81, 81), s.reshape(8, 81, 81))
    assert smh.holes(d) == 0 and len(idx) == (depth >= 0.25).sum()   # regularized: every filled plane is an entry
    seen = ms.directions(ms.CAM, prm)[1][idx]
    assert seen.sum() >= 1000 and (~seen).sum() >= 1000 and (np.abs(ms.directions(ms.CAM, prm)[2]) > 1e-9).all()


# ---- C ---------------------------------------------------------------------------------------------------------------

def test_strip_j_at_other_hypothesis_counts():
    """K = 3, 5, 6, 7: the last plane is filled on at least 300 pixels; K = 8: three or more candidates of one accepted cost"""
    last = []
    for K in ms.STRIP_K:
        mh = ms.strip_reference("j", K, 200)[3]
        last.append(int((mh["disparity"][K - 1] >= 0).sum()))
    print("pixels of case j whose last plane is filled, K = 3, 5, 6, 7:", last)
    assert min(last) >= 300
    _, _, base, mh = ms.strip_reference("j", 8, 200)
    n = ms.tie_pixels(base, mh, strip.prm_of("j")["error_max"])
    print("pixels with three or more candidates of an accepted cost:", n)
    assert n >= 1


@pytest.mark.parametrize("D,K", ms.DISP_MAX_CASES)
def test_rig_with_as_many_hypotheses_as_disparities(D, K):
    base, mh = ms.rig_reference(K, 1000000, disp_max=D)
    filled = [int((mh["disparity"][h] >= 0).sum()) for h in range(K)]
    print("disp_max %d: filled pixels per plane" % D, filled)
    assert filled[1] >= (50 if D == 4 else 1000) and filled[-1] >= (1 if D == 4 else 5)
    assert base["err"].shape[-1] == D == K
    for h in range(K):   # plane h of the cost is the error at index h
        live = mh["cost"][h] != 0
        assert (mh["cost"][h][live] == base["err"][..., h][live]).all()
        for g in range(h):
            assert (mh["cost"][h] != mh["cost"][g]).sum() >= 100, (g, h)


def test_hypo_difference_at_and_below_zero():
    base = strip.reference("a")[2]
    mh = {diff: ms.strip_reference("a", 3, diff)[3] for diff in ms.DIFF_CASES}
    d, c = mh[0]["disparity"], mh[0]["final_cost"]
    second = d[1] >= 0
    print("case a at hypo_difference 0: pixels with a second hypothesis", int(second.sum()))
    assert second.sum() >= 10 and (c[1][second] == c[0][second]).all()
    assert (mh[-1]["disparity"][1:] == -1).all() and (mh[-1]["final_cost"][1:] == smh.NO_COST).all()
    for diff in ms.DIFF_CASES:   # plane 0 has no gate
        assert (mh[diff]["disparity"][0] == mh[0]["disparity"][0]).all() and (mh[diff]["final_cost"][0] == c[0]).all()
    assert (mh[-1]["disparity"][0] >= 0).sum() >= 1000
    assert (mh[1000000]["disparity"][2] >= 0).sum() > (d[2] >= 0).sum()
    assert base["err"].shape[-1] == 256


def test_cost_zero_rig():
    """the same image through the same camera: disparity 0 is the same pixel, its matching error and its aggregated cost are 0,
    and it is taken in the first round only because the start state's disparity is -1"""
    for diff in (50, 1000000):
        base, mh = ms.zero_reference(4, diff)
        zero = (mh["disparity"][0] == 0) & (mh["final_cost"][0] == 0)
        print("cost-0 rig at hypo_difference %d: pixels with disparity 0 at cost 0 in plane 0" % diff, int(zero.sum()), "of", zero.size,
              "; with a second hypothesis", int((mh["disparity"][1] >= 0).sum()))
        assert zero.sum() >= 3000


def test_chunk_case_parameters():
    """the call longer than a chunk: 2 GiB over the scratch of one pair, for K = 2 and for the single hypothesis"""
    P, D = 96 * 40, 256
    assert (ms.CHUNK_PRM["x_max"], ms.CHUNK_PRM["y_max"], ms.CHUNK_PRM["disp_max"]) == (96, 40, D)
    single, mh = (2 << 30) // (P * (5 * D + 3 + 4)), (2 << 30) // (P * (5 * D + 3 + 8))
    assert mh <= single and single + 8 > mh
    out_bytes = (single + 8) * 2 * P * (3 * 8 + 2 * 4)
    print("chunk", single, "multi-hypothesis chunk", mh, "output MB", out_bytes / 1e6)
    assert out_bytes < 128e6


def test_rig_batch_pairs():
    """three different pairs, each with second hypotheses at K = 4 and K = 8 and with a filled last plane at K = 8"""
    a, b = ms.rig_pairs()
    assert a.shape == b.shape == (3,) + ms.rig_scene()[0].shape
    assert all((a[i] != a[j]).any() for i in range(3) for j in range(i))
    for i in range(3):
        four, eight = ms.rig_pair_reference(i, 4, 50)["disparity"], ms.rig_pair_reference(i, 8, 200)["disparity"]
        print("pair %d: filled pixels per plane" % i, [int((p >= 0).sum()) for p in four], [int((p >= 0).sum()) for p in eight])
        assert (four[1] >= 0).sum() >= 100 and (eight[1] >= 0).sum() >= 100 and (eight[7] >= 0).sum() >= 1
