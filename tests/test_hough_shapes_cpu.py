"""The conditions the cases of tests/hough_shapes.py have to meet for tests/test_gpu_hough_shapes.py to test what it says,
asserted on the restatement alone (tests/hough_ref.py): conditions on the cases, not measurements.  No GPU."""
import math

import numpy as np
import pytest

from tests import hough_ref
from tests import hough_shapes as hs

TILE_W, TILE_H = 64, 16   # the vote kernel's tile


def selected_pixels(name):
    """bool [height, width]: the pixels the vote visits and selects"""
    img, _, _, prm = hs.case(name)
    kx, ky = hough_ref.sobel(img)
    m = prm["margin"]
    sel = np.zeros(img.shape, dtype=bool)
    sel[m:img.shape[0] - m, m:img.shape[1] - m] = True
    return sel & ~((kx * kx + ky * ky) / 4194304. < prm["grad_thresh"])


@pytest.mark.parametrize("name", hs.NAMES)
def test_every_case_is_live(name):
    img, cam, acc_cam, prm = hs.case(name)
    ref, st, need = hs.reference(name), hs.stats(name), hs.NEED[name]
    counts = dict(zip(hough_ref.COUNTS, ref["counts"].tolist()))
    aw, ah = hough_ref.acc_size(acc_cam)
    per_block = hs.maxima_per_block(name)
    print(name, "image %d x %d" % img.shape[::-1], "accumulator %d x %d, %d blocks" % (aw, ah, hs.blocks_of(aw * ah)), counts,
          "first", st["first"], "antipode", st["antipode"], "of", st["antipode_tried"], "| lines", len(ref["lines"]), "status 1:",
          int(ref["status"].sum()), "| window", st["window"], "behind", st["behind"], "not reconstructed", st["not_reconstructed"],
          "| fullest block", int(per_block.max()), "blocks with 3 or more", int((per_block >= 3).sum()))
    assert max(img.shape) <= 160 and img.size <= 160 * 120 and max(aw, ah) <= 300 and aw * ah <= 300 * 220   # tests stay quick
    # the counter identities of tests/test_hough_cpu.py, and those of the two kinds of vote
    assert counts["selected"] >= counts["not_reconstructed"] + counts["first_votes"]
    assert int(ref["acc"].sum()) == counts["first_votes"] + counts["antipode_votes"]
    assert sum(st["first"]) == counts["selected"] - counts["not_reconstructed"] and sum(st["antipode"]) == st["antipode_tried"]
    assert counts["selected"] == int(selected_pixels(name).sum())
    assert st["window"] == len(ref["lines"]) + st["behind"] + st["not_reconstructed"] and len(st["bins"]) == len(ref["lines"])
    assert ref["acc"].shape == (ah, aw)
    for key, want in need.items():
        if key == "acc":
            assert (aw, ah) == want and aw != ah
        elif key == "blocks_over":
            assert hs.blocks_of(aw * ah) > want   # so a thread of the scan sums a run of two blocks: maxima in both of a run
            assert ((per_block[0:-1:2] > 0) & (per_block[1::2] > 0)).any()
        elif key == "lines_over":
            assert len(ref["lines"]) > want
        elif key == "blocks_with_3":
            assert int((per_block >= 3).sum()) >= want and int((per_block >= 2).sum()) > want
        elif key == "statuses":
            assert set(ref["status"].tolist()) == want
            assert np.isnan(ref["lines"][ref["status"] == 1, 12:]).all() and np.isfinite(ref["lines"][ref["status"] == 0]).all()
        elif key == "positive":
            for k in want:
                assert counts[k] > 0, k
        elif key == "lines":
            assert len(ref["lines"]) > 0
        elif key == "inside":
            assert counts["first_votes"] + counts["antipode_votes"] > 0
        elif key == "border_selected":   # a selected pixel whose Sobel window touches the image's border: the halo beside it is clamped
            sel = selected_pixels(name)
            assert prm["margin"] == 1 and (sel[1].any() or sel[-2].any()) and (sel[:, 1].any() or sel[:, -2].any())
        elif key == "empty_tiles":
            sel = np.zeros(img.shape, dtype=bool)
            m = prm["margin"]
            sel[m:img.shape[0] - m, m:img.shape[1] - m] = True
            tiles = [sel[y:y + TILE_H, x:x + TILE_W].any() for y in range(0, img.shape[0], TILE_H) for x in range(0, img.shape[1], TILE_W)]
            assert tiles.count(False) == want and m > TILE_H
        elif key == "antipode":
            if want == "all":   # every voting pixel also tries its antipode
                assert st["antipode_tried"] == counts["selected"] - counts["not_reconstructed"] > 0
                assert st["antipode"][1] > 0 and st["first"][1] == 0   # projections that fail for the antipode only
                assert counts["antipode_votes"] + st["antipode"][1] + st["antipode"][2] == counts["selected"] - counts["not_reconstructed"]
            else:
                assert st["antipode_tried"] == 0 and counts["antipode_votes"] == 0 and prm["horizon_ratio"] <= 0
        elif key == "window_dropped":
            assert (st["behind"], st["not_reconstructed"]) == want
        else:
            raise AssertionError(key)


def test_the_cases_cover_the_parameter_ranges():
    """both ends of blur_size, search_size and margin, an anisotropic image and accumulator camera, a negative delta"""
    prm = [hs.case(name)[3] for name in hs.NAMES]
    for key, ends in (("blur_size", (3, 15)), ("search_size", (1, 8)), ("margin", (1, 20))):
        assert {min(p[key] for p in prm), max(p[key] for p in prm)} == set(ends), key
    assert min(p["acc_delta_thresh"] for p in prm) < 0
    for name in ("aniso", "aniso_tall", "no_end_points"):
        _, cam, acc_cam, _ = hs.case(name)
        assert cam[2] != cam[3] and cam[4] != cam[5] and acc_cam[2] != acc_cam[3] and acc_cam[4] != acc_cam[5]
    # the smallest sides the handle accepts: (blur_size + 1) / 2 and 2 search_size + 3 bins, 2 margin + 3 pixels
    assert hough_ref.acc_size(hs.case("blur15_min_side")[2])[0] == (15 + 1) // 2
    assert hough_ref.acc_size(hs.case("blur3_search8")[2])[0] == 2 * 8 + 3
    assert hs.case("min_image")[0].shape == (2 * 1 + 3, 2 * 1 + 3)
    assert hs.case("margin1_one_tile")[0].shape == (TILE_H, TILE_W) and hs.case("margin1_ragged")[0].shape == (TILE_H + 1, TILE_W + 1)


def test_reflect101_folds_across_the_whole_minimal_side():
    """on a side of r + 1 bins every tap index from -r to 2 r folds into the side without the clamp of the kernel's reflect101"""
    n, r = 8, 7
    i = np.arange(-r, n + r)
    folded = hough_ref._reflect101(i, n)
    assert folded.min() == 0 and folded.max() == n - 1
    a, b = np.abs(i), 2 * n - 2 - np.abs(i)
    assert np.array_equal(folded, np.maximum(np.minimum(a, b), 0)) and np.minimum(a, b).min() == 0   # the kernel's form; the clamp idle


def test_the_batch_items_differ():
    counts = [len(hs.batch_reference(item)["lines"]) for item in hs.BATCH]
    print("lines per item", counts)
    assert counts[0] == counts[3] > 128 and counts[1] == 0 and counts[2] > 0
    assert hs.batch_reference("blank")["counts"].tolist() == [0] * 6 and not hs.batch_reference("blank")["acc"].any()
    flipped = hs.batch_reference("flipped")
    assert counts[2] != counts[0] and flipped["lines"].tobytes() != hs.reference("many_maxima")["lines"][:counts[2]].tobytes()
    m = hs.cut_inside_a_block("many_maxima")
    bins = hs.stats("many_maxima")["bins"]
    assert 1 < m < counts[0] - 1 and bins[m - 1] // hs.LANES == bins[m] // hs.LANES   # the cut falls inside a block
    assert bins == sorted(bins)   # raster order


# ---- the three comparisons at equality: the next double changes the restatement's result -----------------------------------

def test_grad_thresh_sits_on_a_pixel_value():
    thresh, n = hs.grad_at_equality()
    img, cam, acc_cam, prm = hs.case("equal_grad")
    k = round(thresh * 4194304.)
    assert prm["grad_thresh"] == thresh == k / 4194304. and float(k) / 4194304. * 4194304. == k and n > 0
    kx, ky = hough_ref.sobel(img)
    assert int(((kx * kx + ky * ky) == k)[5:-5, 5:-5].sum()) == n
    at = hs.reference("equal_grad")["counts"][0]
    above = hough_ref.vote(*hs.with_params("equal_grad", grad_thresh=math.nextafter(thresh, math.inf)))[1][0]
    below = hough_ref.vote(*hs.with_params("equal_grad", grad_thresh=math.nextafter(thresh, 0.)))[1][0]
    print("grad_thresh %r = %d / 2^22: %d pixels at equality; selected %d at it, %d one double above" % (thresh, k, n, at, above))
    assert at - above == n and below == at   # the pixels at equality are selected, and only the threshold's last bit drops them


def test_acc_thresh_sits_on_a_maximum():
    thresh, bin_ = hs.acc_at_equality()
    prm = hs.case("equal_acc")[3]
    blur = hs.reference("equal_acc")["blur"]
    assert prm["acc_thresh"] == thresh == float(blur.ravel()[bin_]) and np.float32(thresh) == thresh
    assert hs.reference("equal_acc")["blur"].tobytes() == hs.reference("aniso")["blur"].tobytes()
    st = {}
    above = hough_ref.maxima(blur, hs.case("equal_acc")[2], dict(prm, acc_thresh=math.nextafter(thresh, math.inf)), st)
    print("acc_thresh %r: bin %d kept with %d others; one double above %d are kept" % (thresh, bin_, len(hs.stats("equal_acc")["bins"]) - 1, len(above)))
    assert bin_ in hs.stats("equal_acc")["bins"] and bin_ not in st["bins"] and len(above) == len(hs.stats("equal_acc")["bins"]) - 1


def test_the_tie_is_a_tie():
    img, _, acc_cam, prm = hs.case("tie")
    assert np.array_equal(img, img[:, ::-1])
    assert hough_ref.gaussian(3, prm["blur_sigma"]).tolist() == [0.25, 0.5, 0.25]
    blur = hs.reference("tie")["blur"]
    peak = blur.max()
    v, u = np.nonzero(blur == peak)
    s = prm["search_size"]
    assert v.tolist() == [v[0]] * 2 and u.tolist() == [24, 25] and s <= v[0] < blur.shape[0] - s   # two equal neighbouring bins
    window = blur[v[0] - s:v[0] + s + 1, 24 - s:25 + s + 1]
    assert (window == peak).sum() == 2 and peak >= prm["acc_thresh"]   # everything else in both windows is lower
    delta = hs.tie_delta()
    assert prm["acc_delta_thresh"] == 0. and hs.case("tie_broken")[3]["acc_delta_thresh"] == delta < 0
    assert float(peak) + delta == math.nextafter(float(peak), 0.)   # one double below the peak
    tied, broken = hs.stats("tie")["bins"], hs.stats("tie_broken")["bins"]
    print("peak %r in bins %s; delta 0 keeps %s, delta %r keeps %s" % (float(peak), (v * blur.shape[1] + u).tolist(), tied, delta, broken))
    both = (v * blur.shape[1] + u).tolist()
    assert not set(both) & set(tied) and set(both) <= set(broken)
    assert hs.reference("tie_broken")["blur"].tobytes() == blur.tobytes()
