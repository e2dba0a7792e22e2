"""Line detection without a GPU: the cases of tests/hough_scene.py exercise the branch each is for, the restatement
(tests/hough_ref.py) finds the lines that were drawn, the library's host entries -- vg_hough_polynomial, vg_hough_end_points,
vg_hough_trace -- equal the restatement bit for bit, and vg_hough_create refuses every limit before HIP is touched."""
import ctypes
import math

import numpy as np
import pytest

from tests import hough_ref, hough_scene, stereo_ref

_dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def lib():
    from visgeom_amd import _build, capi

    _build.build()
    return capi.load()


# the counters each case is for (a condition on the case, not a measurement): all must be positive in the restatement
LIVE = {"five_lines": ("selected", "first_votes", "antipode_votes"), "odd": ("selected", "first_votes", "antipode_votes"),
        "small_acc": ("outside",), "no_reconstruct": ("not_reconstructed",), "flat": ("failed_projections", "outside"),
        "one_line": ("first_votes", "antipode_votes")}


@pytest.mark.parametrize("name", sorted(hough_scene.CASES))
def test_every_case_exercises_its_branch(name):
    ref = hough_scene.reference(name)
    counts = dict(zip(hough_ref.COUNTS, ref["counts"].tolist()))
    print(name, counts, "lines", len(ref["lines"]), "bins hit", int((ref["acc"] > 0).sum()), "fullest", int(ref["acc"].max()))
    for k in LIVE[name]:
        assert counts[k] > 0, (name, k, counts)
    # the counters add up: every selected pixel is dropped or casts, fails or misses its first vote
    assert counts["selected"] >= counts["not_reconstructed"] + counts["first_votes"]
    assert int(ref["acc"].sum()) == counts["first_votes"] + counts["antipode_votes"]
    assert len(ref["lines"]) > 0
    if name == "one_line":
        assert int((ref["acc"] > 0).sum()) <= 16   # every vote in about a dozen bins
    if name == "odd":
        assert ref["acc"].shape == (81, 81)


def test_the_restatement_finds_the_drawn_lines():
    hough_scene.check_truth("five_lines", hough_scene.reference("five_lines")["lines"])


def all_lines():
    """(case, camera, width, height, raw normal, line) of every line the restatement finds"""
    out = []
    for name in sorted(hough_scene.CASES):
        img, cam, acc_cam, _ = hough_scene.case(name)
        for L in hough_scene.reference(name)["lines"]:
            out.append((name, cam, img.shape[1], img.shape[0], stereo_ref.reconstruct(acc_cam, L[0], L[1]), L))
    return out


def test_polynomial_is_the_restatement_bit_for_bit(lib):
    from visgeom_amd import hough

    planes = [(cam, n) for _, cam, _, _, n, _ in all_lines()]
    cam = hough_scene.case("five_lines")[1]
    linear = [(1., 0.4, 0.01), (-0.3, 0.2, 0.001), (0., 1., 0.)]   # C^2 fu fv / (A^2 + B^2) < 1: the curve through the centre
    for n in linear:
        assert n[2] * n[2] * cam[2] * cam[3] / (n[0] * n[0] + n[1] * n[1]) < 1
        planes.append((cam, n))
    planes.append((cam, (0., 0., 1.)))   # A = B = 0: the quadratic branch by its first condition
    branches = set()
    for c, n in planes:
        got, want = hough.polynomial(c, n), np.array(hough_ref.polynomial(c, n))
        assert got.tobytes() == want.tobytes(), (n, got, want)
        branches.add(bool(got[0] == 0 and got[1] == 0 and got[2] == 0))
    assert branches == {True, False}


def test_closed_form_k1_agrees_with_the_epipole_anchored_polynomial(lib):
    """the conic of a plane through the ray of pixel q passes through q: the closed-form k1 against the stereo handles'
    computePolynomial, which anchors k1 at a point of the curve (vg_stereo_host.hpp, restated in stereo_ref)"""
    from visgeom_amd import hough

    cam = hough_scene.case("five_lines")[1]
    for q, w in (((100., 80.), (0.3, -0.5, 1.)), ((31., 17.), (1., 0.2, 0.1)), ((140., 60.), (0., 1., 0.4))):
        X = stereo_ref.reconstruct(cam, *q)
        n = stereo_ref.cross3(X, w)
        got = hough.polynomial(cam, n)
        want = stereo_ref.compute_polynomial(cam, q, n).k
        assert got[0] != 0   # the quadratic branch
        assert got[:5].tolist() == list(want[:5])
        assert abs(got[5] - want[5]) <= 1e-9 * abs(want[5]), (got[5], want[5])


def test_end_points_and_trace_are_the_restatement(lib):
    from visgeom_amd import capi, hough

    n_traced = 0
    for name, cam, w, h, n, L in all_lines():
        pts, status = hough.end_points(w, h, cam, n, L[6:12])
        assert status == capi.HOUGH_OK and pts.tobytes() == L[12:16].tobytes(), (name, pts, L[12:16])
        got, want = hough.trace(L[6:12], pts), hough_ref.trace(L[6:12], L[12:16])
        assert got.shape == want.shape and np.array_equal(got, want), name
        assert 0 < len(got) < hough_ref.MAX_TRACE
        n_traced += len(got)
        # rasterising the plane's conic: the 3 x 3 neighbourhood of every traced pixel inside the image holds rays on both
        # sides of the plane
        for u, v in got.tolist():
            if not (0 <= u < w and 0 <= v < h):
                continue
            sides = set()
            for du in (-1, 0, 1):
                for dv in (-1, 0, 1):
                    X = stereo_ref.reconstruct(cam, float(u + du), float(v + dv))
                    if X is not None:
                        sides.add(stereo_ref.dot3(n, X) > 0)
            assert len(sides) == 2, (name, u, v)
    assert n_traced > 1000
    # a shorter limit cuts the same walk
    name, cam, w, h, n, L = all_lines()[0]
    assert np.array_equal(hough.trace(L[6:12], L[12:16], 10), hough_ref.trace(L[6:12], L[12:16])[:10])
    assert len(hough.trace(L[6:12], L[12:16], 0)) == 0


def test_end_points_on_random_planes_and_cameras(lib):
    """anisotropic cameras reach the "no end points" status (the circle of findCircleIntersections has the radii r fu, r fv, the
    one of distanceCheck the radius sqrt(fu fv) r): both statuses, equal to the restatement"""
    from visgeom_amd import capi, hough

    rng = np.random.default_rng(1)
    seen = {capi.HOUGH_OK: 0, capi.HOUGH_NO_END_POINTS: 0}
    for _ in range(400):
        cam = [rng.uniform(0.3, 0.9), rng.uniform(0.5, 2.5), rng.uniform(20, 120), rng.uniform(20, 120), rng.uniform(20, 140), rng.uniform(20, 100)]
        n = rng.normal(size=3)
        n[2] = abs(n[2]) * rng.choice([1, 0.1, 0.01])
        poly = hough.polynomial(cam, n)
        assert poly.tolist() == hough_ref.polynomial(cam, n)
        pts, status = hough.end_points(160, 120, cam, n, poly)
        want = hough_ref.end_points(160, 120, cam, n, poly.tolist())
        seen[status] += 1
        if want is None:
            assert status == capi.HOUGH_NO_END_POINTS and np.isnan(pts).all()
        else:
            assert status == capi.HOUGH_OK and pts.tolist() == want
            assert np.array_equal(hough.trace(poly, pts), hough_ref.trace(poly.tolist(), want))
    assert seen[capi.HOUGH_OK] > 20 and seen[capi.HOUGH_NO_END_POINTS] > 20, seen


def test_host_entries_check_their_arguments(lib):
    from visgeom_amd import capi

    six, three, four = (ctypes.c_double * 6)(0.5, 1, 30, 30, 64, 64), (ctypes.c_double * 3)(0, 1, 0.5), (ctypes.c_double * 4)(0, 0, 5, 5)
    out6, st, n = (ctypes.c_double * 6)(), ctypes.c_int(), ctypes.c_int()
    uv = (ctypes.c_int32 * 20)()
    bad = capi.ERR_INVALID_ARGUMENT
    assert lib.vg_hough_polynomial(None, three, out6) == bad and lib.vg_hough_polynomial(six, three, None) == bad
    assert lib.vg_hough_end_points(0, 10, six, three, six, four, ctypes.byref(st)) == bad
    assert lib.vg_hough_end_points(10, 16385, six, three, six, four, ctypes.byref(st)) == bad
    assert lib.vg_hough_end_points(10, 10, six, three, six, None, ctypes.byref(st)) == bad
    assert lib.vg_hough_trace(six, four, 10, uv, None) == bad and lib.vg_hough_trace(six, four, 10, None, ctypes.byref(n)) == bad
    assert lib.vg_hough_trace(six, four, -1, uv, ctypes.byref(n)) == bad
    assert lib.vg_hough_trace(six, four, capi.HOUGH_MAX_TRACE + 1, uv, ctypes.byref(n)) == bad
    for pt in ((math.nan, 0, 5, 5), (0, 0, 5, 2. ** 24 + 2), (-math.inf, 0, 5, 5)):
        assert lib.vg_hough_trace(six, (ctypes.c_double * 4)(*pt), 10, uv, ctypes.byref(n)) == bad


def test_create_refuses_every_limit_before_hip_is_touched(lib):
    """without a GPU a valid call ends in VG_ERR_NO_DEVICE; every argument error must come first"""
    from visgeom_amd import capi, hough

    cam, acc = (0.57, 1.1, 60., 60., 80., 60.), (0.5, 1., 30., 30., 64., 64.)

    def create(width=160, height=120, cam=cam, acc=acc, params=True, out=True, **fields):
        h = ctypes.c_void_p()
        c = (ctypes.c_double * 6)(*cam) if cam is not None else None
        a = (ctypes.c_double * 6)(*acc) if acc is not None else None
        p = hough.make_params(**fields)
        rc = lib.vg_hough_create(ctypes.byref(h) if out else None, 0, None, width, height, c, a, ctypes.byref(p) if params else None)
        if rc == capi.OK:
            lib.vg_hough_destroy(h)
        else:
            assert not h.value
        return rc

    bad = capi.ERR_INVALID_ARGUMENT
    assert create() in (capi.OK, capi.ERR_NO_DEVICE)
    assert create(params=False) in (capi.OK, capi.ERR_NO_DEVICE)
    assert create(out=False) == bad and create(cam=None) == bad and create(acc=None) == bad
    # image sides in [2 margin + 3, 16384]
    assert create(width=12) == bad and create(height=12) == bad and create(width=16385) == bad and create(height=16385) == bad
    assert create(width=13, height=13) in (capi.OK, capi.ERR_NO_DEVICE)
    assert create(width=16384, height=16384) in (capi.OK, capi.ERR_NO_DEVICE)
    assert create(width=16, margin=7) == bad and create(width=17, margin=7) in (capi.OK, capi.ERR_NO_DEVICE)
    assert create(margin=0) == bad and create(margin=-1) == bad
    # accumulator sides (int)(2 u0), (int)(2 v0) in [2 search_size + 3, 4096]
    small, fits = (0.5, 1., 30., 30., 3.4, 64.), (0.5, 1., 30., 30., 3.5, 64.)
    assert create(acc=small) == bad and create(acc=small[:4] + (64., 3.4)) == bad and create(acc=fits) in (capi.OK, capi.ERR_NO_DEVICE)
    assert create(acc=(0.5, 1., 30., 30., 2048.5, 64.)) == bad and create(acc=(0.5, 1., 30., 30., 64., 2048.5)) == bad
    assert create(acc=(0.5, 1., 30., 30., 2048.4, 2048.)) in (capi.OK, capi.ERR_NO_DEVICE)
    assert create(acc=(0.5, 1., 30., 30., 5., 64.), search_size=4) == bad   # 10 < 2 * 4 + 3
    assert create(search_size=0) == bad and create(search_size=9) == bad
    assert create(acc=fits, blur_size=15) == bad   # a side below the blur's radius + 1
    # blur_size odd and in [3, 15]
    for b in (1, 2, 4, 16, 17, -3):
        assert create(blur_size=b) == bad, b
    for b in (3, 15):
        assert create(blur_size=b) in (capi.OK, capi.ERR_NO_DEVICE)
    assert create(blur_sigma=0.) == bad and create(blur_sigma=-1.) == bad
    # non-finite values
    for f in ("grad_thresh", "acc_thresh", "acc_delta_thresh", "horizon_ratio", "blur_sigma"):
        assert create(**{f: math.nan}) == bad and create(**{f: math.inf}) == bad, f
    assert create(cam=(0.57, math.nan, 60., 60., 80., 60.)) == bad and create(acc=(0.5, 1., math.inf, 30., 64., 64.)) == bad
    assert create(cam=(0.57, 1.1, 0., 60., 80., 60.)) == bad and create(acc=(0.5, 1., 30., 0., 64., 64.)) == bad
    assert create(blur_size=4) == bad and b"blur_size" in lib.vg_last_error()   # a refusal leaves its message


def test_calls_check_their_arguments_without_a_handle(lib):
    from visgeom_amd import capi

    bad = capi.ERR_INVALID_ARGUMENT
    cnt = (ctypes.c_int32 * 1)()
    assert lib.vg_hough_vote(None, 1, 1, 1, None) == bad and lib.vg_hough_vote(None, -1, None, None, None) == bad
    assert lib.vg_hough_vote(None, 65536, 1, 1, None) == bad
    assert lib.vg_hough_detect(None, 1, 1, 4, None, None, cnt, None) == bad
    assert lib.vg_hough_detect(None, 1, 1, -1, None, None, cnt, None) == bad
    assert lib.vg_hough_detect(None, 1, 1, capi.HOUGH_MAX_LINES + 1, None, None, cnt, None) == bad
    w, h = ctypes.c_int(), ctypes.c_int()
    assert lib.vg_hough_size(None, ctypes.byref(w), ctypes.byref(h)) == bad
    lib.vg_hough_destroy(None)
    p = capi.HoughParams()
    lib.vg_hough_params_default(ctypes.byref(p))
    assert (p.margin, p.grad_thresh, p.search_size, p.acc_thresh, p.acc_delta_thresh, p.horizon_ratio, p.blur_size, p.blur_sigma) == \
        (5, 0.001, 2, 7., 0.05, 3e-3, 5, 0.9)
