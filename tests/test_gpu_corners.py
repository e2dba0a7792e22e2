"""Corner detection on the GPU (include/visgeom_amd.h section 8) against the numpy restatement (tests/corners_ref.py) and
against rendered checkerboards (tests/board_render.py): stage parity, detection and corner order, accuracy with and without
the subpixel refinement, negatives, batch equivalence, a call past 2^31 bytes, and calibration from image files."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import board_render as br
from tests import corners_ref

pytestmark = pytest.mark.gpu

EUCM = [0.6, 1.1, 300., 300., 400., 300.]
UCM = [0.8, 350., 350., 400., 300.]
CAMS = {"eucm": EUCM, "ucm": UCM}
W, H = 800, 600


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def cuda(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def render(model, pose, cols, rows, size=0.05, w=W, h=H, **kw):
    R, t = br.look_at_pose(cols=cols, rows=rows, size=size, **pose)
    img = br.render(model, CAMS[model], R, t, cols, rows, size, w, h, **kw)
    T, ok = br.truth(model, CAMS[model], R, t, cols, rows, size)
    assert ok and T.min() > 8 and T[:, 0].max() < w - 8 and T[:, 1].max() < h - 8, "pose leaves the image"
    return img, T


POSES = [dict(centre_cam=[0.0, 0.0, 0.5]),
         dict(centre_cam=[0.05, -0.03, 0.55], yaw=0.5, pitch=-0.3),
         dict(centre_cam=[-0.04, 0.02, 0.5], roll=0.7, pitch=0.25),
         dict(centre_cam=[-0.03, 0.05, 0.6], roll=-2.3, yaw=-0.4)]


def edge_pose(model, cols, rows, size):
    """a board pushed towards the image border, where the fisheye distortion is strongest"""
    for x in (0.45, 0.4, 0.35, 0.3, 0.25, 0.2):
        pose = dict(centre_cam=[x * 0.5 * (1 + 0.05 * cols), 0.08, 0.45], yaw=-0.4, roll=0.3)
        R, t = br.look_at_pose(cols=cols, rows=rows, size=size, **pose)
        T, ok = br.truth(model, CAMS[model], R, t, cols, rows, size)
        if ok and T.min() > 15 and T[:, 0].max() < W - 15 and T[:, 1].max() < H - 15:
            return pose
    raise AssertionError("no edge pose")


# ---- 1. stage parity ----

@pytest.mark.parametrize("w,h,kind", [(64, 48, "random"), (333, 251, "render"), (97, 61, "random"), (1920, 1080, "random")])
def test_response_maps_match_the_restatement(torch, w, h, kind):
    from visgeom_amd.corners import CornerDetector

    rng = np.random.default_rng(w * h)
    if kind == "random":
        imgs = [rng.integers(0, 256, (h, w), dtype=np.uint8), (rng.random((h, w)) * 60 + 100).astype(np.uint8)]
    else:
        imgs = [br.render("eucm", EUCM, *br.look_at_pose([0., 0., 0.5], 0.3, -0.2, 0.5, 5, 4, 0.03), 5, 4, 0.03, w, h)]
    det = CornerDetector(5, 4)
    batch = cuda(torch, np.stack(imgs))
    for sigma in corners_ref.SIGMAS:
        got = det.response(batch, sigma)
        for i, img in enumerate(imgs):
            ref = corners_ref.response(img, sigma)
            for k in ("src1", "src2"):
                assert np.array_equal(got[k][i].cpu().numpy(), ref[k]), (k, sigma, i)   # bit-identical blurs
            for k in ("gradx", "grady", "imgrad", "resp"):
                g, r = got[k][i].cpu().numpy(), ref[k]
                assert np.max(np.abs(g - r)) <= 1e-6 * max(1., np.max(np.abs(r))), (k, sigma)
            if np.isnan(ref["avg"]):
                assert np.isnan(got["avg"][i])
            else:
                assert abs(got["avg"][i] - ref["avg"]) <= 1e-12 * abs(ref["avg"]), (sigma, got["avg"][i], ref["avg"])
    det.close()


@pytest.mark.parametrize("kind", ["render", "random", "noisy_render"])
def test_candidates_match_the_restatement(torch, kind):
    from visgeom_amd.corners import CornerDetector

    cols, rows = 9, 7
    if kind == "random":
        img = np.random.default_rng(5).integers(0, 256, (121, 163), dtype=np.uint8)
    else:
        img, _ = render("eucm", POSES[1], cols, rows, noise=4. if kind == "noisy_render" else 0., seed=2)
    det = CornerDetector(cols, rows)
    for sigma in corners_ref.SIGMAS:
        uv, thresh, nmax = det.candidates(cuda(torch, img[None]), sigma)
        ref, rthresh, rnmax = corners_ref.candidates(img, sigma, cols, rows)
        assert nmax[0] == rnmax
        assert abs(thresh[0] - rthresh) <= 1e-15 * abs(rthresh)
        assert [tuple(p) for p in uv[0]] == ref, sigma
    det.close()


# ---- 2. detection on renders ----

def _check_order_and_accuracy(corners, T, tol):
    E = br.expected_order(T)
    err = np.linalg.norm(corners - E, axis=1)
    assert err.max() < tol, err.max()
    R = np.linalg.norm(corners - T[::-1] if E is T else corners - T, axis=1)
    assert R.max() > 2., "indistinguishable from the reversed assignment"
    return err


@pytest.mark.parametrize("model", ["eucm", "ucm"])
@pytest.mark.parametrize("cols,rows", [(9, 7), (12, 8), (5, 4)])
def test_detects_rendered_boards_in_the_reference_order(torch, model, cols, rows):
    from visgeom_amd.corners import CornerDetector

    size = {9: 0.04, 12: 0.03, 5: 0.06}[cols]
    poses = POSES + [edge_pose(model, cols, rows, size)]
    imgs, truths = zip(*[render(model, p, cols, rows, size) for p in poses])
    batch = cuda(torch, np.stack(imgs))
    det = CornerDetector(cols, rows)
    corners, found, sigma = det.detect(batch, return_sigma=True)
    assert found.all(), found
    worst = max(_check_order_and_accuracy(corners[i].numpy(), truths[i], 1.0).max() for i in range(len(imgs)))
    det.close()
    det = CornerDetector(cols, rows, improve=True)
    c2, f2 = det.detect(batch)
    assert f2.all()
    errs = np.concatenate([_check_order_and_accuracy(c2[i].numpy(), truths[i], 0.5) for i in range(len(imgs))])
    rms = float(np.sqrt(np.mean(errs ** 2)))
    print("%s %dx%d: max error %.3f px at pixel level, %.4f px RMS refined; sigmas %s" % (model, cols, rows, worst, rms,
                                                                                         sigma.tolist()))
    # measured on the MI355X: 0.031 to 0.038 px RMS refined, 0.65 to 0.72 px worst at pixel level (noise-free renders)
    assert rms < 0.06
    det.close()


def test_detect_pattern_wrapper_single_image(torch):
    from visgeom_amd.corners import detect_pattern

    img, T = render("eucm", POSES[0], 9, 7, 0.04)
    corners, found = detect_pattern(cuda(torch, img), 9, 7)
    assert corners.shape == (63, 2) and corners.dtype == torch.float64 and bool(found)
    _check_order_and_accuracy(corners.numpy(), T, 1.0)


# ---- 3. negatives ----

def test_blank_noise_and_cut_boards_are_not_found(torch):
    from visgeom_amd.corners import CornerDetector

    rng = np.random.default_rng(9)
    blank = np.full((H, W), 128, np.uint8)
    noise = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R, t = br.look_at_pose([0.0, 0.0, 0.45], cols=9, rows=7, size=0.05)
    off_centre = EUCM[:4] + [10., 300.]   # the principal point on the left border: the board's left half leaves the image
    cut = br.render("eucm", off_centre, R, t, 9, 7, 0.05, W, H)
    T, _ = br.truth("eucm", off_centre, R, t, 9, 7, 0.05)
    assert T[:, 0].min() < -50 and T[:, 0].max() > 50, "the board must cross the image border"
    corners, found = CornerDetector(9, 7).detect(cuda(torch, np.stack([blank, noise, cut])))
    assert not found.any()
    assert float(corners.abs().sum()) == 0.


# ---- 4. batch equivalence ----

def _defocus(img, passes=5):
    """five passes of a 5-point box blur with a wrap-around border"""
    x = img.astype(np.float64)
    for _ in range(passes):
        x = (np.roll(x, 1, 0) + np.roll(x, -1, 0) + np.roll(x, 1, 1) + np.roll(x, -1, 1) + x) / 5
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def test_batch_equals_single_calls_including_retries(torch):
    from visgeom_amd.corners import CornerDetector

    imgs = [render("eucm", p, 9, 7, 0.04)[0] for p in POSES]
    imgs += [render("ucm", POSES[2], 9, 7, 0.02)[0],                               # a small, far board
             render("eucm", POSES[1], 9, 7, 0.04, noise=10., seed=4)[0],
             render("eucm", POSES[3], 9, 7, 0.04, dark=90., light=150., gradient=(0.05, -0.04))[0],
             br.render("eucm", EUCM, *br.look_at_pose([0., 0., 1.1], cols=9, rows=7, size=0.02), 9, 7, 0.02, W, H),
             _defocus(render("eucm", POSES[0], 9, 7, 0.04)[0]),                        # found only at the sigma = 2 retry
             np.full((H, W), 70, np.uint8)]
    for improve in (False, True):
        det = CornerDetector(9, 7, improve=improve)
        cb, fb, sb = det.detect(cuda(torch, np.stack(imgs)), return_sigma=True)
        for i, img in enumerate(imgs):
            c1, f1, s1 = det.detect(cuda(torch, img[None]), return_sigma=True)
            assert bool(f1[0]) == bool(fb[i]) and float(s1[0]) == float(sb[i])
            assert np.array_equal(c1[0].numpy(), cb[i].numpy()), i
        print("improve", improve, "found", fb.tolist(), "sigma", sb.tolist())
        assert fb[:8].all() and not fb[9]
        assert float(sb[8]) == 2.0 and bool(fb[8])   # measured: the defocused board fails at 1.4 and is found at 2
        det.close()


# ---- 5. a call past 2^31 bytes ----

def test_one_call_past_2_31_bytes(torch):
    from visgeom_amd.corners import CornerDetector

    n, w, h = 280, 4096, 2048
    assert n * w * h > 2 ** 31
    pose = dict(centre_cam=[0.02, -0.01, 0.5], yaw=0.3, roll=0.4)
    cam = [0.6, 1.1, 1200., 1200., 2048., 1024.]
    R, t = br.look_at_pose(cols=9, rows=7, size=0.05, **pose)
    board = br.render("eucm", cam, R, t, 9, 7, 0.05, w, h)
    T, _ = br.truth("eucm", cam, R, t, 9, 7, 0.05)
    batch = torch.full((n, h, w), 128, dtype=torch.uint8, device="cuda")
    late = [200, 266, 279]
    for k in late:
        batch[k] = cuda(torch, board)
    det = CornerDetector(9, 7)
    assert det.chunk(w, h) < n
    corners, found = det.detect(batch)
    assert found.nonzero().flatten().tolist() == late
    for k in late:
        _check_order_and_accuracy(corners[k].numpy(), T, 1.0)
    det.close()


# ---- 6. calibration from image files ----

def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def _views(n, seed, cols=9, rows=7, size=0.04):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        pose = dict(centre_cam=[rng.uniform(-0.08, 0.08), rng.uniform(-0.06, 0.06), rng.uniform(0.38, 0.6)],
                    yaw=rng.uniform(-0.6, 0.6), pitch=rng.uniform(-0.5, 0.5), roll=rng.uniform(-0.6, 0.6))
        R, t = br.look_at_pose(cols=cols, rows=rows, size=size, **pose)
        T, ok = br.truth("eucm", EUCM, R, t, cols, rows, size)
        if ok and T.min() > 20 and T[:, 0].max() < W - 20 and T[:, 1].max() < H - 20:
            out.append((R, t))
    return out


def _mono_json(tmp_path, names, flags=("improve_detection",)):
    root = {"transformations": [{"name": "xiCamBoard", "global": False, "constant": False, "prior": False}],
            "cameras": [{"name": "cam", "type": "eucm", "constant": False, "value": [0.55, 1.0, 280., 280., 390., 310.]}],
            "data": [{"type": "images", "camera": "cam", "init": "xiCamBoard", "parameters": list(flags),
                      "transform_chain": [{"name": "xiCamBoard", "direct": True}],
                      "object": {"type": "checkboard", "cols": 9, "rows": 7, "size": 0.04},
                      "images": {"prefix": "img/", "names": names}}]}
    path = tmp_path / "calib_images.json"
    json.dump(root, open(path, "w"), indent=1)
    return str(path)


def test_mono_calibration_from_pgm_files(torch, tmp_path):
    from visgeom_amd import _build
    from visgeom_amd.calibration import GenericCameraCalibration

    os.makedirs(tmp_path / "img")
    names = []
    for i, (R, t) in enumerate(_views(40, 11)):
        _write_pgm(tmp_path / "img" / ("v%02d.pgm" % i), br.render("eucm", EUCM, R, t, 9, 7, 0.04, W, H))
        names.append("v%02d.pgm" % i)
    names.insert(5, "missing.pgm")
    path = _mono_json(tmp_path, names)
    c = GenericCameraCalibration()
    c.addResiduals(path)
    log = c.log()
    assert str(tmp_path / "img" / "missing.pgm") + " : ERROR, file not found" in log
    assert "DETECTION RATE : 40 of 41 detected" in log
    c.compute(max_num_iterations=200)
    got = np.asarray(c.intrinsics("cam"))
    print("intrinsics", got.tolist(), "vs", EUCM)
    assert np.max(np.abs(got[2:] - EUCM[2:])) < 1.0 and np.max(np.abs(got[:2] - EUCM[:2])) < 0.01
    c.close()
    r = subprocess.run([_build.CLI, path], capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr
    assert "DETECTION RATE : 40 of 41 detected" in r.stdout
    line = [l for l in r.stdout.splitlines() if l.startswith("cam : ")][0]
    vals = np.array([float(v) for v in line.split(":")[1].split()])
    assert np.max(np.abs(vals[2:] - EUCM[2:])) < 1.0 and np.max(np.abs(vals[:2] - EUCM[:2])) < 0.01


def test_stereo_images_skip_frames_not_found_in_the_first_camera(torch, tmp_path):
    from visgeom_amd.calibration import GenericCameraCalibration

    os.makedirs(tmp_path / "img")
    views = _views(12, 21)
    xi12_R, xi12_t = br.rodrigues([0., 0.05, 0.]), np.array([-0.05, 0., 0.])
    miss = 4
    n1, n2 = [], []
    for i, (R, t) in enumerate(views):
        im1 = br.render("eucm", EUCM, R, t, 9, 7, 0.04, W, H)
        if i == miss:
            im1 = np.full((H, W), 128, np.uint8)   # no board in camera 1
        R2, t2 = xi12_R.T @ R, xi12_R.T @ (t - xi12_t)
        im2 = br.render("eucm", EUCM, R2, t2, 9, 7, 0.04, W, H)
        _write_pgm(tmp_path / "img" / ("a%02d.pgm" % i), im1)
        _write_pgm(tmp_path / "img" / ("b%02d.pgm" % i), im2)
        n1.append("a%02d.pgm" % i)
        n2.append("b%02d.pgm" % i)
    obj = {"type": "checkboard", "cols": 9, "rows": 7, "size": 0.04}

    def entry(cam, init, chain, names):
        return {"type": "images", "camera": cam, "init": init, "parameters": [], "object": obj,
                "transform_chain": [{"name": nm, "direct": dr} for nm, dr in chain], "images": {"prefix": "img/", "names": names}}

    root = {"transformations": [{"name": "xiCamBoard", "global": False, "constant": False, "prior": False},
                                {"name": "xiCam12", "global": True, "constant": False, "prior": True,
                                 "value": [-0.045, 0.003, 0.002, 0.002, 0.045, -0.001]}],
            "cameras": [{"name": "cam1", "type": "eucm", "constant": False, "value": EUCM},
                        {"name": "cam2", "type": "eucm", "constant": False, "value": EUCM}],
            "data": [entry("cam1", "xiCamBoard", [("xiCamBoard", True)], n1),
                     entry("cam2", "none", [("xiCam12", False), ("xiCamBoard", True)], n2)]}
    path = tmp_path / "stereo.json"
    json.dump(root, open(path, "w"))
    c = GenericCameraCalibration()
    c.addResiduals(str(path))
    log = c.log()
    a, b = str(tmp_path / "img" / ("a%02d.pgm" % miss)), str(tmp_path / "img" / ("b%02d.pgm" % miss))
    assert a + " : ERROR, pattern not found" in log
    assert b + " : ERROR, the pattern has not been found on the corresponding image" in log
    assert "DETECTION RATE : 11 of 12 detected" in log
    c.compute(max_num_iterations=200)
    c.close()
