"""Line detection on the GPU against the numpy restatement (tests/hough_ref.py) on the six cases of tests/hough_scene.py.

What may differ: nothing.  The votes are integer adds, which commute; the chain from a pixel to its bin, the blur, the maxima
and the lines are +, -, *, /, sqrt and round in one order on both sides (FP64, the blur float32, no contraction), and device
sqrt and division are correctly rounded under the build's flags.  So the accumulator, the six counters, the blurred
accumulator and every field of every line are compared for equal bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hough_dump, hough_ref, hough_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(hough_scene.CASES)
# One handle is one image size, camera and accumulator camera, and of the six cases only five_lines and one_line share all three
# (small_acc has the size and camera but another accumulator camera): "all cases that share a size" are these two, each twice.
SHARED = ("five_lines", "one_line", "one_line", "five_lines")


@pytest.fixture(scope="module")
def gpu():
    """every case through vote and detect, once"""
    return {name: hough_dump.run(name) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_accumulator_and_counters(gpu, name):
    ref, got = hough_scene.reference(name), gpu[name]
    print(name, dict(zip(hough_ref.COUNTS, got["counts"].tolist())))
    assert got["acc"].dtype == np.int32 and got["acc"].shape == ref["acc"].shape
    assert np.array_equal(got["acc"], ref["acc"]), "%d bins differ" % int((got["acc"] != ref["acc"]).sum())
    assert got["counts"].tolist() == ref["counts"].tolist()


@pytest.mark.parametrize("name", NAMES)
def test_blur(gpu, name):
    ref, got = hough_scene.reference(name), gpu[name]
    assert got["blur"].dtype == np.float32
    assert got["blur"].tobytes() == ref["blur"].tobytes(), "%d bins differ" % int((got["blur"] != ref["blur"]).sum())


@pytest.mark.parametrize("name", NAMES)
def test_detect(gpu, name):
    ref, got = hough_scene.reference(name), gpu[name]
    assert int(got["count"][0]) == len(ref["lines"]) <= hough_dump.MAX_LINES
    assert got["lines"].shape == ref["lines"].shape
    for field, sl in (("centroid", slice(0, 2)), ("value", slice(2, 3)), ("normal", slice(3, 6)), ("poly6", slice(6, 12))):
        assert got["lines"][:, sl].tobytes() == ref["lines"][:, sl].tobytes(), (field, got["lines"][:, sl], ref["lines"][:, sl])
    assert np.array_equal(got["lines"][:, 12:], ref["lines"][:, 12:], equal_nan=True)
    assert got["status"].tolist() == ref["status"].tolist()


def test_max_lines_below_the_count_returns_the_first_ones(gpu):
    import torch

    from visgeom_amd import hough

    img, cam, acc_cam, prm = hough_scene.case("five_lines")
    full = gpu["five_lines"]
    assert int(full["count"][0]) == 4
    h = hough.Hough(cam, acc_cam, img.shape[1], img.shape[0], hough.make_params(**prm))
    dev = torch.from_numpy(np.array(img)).cuda()
    for m in (0, 1, 3):
        lines, status, count = h.detect(dev, m)
        assert count == 4 and lines.shape == (m, 16) and status.shape == (m,)
        assert lines.tobytes() == full["lines"][:m].tobytes() and status.tolist() == full["status"][:m].tolist()
    h.close()


def test_batch_equals_single_calls_and_repeats(gpu):
    import torch

    from visgeom_amd import hough

    img, cam, acc_cam, prm = hough_scene.case(SHARED[0])
    for name in SHARED:
        c = hough_scene.case(name)
        assert c[0].shape == img.shape and np.array_equal(c[1], cam) and np.array_equal(c[2], acc_cam) and c[3] == prm
    h = hough.Hough(cam, acc_cam, img.shape[1], img.shape[0], hough.make_params(**prm))
    batch = torch.from_numpy(np.stack([hough_scene.case(name)[0] for name in SHARED])).cuda()
    runs = []
    for _ in range(2):
        acc = h.vote(batch).cpu().numpy()
        counts = h.counts.copy()
        res, blur = h.detect(batch, hough_dump.MAX_LINES, blur=True)
        runs.append((acc, counts, blur.cpu().numpy(), res))
    h.close()
    for k, name in enumerate(SHARED):   # no leakage between the items, scratch cleared between the calls
        for acc, counts, blur, res in runs:
            single = gpu[name]
            assert np.array_equal(acc[k], single["acc"]) and counts[k].tolist() == single["counts"].tolist(), (k, name)
            assert blur[k].tobytes() == single["blur"].tobytes(), (k, name)
            lines, status, count = res[k]
            assert count == int(single["count"][0]) and status.tolist() == single["status"].tolist()
            assert lines.tobytes() == single["lines"].tobytes(), (k, name)


def test_a_batch_longer_than_one_chunk():
    """A 4096 x 4096 accumulator takes 12 B x 2^24 bins of scratch an image, so 1 GiB holds five: a batch of six is worked through
    as chunks of five and one.  Item 5, the second chunk, differs from item 0; every item equals its single call (lines, status,
    count and, compared on the device, the blurred accumulator)."""
    import torch

    from visgeom_amd import hough

    order = ("five_lines", "one_line", "one_line", "five_lines", "five_lines", "one_line")
    img, cam, _, prm = hough_scene.case("five_lines")
    big = np.array([0.5, 1., 30., 30., 2048., 2048.])
    h = hough.Hough(cam, big, img.shape[1], img.shape[0], hough.make_params(**prm))
    assert (h.acc_w, h.acc_h) == (4096, 4096)
    dev = {name: torch.from_numpy(np.array(hough_scene.case(name)[0])).cuda() for name in set(order)}
    single = {name: h.detect(d, hough_dump.MAX_LINES, blur=True) for name, d in dev.items()}
    for (lines, status, count), _ in single.values():   # the single call is what the other tests hold to the restatement
        assert 0 < count <= hough_dump.MAX_LINES
    assert single["five_lines"][0][0].tobytes() != single["one_line"][0][0].tobytes()
    res, blur = h.detect(torch.stack([dev[name] for name in order]), hough_dump.MAX_LINES, blur=True)
    for k, name in enumerate(order):
        (lines, status, count), b = single[name]
        assert res[k][2] == count and res[k][1].tolist() == status.tolist() and res[k][0].tobytes() == lines.tobytes(), (k, name)
        assert torch.equal(blur[k], b), (k, name)
    h.close()


def test_the_gpu_finds_the_drawn_lines(gpu):
    hough_scene.check_truth("five_lines", gpu["five_lines"]["lines"])


def read_pgm(path):
    data = open(path, "rb").read()
    magic, w, h, maxval = data.split(None, 4)[:4]
    assert magic == b"P5" and maxval == b"255"
    w, h = int(w), int(h)
    return np.frombuffer(data[len(data) - w * h:], dtype=np.uint8).reshape(h, w)


def test_the_program(gpu, tmp_path):
    import json

    from visgeom_amd import _build, hough

    img, cam, acc_cam, _ = hough_scene.case("five_lines")
    h, w = img.shape
    with open(str(tmp_path / "img.pgm"), "wb") as fh:
        fh.write(b"P5\n%d %d\n255\n" % (w, h) + img.tobytes())
    path = str(tmp_path / "lines.json")
    with open(path, "w") as fh:
        json.dump({"width": w, "height": h, "camera_params": cam.tolist(), "acc_params": acc_cam.tolist(), "names": ["img.pgm"]}, fh)
    r = subprocess.run([_build.HOUGH_CLI, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = gpu["five_lines"]
    rows = [ln.split() for ln in open(str(tmp_path / "lines_0.txt")).read().splitlines()]
    assert len(rows) == len(want["lines"]) and all(len(row) == 17 for row in rows)
    lines = np.array([[float(x) for x in row[:16]] for row in rows])
    assert lines.tobytes() == want["lines"].tobytes()   # %.17g round-trips a double
    assert [int(row[16]) for row in rows] == want["status"].tolist()
    traced = np.zeros(img.shape, dtype=bool)
    for L, st in zip(want["lines"], want["status"]):
        assert st == 0
        for u, v in hough.trace(L[6:12], L[12:16]).tolist():
            if 0 <= u < w and 0 <= v < h:
                traced[v, u] = True
    res = read_pgm(str(tmp_path / "res_0.pgm"))
    assert traced.sum() > 400 and (img[traced] != 255).all()   # so that "differs" and "traced" are the same set
    assert np.array_equal(res != img, traced) and (res[traced] == 255).all()
    acc8 = read_pgm(str(tmp_path / "acc_0.pgm"))
    expect = np.clip(np.rint(want["blur"] * np.float32(255) / np.float32(100)), 0, 255).astype(np.uint8)
    assert np.array_equal(acc8, expect)
    # a malformed input is one line on stderr and a non-zero exit, before the GPU is touched
    with open(path, "w") as fh:
        json.dump({"width": w + 1, "height": h, "camera_params": cam.tolist(), "acc_params": acc_cam.tolist(), "names": ["img.pgm"]}, fh)
    r = subprocess.run([_build.HOUGH_CLI, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stderr.startswith("hough: ") and len(r.stderr.strip().splitlines()) == 1


def test_production_library_gives_the_same_bytes(gpu, tmp_path):
    from visgeom_amd import _build

    assert os.path.exists(_build.PRODUCTION_LIB), "python -m visgeom_amd._build --production (or __graft_entry__.build())"
    path = str(tmp_path / "production.npz")
    env = dict(os.environ, VISGEOM_AMD_LIBRARY="production")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "hough_dump.py"), path], env=env, cwd=ROOT, timeout=300)
    got = np.load(path)
    assert int(got["has_hooks"][0]) == 0 and "production" in str(got["library"][0])
    for name in NAMES:
        for k, v in gpu[name].items():
            assert got[name + "." + k].tobytes() == np.asarray(v).tobytes(), (name, k)
