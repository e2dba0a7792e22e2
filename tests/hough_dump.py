"""Runs vote and detect on every case of tests/hough_scene.py -- or, with "shapes" as a second argument, of tests/hough_shapes.py --
with the library this process loads and writes every output to the .npz file named on the command line (tests/test_gpu_hough.py
and tests/test_gpu_hough_shapes.py start it with VISGEOM_AMD_LIBRARY=production)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import hough_scene  # noqa: E402
from visgeom_amd import capi, hough  # noqa: E402

MAX_LINES = 16


def run(name, source=hough_scene, max_lines=MAX_LINES):
    """dict of one case's outputs: acc, counts, blur, lines, status, count; source: the module whose case(name) it is"""
    import torch

    img, cam, acc_cam, prm = source.case(name)
    h = hough.Hough(cam, acc_cam, img.shape[1], img.shape[0], hough.make_params(**prm))
    dev = torch.from_numpy(np.array(img)).cuda()
    acc = h.vote(dev).cpu().numpy()
    (lines, status, count), blur = h.detect(dev, max_lines, blur=True)
    out = dict(acc=acc, counts=h.counts[0], blur=blur.cpu().numpy(), lines=lines, status=status, count=np.array([count]))
    h.close()
    return out


def main(path, which="scene"):
    out = dict(has_hooks=np.array([int(capi.has_debug_hooks())]), library=np.array([capi.lib_path()]))
    if which == "shapes":
        from tests import hough_shapes

        cases = [(name, hough_shapes, hough_shapes.MAX_LINES) for name in hough_shapes.NAMES]
    else:
        cases = [(name, hough_scene, MAX_LINES) for name in sorted(hough_scene.CASES)]
    for name, source, max_lines in cases:
        for k, v in run(name, source, max_lines).items():
            out[name + "." + k] = v
    np.savez(path, **out)


if __name__ == "__main__":
    main(*sys.argv[1:3])
