"""Runs vote and detect on every case of tests/hough_scene.py with the library this process loads and writes every output to the
.npz file named on the command line (tests/test_gpu_hough.py starts it with VISGEOM_AMD_LIBRARY=production)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import hough_scene  # noqa: E402
from visgeom_amd import capi, hough  # noqa: E402

MAX_LINES = 16


def run(name):
    """dict of one case's outputs: acc, counts, blur, lines, status, count"""
    import torch

    img, cam, acc_cam, prm = hough_scene.case(name)
    h = hough.Hough(cam, acc_cam, img.shape[1], img.shape[0], hough.make_params(**prm))
    dev = torch.from_numpy(np.array(img)).cuda()
    acc = h.vote(dev).cpu().numpy()
    (lines, status, count), blur = h.detect(dev, MAX_LINES, blur=True)
    out = dict(acc=acc, counts=h.counts[0], blur=blur.cpu().numpy(), lines=lines, status=status, count=np.array([count]))
    h.close()
    return out


def main(path):
    out = dict(has_hooks=np.array([int(capi.has_debug_hooks())]), library=np.array([capi.lib_path()]))
    for name in sorted(hough_scene.CASES):
        for k, v in run(name).items():
            out[name + "." + k] = v
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
