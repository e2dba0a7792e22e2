"""Renders the test scene's three views in one batch with the library this process loads and writes every output to the .npz
file named on the command line (tests/test_gpu_render.py starts it with VISGEOM_AMD_LIBRARY=production)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import render_scene as sc  # noqa: E402
from visgeom_amd import capi, render  # noqa: E402


def main(path):
    r = render.Renderer(sc.CAM, sc.W, sc.H, sc.textures()[0], sc.planes())
    image, depth, index, u, v = r.render(sc.VIEWS, buffers=True)
    np.savez(path, image=image.cpu().numpy(), depth=depth.cpu().numpy(), index=index.cpu().numpy(), u=u.cpu().numpy(), v=v.cpu().numpy(),
             counts=r.counts, has_hooks=np.array([int(capi.has_debug_hooks())]), library=np.array([capi.lib_path()]))
    r.close()


if __name__ == "__main__":
    main(sys.argv[1])
