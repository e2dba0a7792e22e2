"""Child process of tests/test_gpu_depth_fusion.py: warp, merge and the noise filter on the synthetic maps with whichever
library VISGEOM_AMD_LIBRARY selects, the outputs saved to the .npz named on the command line."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import depth_scene as ds  # noqa: E402
from tests import motion_ref as mr  # noqa: E402
from tests import motion_scene as ms  # noqa: E402
from visgeom_amd import capi, depth_fusion, stereo  # noqa: E402


def main(path):
    prm = mr.params(**ms.prm_of("sideways"))
    a, b = ds.synthetic_maps(prm)
    h = depth_fusion.DepthFusion(ds.CAM, stereo.make_params(**{k: v for k, v in ms.prm_of("sideways").items() if k != "gradient_thresh"}))
    ta, tb = ([torch.from_numpy(x).cuda() for x in m] for m in (a, b))
    out = {"has_hooks": np.array([int(capi.has_debug_hooks())])}
    w = h.warp(ds.WARP_POSES["backward"], ta)
    out.update(warp_depth=w[0].cpu().numpy(), warp_sigma=w[1].cpu().numpy(), warp_cost=w[2].cpu().numpy(), warp_counts=h.counts.copy())
    f = h.filter_noise(ta)
    out.update(filter_depth=f[0].cpu().numpy(), filter_sigma=f[1].cpu().numpy(), filter_counts=h.counts.copy())
    h.merge(ta, tb)
    out.update(merge_depth=ta[0].cpu().numpy(), merge_sigma=ta[1].cpu().numpy(), merge_counts=h.counts.copy())
    h.close()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
