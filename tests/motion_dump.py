"""Runs motion stereo on the library the process loads and dumps every output (tests/test_gpu_motion_stereo.py compares the
hooks build with the production build).  usage: python tests/motion_dump.py out.npz"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import motion_scene as ms, stereo_scene  # noqa: E402
from visgeom_amd import capi, motion_stereo, stereo  # noqa: E402


def main(path):
    rig = "forward"
    img1, img2, _, xi = stereo_scene.make_scene(rig)
    p = ms.prm_of(rig)
    a, b = (torch.from_numpy(x).cuda() for x in (img1, img2))
    sp = {k: v for k, v in p.items() if k != "gradient_thresh"}
    s = stereo.Stereo(stereo_scene.CAM1, stereo_scene.CAM2, xi, stereo.make_params(**sp))
    sgm = s.compute(a, b)[:3]
    s.close()
    h = motion_stereo.MotionStereo(stereo_scene.CAM1, stereo_scene.CAM2, motion_stereo.make_params(**p))
    h.set_base(a)
    out = {"has_hooks": np.array([int(capi.has_debug_hooks())]), "mask": h.mask().cpu().numpy()}
    for name, t in zip(("depth", "sigma", "cost"), h.compute(xi, b)):
        out[name] = t.cpu().numpy()
    out["counts"] = h.counts.copy()
    pose = ms.poses(rig)[0]
    v = torch.from_numpy(ms.view(pose)).cuda()
    out["record_prior"] = h.select(pose, v, sgm).cpu().numpy()
    for name, t in zip(("depth_prior", "sigma_prior", "cost_prior"), h.compute(pose, v, sgm)):
        out[name] = t.cpu().numpy()
    out["counts_prior"] = h.counts.copy()
    h.close()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
