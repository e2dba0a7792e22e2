#!/usr/bin/env python3
"""One-GPU measurement of motion stereo (include/visgeom_amd.h section 10; visgeom_amd/csrc/vg_motion.hpp): call time from HIP
events, algorithmic bytes from the shapes and the fraction of the 8 TB/s HBM peak they amount to, next to the project's own
vg_stereo_compute on the same images in the same run.  tools only -- bench.py stays the driver's contract.

Case: the reference's example geometry (ex_epipolar_stereo.json: 1280 x 800, margins 50, disparity_max 120, descriptor 15:
1181 x 701 depth pixels), n in {1, 8} items, without a prior and with the SGM map of the first pair as the prior (the further
view then lies 1.25 baselines out).  The images are the textured planes of tests/stereo_scene.py through the example's cameras.

Algorithmic bytes per item: the key frame, its mask and the new image read once (3 uMax vMax), 24 per depth pixel written
(depth, sigma, cost), 24 more read with a prior; the per-item geometry (2 x 2001 curves x 48 bytes) goes host -> device.

usage: python tools/bench_motion_stereo.py [reps]     (one JSON line per case)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import stereo_ref, stereo_scene  # noqa: E402
from visgeom_amd import motion_stereo, stereo  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
HBM_PEAK = 8.0e12
EXAMPLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ex_epipolar_stereo.json")


def timed(fn, stream):
    """median seconds of fn() over REPS calls after two warm-ups, HIP events on `stream`"""
    fn()
    fn()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ex = json.load(open(EXAMPLE))
    c1, c2 = list(ex["camera_params_left"]), list(ex["camera_params_right"])
    xi = [float(v) for v in ex["stereo_transformation"]]
    xi2 = [1.25 * v for v in xi[:3]] + xi[3:]
    mp = motion_stereo.params_from_json(ex["stereo_parameters"])
    p = mp.stereo

    def render(cam, pose):
        R = np.array(stereo_ref.rotation_matrix(pose[3:], 1.)).reshape(3, 3)
        return stereo_scene.render(cam, R, np.array(pose[:3]), p.u_max, p.v_max, ss=2)

    img1 = stereo_scene.render(c1, np.eye(3), np.zeros(3), p.u_max, p.v_max, ss=2)
    img2, img3 = render(c2, xi), render(c2, xi2)
    for n in (1, 8):
        a, b, c = (torch.from_numpy(np.stack([np.roll(im, k, axis=1) for k in range(n)])).cuda() for im in (img1, img2, img3))
        s = stereo.Stereo(c1, c2, xi, stereo.params_from_json(ex["stereo_parameters"]))
        t_sgm = timed(lambda: s.compute(a, b), s._stream)
        sgm = s.compute(a, b)[:3]
        s.close()
        h = motion_stereo.MotionStereo(c1, c2, mp)
        t_base = timed(lambda: h.set_base(a), h._stream)
        P, img = h.x_max * h.y_max, p.u_max * p.v_max
        for prior, pose, view in ((None, [xi] * n, b), (sgm, [xi2] * n, c)):
            out = [torch.empty_like(sgm[0]) for _ in range(3)]
            t = timed(lambda: h.compute(pose, view, prior, out=out), h._stream)
            by = n * (3 * img + P * (24 if prior is None else 48))
            cnt = h.counts.sum(axis=0)
            rec = {"workload": "motion_stereo", "u_max": p.u_max, "v_max": p.v_max, "x_max": h.x_max, "y_max": h.y_max,
                   "disp_max": p.disp_max, "desc_length": p.desc_length, "items": n, "prior": prior is not None,
                   "compute_ms": t[0] * 1e3, "compute_ms_min_max": [t[1] * 1e3, t[2] * 1e3], "ms_per_item": t[0] * 1e3 / n,
                   "depth_pixels_per_s": n * P / t[0], "algorithmic_bytes": by, "GB_per_s": by / t[0] / 1e9,
                   "frac_hbm_peak": by / t[0] / HBM_PEAK, "counts": [int(v) for v in cnt], "updated_fraction": float(cnt[5]) / (n * P),
                   "set_base_ms": t_base[0] * 1e3, "set_base_frac_hbm_peak": n * 3 * img / t_base[0] / HBM_PEAK,
                   "sgm_compute_ms_same_run": t_sgm[0] * 1e3, "ratio_to_sgm": t[0] / t_sgm[0], "reps": REPS}
            print(json.dumps(rec), flush=True)
        h.close()


if __name__ == "__main__":
    main()
