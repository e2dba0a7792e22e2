#!/usr/bin/env python3
"""One-GPU measurement of depth map propagation (include/visgeom_amd.h section 11; visgeom_amd/csrc/vg_depth.hpp): time per call
of warp, merge and the noise filter from HIP events, their algorithmic bytes from the shapes and the fraction of the 8 TB/s HBM
peak they amount to, next to the motion stereo refine call on the same maps in the same run.  tools only -- bench.py stays the
driver's contract.

Case: the reference's example geometry (ex_epipolar_stereo.json: 1280 x 800, margins 50: 1181 x 701 depth pixels), n in {1, 8}
items.  The map is the SGM map of the first pair; the warp pose is the pair's pose (a sideways key-frame change).

Algorithmic bytes per depth pixel and item: warp 8 (depth read for the z-buffer) + 8 (read again for the winner) + 12 (z-buffer
and winner read by the gather) + 16 (the winner's sigma and cost) + 24 written = 68, the atomics' traffic not counted; merge
32 read + 16 written = 48; filter 16 read + 16 written = 32 out of place, 32 more for the copy in place.

usage: python tools/bench_depth_fusion.py [reps]     (one JSON line per case)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import stereo_ref, stereo_scene  # noqa: E402
from visgeom_amd import depth_fusion, motion_stereo, stereo  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
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
    c1 = list(ex["camera_params_left"])
    xi = [float(v) for v in ex["stereo_transformation"]]
    xi2 = [1.25 * v for v in xi[:3]] + xi[3:]
    mp = motion_stereo.params_from_json(ex["stereo_parameters"])
    p = mp.stereo

    def render(pose):
        R = np.array(stereo_ref.rotation_matrix(pose[3:], 1.)).reshape(3, 3)
        return stereo_scene.render(c1, R, np.array(pose[:3]), p.u_max, p.v_max, ss=2)

    img1, img2, img3 = render([0.] * 6), render(xi), render(xi2)
    for n in (1, 8):
        a, b, c = (torch.from_numpy(np.stack([np.roll(im, k, axis=1) for k in range(n)])).cuda() for im in (img1, img2, img3))
        s = stereo.Stereo(c1, c1, xi, stereo.params_from_json(ex["stereo_parameters"]))
        sgm = s.compute(a, b)[:3]
        s.close()
        m = motion_stereo.MotionStereo(c1, c1, mp)
        m.set_base(a)
        out = [torch.empty_like(sgm[0]) for _ in range(3)]
        t_refine = timed(lambda: m.compute([xi2] * n, c, sgm, out=out), m._stream)
        m.close()
        h = depth_fusion.DepthFusion(c1, mp)
        P = h.x_max * h.y_max
        t_warp = timed(lambda: h.warp([xi] * n, sgm), h._stream)
        warped = h.warp([xi] * n, sgm)
        c_warp = h.counts.sum(axis=0)
        t_filter = timed(lambda: h.filter_noise(sgm, out=out[:2]), h._stream)
        c_filter = h.counts.sum(axis=0)
        buf = [t.clone() for t in sgm[:2]]
        t_filter_in_place = timed(lambda: h.filter_noise(buf, out=buf), h._stream)
        t_merge = timed(lambda: h.merge(warped, out), h._stream)   # repeated merges change map 1, not the work per pixel
        c_merge = h.counts.sum(axis=0)
        h.close()

        def rate(t, per_pixel):
            return {"ms": t[0] * 1e3, "ms_min_max": [t[1] * 1e3, t[2] * 1e3], "algorithmic_bytes": n * P * per_pixel,
                    "GB_per_s": n * P * per_pixel / t[0] / 1e9, "frac_hbm_peak": n * P * per_pixel / t[0] / HBM_PEAK}

        three = t_warp[0] + t_merge[0] + t_filter[0]
        rec = {"workload": "depth_fusion", "x_max": h.x_max, "y_max": h.y_max, "items": n, "warp": rate(t_warp, 68),
               "merge": rate(t_merge, 48), "filter_noise": rate(t_filter, 32), "filter_noise_in_place": rate(t_filter_in_place, 64),
               "warp_counts": [int(v) for v in c_warp], "merge_counts": [int(v) for v in c_merge],
               "filter_counts": [int(v) for v in c_filter], "motion_stereo_refine_ms_same_run": t_refine[0] * 1e3,
               "three_ops_ms": three * 1e3, "ratio_to_refine": three / t_refine[0], "library": os.environ.get("VISGEOM_AMD_LIBRARY", "default"),
               "reps": REPS}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
