#!/usr/bin/env python3
"""One-GPU measurement of dense stereo (include/visgeom_amd.h section 9; visgeom_amd/csrc/vg_stereo.hpp): per-stage time from
HIP events around the stage entries, algorithmic bytes from the shapes, and the fraction of the 8 TB/s HBM peak they amount to.
tools only -- bench.py stays the driver's contract (the calibration metric).

Cases: the reference's example geometry (ex_epipolar_stereo.json: 1280 x 800, margins 50, disparity_max 120, descriptor 15,
scales {1, 2, 3, 5}: 1181 x 701 depth pixels) and the same rig at 640 x 400 (margins 25: 591 x 351), each with n in {1, 8}
pairs.  The images are the textured planes of tests/stereo_scene.py rendered through the example's cameras.

Stages (each entry synchronises the handle's stream; the events bracket it on that stream):
  cost       vg_stereo_curve_cost                   bytes: D + 3 per depth pixel written (the image reads are not counted)
  aggregate  vg_stereo_aggregate - cost             bytes: rows 14 D (err read twice, sum written, then read and written)
                                                           + columns 14 D + 4 (err read twice, sum read-write, sum read, winner)
  depth      vg_stereo_compute - vg_stereo_aggregate  bytes: 64 per depth pixel (geometry 32, err, step, salient, skip, winner,
                                                           depth / sigma / cost written)
  compute    vg_stereo_compute (the product call), with the least and the greatest of its repetitions: its run-to-run spread
  compute_mh vg_stereo_compute_mh at 2 and 4 hypotheses next to it: the selection rides in the column pass, the depth launch
             grows with the planes                  bytes beyond compute's: 4 more winner planes written (disparity, final
                                                           cost) and (K - 1) x 64 in the depth launch, per depth pixel

usage: python tools/bench_stereo.py [reps]     (one JSON line per case)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import stereo_ref, stereo_scene  # noqa: E402
from visgeom_amd import stereo  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
HBM_PEAK = 8.0e12
MH = (2, 4)   # hypothesis counts of the compute_mh section
EXAMPLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ex_epipolar_stereo.json")


def timed(fn, stream, spread=False):
    """median seconds of fn() over REPS calls after one warm-up, HIP events on `stream`; spread: (median, least, greatest)"""
    fn()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return (float(np.median(ts)), float(min(ts)), float(max(ts))) if spread else float(np.median(ts))


def case(ex, half, n):
    c1, c2 = list(ex["camera_params_left"]), list(ex["camera_params_right"])
    sp = json.loads(json.dumps(ex["stereo_parameters"]))
    if half:
        for c in (c1, c2):
            c[2:] = [v / 2 for v in c[2:]]
        sp.update(uMax=640, vMax=400, u0=25, v0=25)
    xi = ex["stereo_transformation"]
    p = stereo.params_from_json(sp)
    R = np.array(stereo_ref.rotation_matrix(xi[3:], 1.)).reshape(3, 3)
    img1 = stereo_scene.render(c1, np.eye(3), np.zeros(3), p.u_max, p.v_max, ss=2)
    img2 = stereo_scene.render(c2, R, np.array(xi[:3]), p.u_max, p.v_max, ss=2)
    a = torch.from_numpy(np.stack([np.roll(img1, k, axis=1) for k in range(n)])).cuda()
    b = torch.from_numpy(np.stack([np.roll(img2, k, axis=1) for k in range(n)])).cuda()
    s = stereo.Stereo(c1, c2, xi, p)
    st = s._stream
    t_cost = timed(lambda: s.curve_cost(a, b), st)
    t_agg = timed(lambda: s.aggregate(a, b), st)
    t_all, t_lo, t_hi = timed(lambda: s.compute(a, b), st, spread=True)
    t_mh = {k: timed(lambda: s.compute_mh(a, b, k), st) for k in MH}
    dep = s.compute(a, b)[0]
    P, D = s.x_max * s.y_max, p.disp_max
    stages = {"cost": (t_cost, n * P * (D + 3)), "aggregate": (t_agg - t_cost, n * P * (28 * D + 4)),
              "depth": (t_all - t_agg, n * P * 64)}
    rec = {"workload": "stereo", "u_max": p.u_max, "v_max": p.v_max, "x_max": s.x_max, "y_max": s.y_max, "disp_max": D,
           "desc_length": p.desc_length, "scales": list(p.scales)[:p.n_scales], "use_uv_cache": p.use_uv_cache, "pairs": n,
           "chunk": s.chunk(), "compute_ms": t_all * 1e3, "compute_ms_min": t_lo * 1e3, "compute_ms_max": t_hi * 1e3,
           "compute_mh_ms": {str(k): t * 1e3 for k, t in t_mh.items()}, "compute_mh_over_compute": {str(k): t / t_all for k, t in t_mh.items()},
           "hypo_difference": p.hypo_difference, "depth_pixels_per_s": n * P / t_all,
           "valid_fraction": float((dep > 0).float().mean()), "stages": {}}
    for k, (t, by) in stages.items():
        rec["stages"][k] = {"ms": t * 1e3, "algorithmic_bytes": by, "GB_per_s": by / t / 1e9, "frac_hbm_peak": by / t / HBM_PEAK}
    s.close()
    return rec


def main():
    ex = json.load(open(EXAMPLE))
    for half in (False, True):
        for n in (1, 8):
            print(json.dumps(case(ex, half, n)), flush=True)


if __name__ == "__main__":
    main()
