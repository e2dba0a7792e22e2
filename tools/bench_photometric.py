#!/usr/bin/env python3
"""One-GPU measurement of photometric localization (include/visgeom_amd.h section 12; visgeom_amd/csrc/vg_photometric.hpp):
time per call of set_base, set_targets, one evaluate (sums only) at the finest scale and one compute_pose from HIP events,
the same for the mutual-information cost (evaluate_mi with its gradient, compute_pose_mi), next to the motion stereo refine
call on the same maps in the same run.  tools only -- bench.py stays the driver's contract.

Case: the reference's example geometry (ex_epipolar_stereo.json: 1280 x 800 images, margins 50: 1181 x 701 depth pixels), 5
scales, n in {1, 8} poses, each against its own target image.  The depth map is the SGM map of the first pair; the targets
are the second view, the start poses its pose moved by up to 1 cm and 0.2 degrees.

Algorithmic bytes: set_base reads 1 + 8 bytes per pixel (image, depth) and writes 12 per pyramid pixel (level, two gradients)
plus 36 per pack point; set_targets reads 1 and writes 4 per pyramid pixel (1.33 x the image); evaluate reads 32 per pack
point and pose (value, cloud) and 16 target samples of 4 bytes, mostly from cache; evaluate_mi reads the same twice (the
gradient pass samples again) and writes 560 bytes of partial sums per 256 points.

usage: python tools/bench_photometric.py [reps]     (one JSON line per case)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import stereo_ref, stereo_scene  # noqa: E402
from visgeom_amd import motion_stereo, photometric, stereo  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
NUM_SCALES = 5
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
    mp = motion_stereo.params_from_json(ex["stereo_parameters"])
    p = mp.stereo

    def render(pose):
        R = np.array(stereo_ref.rotation_matrix(pose[3:], 1.)).reshape(3, 3)
        return stereo_scene.render(c1, R, np.array(pose[:3]), p.u_max, p.v_max, ss=2)

    img1, img2 = render([0.] * 6), render(xi)
    a1, b1 = torch.from_numpy(img1[None]).cuda(), torch.from_numpy(img2[None]).cuda()
    s = stereo.Stereo(c1, c1, xi, stereo.params_from_json(ex["stereo_parameters"]))
    sgm = s.compute(a1, b1)[:3]
    s.close()
    m = motion_stereo.MotionStereo(c1, c1, mp)
    m.set_base(a1)
    out = [torch.empty_like(sgm[0]) for _ in range(3)]
    t_refine = timed(lambda: m.compute([xi], b1, sgm, out=out), m._stream)
    m.close()
    rnd = np.random.default_rng(1)
    for n in (1, 8):
        h = photometric.Photometric(c1, p, [0.] * 6, p.u_max, p.v_max, NUM_SCALES)
        targets = torch.from_numpy(np.stack([img2] * n)).cuda()
        starts = np.array(xi) + np.concatenate([rnd.uniform(-0.01, 0.01, (n, 3)), rnd.uniform(-0.0035, 0.0035, (n, 3))], 1)
        t_base = timed(lambda: h.set_base(a1[0], sgm[0][0]), h._stream)
        t_targets = timed(lambda: h.set_targets(targets), h._stream)
        points = [int(h.pack(i)[0].shape[0]) for i in range(NUM_SCALES)]
        idx = list(range(n))
        t_eval = timed(lambda: h.evaluate(0, starts, idx, rows=False), h._stream)
        t_pose = timed(lambda: h.compute_pose(starts, idx), h._stream)
        poses, report = h.compute_pose(starts, idx)
        t_eval_mi = timed(lambda: h.evaluate_mi(0, starts, idx, values=False), h._stream)
        t_pose_mi = timed(lambda: h.compute_pose_mi(starts, idx), h._stream)
        poses_mi, report_mi = h.compute_pose_mi(starts, idx)
        h.close()

        def ms(t):
            return {"ms": t[0] * 1e3, "ms_min_max": [t[1] * 1e3, t[2] * 1e3]}

        rec = {"workload": "photometric", "width": p.u_max, "height": p.v_max, "x_max": int(sgm[0].shape[-1]), "y_max": int(sgm[0].shape[-2]),
               "scales": NUM_SCALES, "poses": n, "pack_points": points, "set_base": ms(t_base), "set_targets": ms(t_targets),
               "evaluate_finest": ms(t_eval), "compute_pose": ms(t_pose),
               "evaluate_mi_finest": ms(t_eval_mi), "compute_pose_mi": ms(t_pose_mi),
               "mi_iterations_per_scale": report_mi[:, :, 0].mean(axis=0).tolist(), "mi_final_cost_finest": report_mi[:, 0, 2].tolist(),
               "mi_pose_moved_m": float(np.linalg.norm(poses_mi[:, :3] - np.array(xi[:3]), axis=1).max()),
               "iterations_per_scale": report[:, :, 0].mean(axis=0).tolist(), "final_cost_finest": report[:, 0, 2].tolist(),
               "pose_moved_m": float(np.linalg.norm(poses[:, :3] - np.array(xi[:3]), axis=1).max()),
               "motion_stereo_refine_ms_same_run": t_refine[0] * 1e3, "compute_pose_ratio_to_refine": t_pose[0] / t_refine[0],
               "library": os.environ.get("VISGEOM_AMD_LIBRARY", "default"), "reps": REPS}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
