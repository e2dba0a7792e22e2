#!/usr/bin/env python3
"""One-GPU measurement of photometric bundle adjustment (include/visgeom_amd.h section 18; visgeom_amd/csrc/vg_dense_ba.hpp):
time per call of set_base, set_frames, evaluate (sums only), reduce, one iteration (reduce, the host's K x K solve,
back-substitution, evaluate at the candidate) and solve from HIP events, for F = 2 and F = 8 frames, next to
vg_photometric_evaluate (one scale, F poses, sums only) on the same images and depth map in the same run.  tools only --
bench.py stays the driver's contract.

Case: the reference's example geometry (ex_epipolar_stereo.json: 1280 x 800 images, margins 50: 1181 x 701 depth cells).  The
depth and sigma maps are the SGM maps of the first pair; the frames are two further views, cyclically; the start poses their
poses moved by up to 3 mm and 1 mrad.

Algorithmic bytes per (frame, point): evaluate reads 40 (grey, direction, depth) and 16 image samples of 4 bytes, mostly from
cache, and writes 64 (residual, six pose entries, depth entry); reduce reads those 64 again plus 16 per point (a, g_d).
photo_eval_kernel reads 32 per (pose, point) and, without rows, writes nothing but its partial sums.

usage: python tools/bench_dense_ba.py [reps]     (one JSON line per case)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import stereo_ref, stereo_scene  # noqa: E402
from visgeom_amd import dense_ba, motion_stereo, photometric, stereo  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
EXAMPLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ex_epipolar_stereo.json")


def timed(fn, stream, reps=REPS):
    """median seconds of fn() over reps calls after two warm-ups, HIP events on `stream`"""
    fn()
    fn()
    ts = []
    for _ in range(reps):
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
    xi = np.array([float(v) for v in ex["stereo_transformation"]])
    p = motion_stereo.params_from_json(ex["stereo_parameters"]).stereo

    def render(pose):
        R = np.array(stereo_ref.rotation_matrix(list(pose[3:]), 1.)).reshape(3, 3)
        return stereo_scene.render(c1, R, np.array(pose[:3]), p.u_max, p.v_max, ss=2)

    views = [xi, 0.5 * xi]
    img1, others = render(np.zeros(6)), [render(v) for v in views]
    a1 = torch.from_numpy(img1[None]).cuda()
    s = stereo.Stereo(c1, c1, list(xi), stereo.params_from_json(ex["stereo_parameters"]))
    depth, sigma = [t[0].contiguous() for t in s.compute(a1, torch.from_numpy(others[0][None]).cuda())[:2]]
    s.close()
    rnd = np.random.default_rng(1)
    for F in (2, 8):
        frames = torch.from_numpy(np.stack([others[f % 2] for f in range(F)])).cuda()
        starts = np.stack([views[f % 2] for f in range(F)]) + np.concatenate([rnd.uniform(-0.003, 0.003, (F, 3)), rnd.uniform(-0.001, 0.001, (F, 3))], 1)
        h = dense_ba.DenseBA(c1, p, [0.] * 6, p.u_max, p.v_max)
        t_base = timed(lambda: h.set_base(a1[0], depth, sigma), h._stream)
        t_frames = timed(lambda: h.set_frames(frames), h._stream)
        m = h.count
        t_eval = timed(lambda: h.evaluate(starts, rows=False), h._stream)
        mu = 1e-4
        t_reduce = timed(lambda: h.reduce(mu), h._stream)

        def iteration():
            h.evaluate(starts, rows=False)
            S, rhs = h.reduce(mu)
            dp = -np.linalg.solve(S, rhs)
            cand, _ = h.back_substitute(mu, dp)
            h.evaluate(starts + dp.reshape(-1, 6), cand, rows=False)

        t_iter2 = timed(iteration, h._stream)   # two evaluations: the one at the start is subtracted below
        t_solve = timed(lambda: h.solve(starts), h._stream, reps=3)
        poses, _, _, report = h.solve(starts)
        h.close()
        ph = photometric.Photometric(c1, p, [0.] * 6, p.u_max, p.v_max, 1)
        ph.set_base(a1[0], depth)
        ph.set_targets(frames)
        m_photo = int(ph.pack(0)[0].shape[0])
        t_photo = timed(lambda: ph.evaluate(0, starts, list(range(F)), rows=False), ph._stream)
        ph.close()

        def ms(t):
            return {"ms": t[0] * 1e3, "ms_min_max": [t[1] * 1e3, t[2] * 1e3]}

        per_ba, per_photo = t_eval[0] / (F * m), t_photo[0] / (F * m_photo)
        rec = {"workload": "dense_ba", "width": p.u_max, "height": p.v_max, "x_max": int(depth.shape[-1]), "y_max": int(depth.shape[-2]),
               "frames": F, "pack_points": m, "set_base": ms(t_base), "set_frames": ms(t_frames), "evaluate": ms(t_eval), "reduce": ms(t_reduce),
               "one_iteration_ms": (t_iter2[0] - t_eval[0]) * 1e3, "solve": ms(t_solve), "solve_report": report.tolist(),
               "solve_ms_per_iteration": t_solve[0] * 1e3 / max(report[0], 1.),
               "pose_moved_m": float(np.linalg.norm(poses[:, :3] - starts[:, :3], axis=1).max()),
               "photometric_evaluate_same_run": ms(t_photo), "photometric_pack_points": m_photo,
               "evaluate_ns_per_frame_point": per_ba * 1e9, "photometric_ns_per_pose_point": per_photo * 1e9,
               "evaluate_ratio_per_frame_point": per_ba / per_photo,
               "library": os.environ.get("VISGEOM_AMD_LIBRARY", "default"), "reps": REPS}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
