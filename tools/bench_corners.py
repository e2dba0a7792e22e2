"""Corner detection throughput on rendered checkerboards (include/visgeom_amd.h section 8).

    python tools/bench_corners.py [--frames 64 512] [--sizes 1280x800 1920x1080] [--improve] [--reps 3] [--out file.jsonl]

Every workload is N frames of one size: 8 distinct renders of a 9 x 7 board through an EUCM camera (8 x 8 samples per pixel),
repeated.  One JSON line per workload: the end-to-end images per second of one detect call, and the call's split from the
detector's own clocks: GPU stages (launch to the hit-count read-back), the device -> host copy and its bytes, the host graph
stage (16 threads) per image, and the refinement per corner.  Kernel times come from a separate `rocprofv3 --kernel-trace
--stats` run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def renders(w, h, k=8):
    from tests import board_render as br

    f = 300. * w / 800.
    cam = [0.6, 1.1, f, f, w / 2., h / 2.]
    rng = np.random.default_rng(w)
    out = []
    while len(out) < k:
        pose = dict(centre_cam=[rng.uniform(-0.06, 0.06), rng.uniform(-0.04, 0.04), rng.uniform(0.4, 0.6)],
                    yaw=rng.uniform(-0.5, 0.5), pitch=rng.uniform(-0.4, 0.4), roll=rng.uniform(-0.6, 0.6))
        R, t = br.look_at_pose(cols=9, rows=7, size=0.04, **pose)
        T, ok = br.truth("eucm", cam, R, t, 9, 7, 0.04)
        if ok and T.min() > 20 and T[:, 0].max() < w - 20 and T[:, 1].max() < h - 20:
            out.append(br.render("eucm", cam, R, t, 9, 7, 0.04, w, h))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--sizes", nargs="+", default=["1280x800", "1920x1080"])
    ap.add_argument("--improve", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    from visgeom_amd.corners import CornerDetector

    lines = []
    for size in a.sizes:
        w, h = (int(x) for x in size.split("x"))
        base = torch.from_numpy(renders(w, h)).cuda()
        for n in a.frames:
            batch = base.repeat((n + 7) // 8, 1, 1)[:n].contiguous()
            det = CornerDetector(9, 7, improve=a.improve)
            det.detect(batch[:min(n, 8)])   # warm-up: scratch allocation and first launches
            s0 = det.stats()
            best = None
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, found = det.detect(batch)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            s1 = det.stats()
            d = {k: (s1[k] - s0[k]) / a.reps for k in s1}
            rec = {"workload": "corners", "width": w, "height": h, "frames": n, "improve": a.improve, "chunk": det.chunk(w, h),
                   "found": int(found.sum()), "best_call_s": best, "images_per_s": n / best,
                   "gpu_stages_ms": 1e3 * d["gpu_s"], "d2h_ms": 1e3 * d["d2h_s"], "d2h_GB": d["d2h_bytes"] / 1e9,
                   "d2h_GB_per_s": d["d2h_bytes"] / d["d2h_s"] / 1e9 if d["d2h_s"] > 0 else None,
                   "graph_ms": 1e3 * d["graph_s"], "graph_ms_per_image": 1e3 * d["graph_s"] / max(1., d["graph_images"]),
                   "refine_ms": 1e3 * d["refine_s"],
                   "refine_us_per_corner": 1e6 * d["refine_s"] / d["refine_corners"] if d["refine_corners"] else None}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            det.close()
            del batch
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
