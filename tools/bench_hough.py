#!/usr/bin/env python3
"""One-GPU measurement of fisheye line detection (include/visgeom_amd.h section 19; visgeom_amd/csrc/vg_hough.hpp): time per call
of vote and detect from HIP events for 1 and 8 images at 1280 x 800 with a 512 x 512 accumulator, the votes per second, and the
call time next to the algorithmic bytes (1 B per pixel read, 4 B per bin cleared and 4 B per bin read).  tools only -- bench.py
stays the driver's contract.

Two images:
  scene     a rendered view of tests/render_scene.py's world at 1280 x 800: noise textures, many short edges, votes spread out
  one_edge  a single straight edge through the centre: every vote in a few dozen bins, the worst same-address contention.  Its
            normal lies on the accumulator camera's horizon and both peaks are dropped by the reference's ABC[2] < 0 rule, so
            lines_found is 0 (profiles/r22_hough.md); the votes, the blur and the maxima test are timed all the same

usage: python tools/bench_hough.py [reps]     (one JSON line per case)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import hough_scene, render_scene  # noqa: E402
from visgeom_amd import hough, render  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
W, H = 1280, 800
CAM = [0.57, 1.1, 480., 480., 640., 400.]
ACC = [0.5, 1., 120., 120., 256., 256.]   # 512 x 512 bins


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


def images():
    r = render.Renderer(CAM, W, H, render_scene.textures()[0], render_scene.planes())
    scene = r.render(render_scene.VIEWS[1]).clone()
    r.close()
    edge = torch.from_numpy(hough_scene.image(W, H, CAM, ((0., 1., 0.),), (200.,), 0.005)).cuda()
    return {"scene": scene, "one_edge": edge}


def main():
    for name, img in images().items():
        for n in (1, 8):
            batch = img[None].repeat(n, 1, 1).contiguous()
            h = hough.Hough(CAM, ACC, W, H)
            bins = h.acc_w * h.acc_h
            t_vote = timed(lambda: h.vote(batch), h._stream)
            acc = h.vote(batch)
            counts = h.counts.sum(axis=0)
            t_detect = timed(lambda: h.detect(batch, 256), h._stream)
            found = [c for _, _, c in h.detect(batch, 256)]
            votes = int(counts[2] + counts[3])
            nbytes = n * (W * H + 8 * bins)
            rec = {"workload": "hough", "image": name, "width": W, "height": H, "acc": [h.acc_w, h.acc_h], "items": n,
                   "vote_ms": t_vote[0] * 1e3, "vote_ms_min_max": [t_vote[1] * 1e3, t_vote[2] * 1e3],
                   "detect_ms": t_detect[0] * 1e3, "detect_ms_min_max": [t_detect[1] * 1e3, t_detect[2] * 1e3],
                   "counts": [int(v) for v in counts], "votes": votes, "bins_hit": int((acc[0] > 0).sum()), "fullest_bin": int(acc[0].max()),
                   "votes_per_s": votes / t_vote[0], "algorithmic_bytes": nbytes, "vote_GB_per_s": nbytes / t_vote[0] / 1e9,
                   "lines_found": found[0], "library": os.environ.get("VISGEOM_AMD_LIBRARY", "default"), "reps": REPS}
            h.close()
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
