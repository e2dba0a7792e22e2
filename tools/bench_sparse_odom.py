#!/usr/bin/env python3
"""One-GPU measurement of the sparse visual odometry (include/visgeom_amd.h section 13; visgeom_amd/csrc/vg_sparse_odom.hpp):
HIP-event time per call of detect, match, solve (200 problems of 2 points), score (200 hypotheses) and feed, at the example
size 1181 x 701 and at the test size 192 x 144, on the rendered planes of tests/stereo_scene.py.  tools only -- bench.py stays
the driver's contract.

usage: python tools/bench_sparse_odom.py [reps]     (one JSON object)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import photometric_ref as pr  # noqa: E402
from tests import photometric_scene as ps  # noqa: E402
from tests import stereo_scene  # noqa: E402
from visgeom_amd import sparse_odom  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
STEP = [0.15, 0.01, 0.0, 0.0, 0.0, 0.05]


def timed(fn, stream):
    """median / min / max milliseconds of fn() over REPS calls after two warm-ups, HIP events on `stream`"""
    fn()
    fn()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"ms": float(np.median(ts)), "ms_min_max": [float(min(ts)), float(max(ts))]}


def case(w, h, cam):
    imgs = [stereo_scene.render(cam, *ps.camera_pose(xi), w, h, ss=2) for xi in (np.zeros(6), np.asarray(STEP))]
    d = torch.from_numpy(np.stack(imgs)).cuda()
    odo = sparse_odom.SparseOdometry(cam, ps.XI_BASE_CAM, w, h)
    st = odo._stream
    count, kp, desc = odo.detect(d)
    mc, matches, dist = odo.match(count[:1], desc[:1], count[1:], desc[1:])
    m = int(mc[0])
    pairs = matches[0, :m].cpu().numpy()
    k1, k2 = kp[0].cpu().numpy()[pairs[:, 0]].astype(float), kp[1].cpu().numpy()[pairs[:, 1]].astype(float)
    x1, x2 = (torch.from_numpy(np.ascontiguousarray(pr.reconstruct(cam, k[:, 0], k[:, 1])[0])).cuda() for k in (k1, k2))
    p2, size = torch.from_numpy(k2).cuda(), torch.ones(m, dtype=torch.float64, device="cuda")
    odom = np.asarray(STEP) * 1.05
    tab = odo.draw_samples(m)
    idx = torch.from_numpy(tab.ravel().astype(np.int64)).cuda()
    g = [t[idx].contiguous() for t in (x1, x2, p2, size)]
    hyp, _ = odo.solve(np.arange(201) * 2, *g, odom)

    def feed_pair():
        o = sparse_odom.SparseOdometry(cam, ps.XI_BASE_CAM, w, h)
        o.feed(d[0], np.zeros(6), tab % 1)   # placeholder table for the first frame: it only detects
        o.feed(d[1], odom)
        o.close()

    out = {"width": w, "height": h, "keypoints": count.tolist(), "matches": m,
           "detect_2_images": timed(lambda: odo.detect(d), st), "detect_1_image": timed(lambda: odo.detect(d[:1]), st),
           "match": timed(lambda: odo.match(count[:1], desc[:1], count[1:], desc[1:]), st),
           "solve_200x2": timed(lambda: odo.solve(np.arange(201) * 2, *g, odom), st),
           "score_200": timed(lambda: odo.score(hyp, x1, x2, p2, residuals=False), st),
           "ransac": timed(lambda: odo.ransac(x1, x2, p2, size, odom, tab), st),
           "feed_two_frames_with_handle": timed(feed_pair, st)}
    odo.close()
    return out


def main():
    ex = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ex_epipolar_stereo.json")))
    rec = {"workload": "sparse_odom", "reps": REPS, "library": os.environ.get("VISGEOM_AMD_LIBRARY", "default"),
           "example_size": case(1181, 701, list(ex["camera_params_left"])), "test_size": case(192, 144, ps.CAM)}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
