#!/usr/bin/env python3
"""One-GPU measurement of depth map point clouds, the plane prior and the accuracy score (include/visgeom_amd.h section 11,
continued; visgeom_amd/csrc/vg_depth.hpp): time per call of DepthFusion.reconstruct for a full and a half-empty 1181 x 701 map, 1
and 8 items, flags 0 and MINMAX | SIGMA_VALUE, and for 100 000 query points; of compare and of generate_plane; and the figures
the stereo_accuracy loop gives per step on tests/stereo_accuracy_scene.py.  Times are HIP events around whole calls
(benchlib.timed): a reconstruct call is two synchronous legs (count, place) and the allocation of its outputs.  tools only --
bench.py stays the driver's contract.

usage: python tools/bench_cloud.py [reps]     (one JSON line per case)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import cloud_dump  # noqa: E402
from visgeom_amd import benchlib, capi, depth_fusion, stereo  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
X, Y = 1181, 701
CAM = [0.57, 1.1, 480., 480., 590., 350.]
PLANE = ([0.1, -0.05, 1.5, 0.2, -0.1, 0.05], [[-2., -1.5, 0.], [2., -1.5, 0.], [2., 1.5, 0.], [-2., 1.5, 0.]])


def emit(**rec):
    rec.update(library=os.environ.get("VISGEOM_AMD_LIBRARY", "default"), reps=REPS)
    print(json.dumps(rec), flush=True)


def main():
    rng = np.random.default_rng(23)
    f = depth_fusion.DepthFusion(CAM, stereo.make_params(scale=1, u0=0, v0=0, u_max=X, v_max=Y, x_max=X, y_max=Y))
    full = torch.from_numpy(rng.uniform(0.5, 20., (8, 1, Y, X))).cuda()
    half = torch.where(torch.from_numpy(rng.random((8, 1, Y, X)) < 0.5).cuda(), full, torch.zeros_like(full))
    sigma = torch.from_numpy(rng.uniform(0.01, 0.5, (8, 1, Y, X))).cuda()
    for name, depth in (("full", full), ("half_empty", half)):
        for n in (1, 8):
            for flags in (0, capi.RECON_MINMAX | capi.RECON_SIGMA_VALUE):
                maps = (depth[:n], sigma[:n])
                t = benchlib.timed(lambda: f.reconstruct(maps, flags), REPS)
                c = f.reconstruct(maps, flags)
                m = int(c.counts.sum())
                per = 4 + 4 + 16 + 4 + 1 + (48 + 8 if flags else 24)   # indices, hyp, points, item, valid, cloud (+ sigma)
                nbytes = 2 * n * X * Y * 8 + m * ((8 if flags else 0) + per)   # plane 0 read by both passes
                emit(workload="reconstruct", map=name, width=X, height=Y, items=n, flags=flags, entries=m, call_us=t * 1e6,
                     algorithmic_bytes=nbytes, GB_per_s=nbytes / t / 1e9)
    pts = torch.from_numpy(np.stack([rng.uniform(-50., X + 50., 100000), rng.uniform(-50., Y + 50., 100000)], 1)).cuda()
    flags = capi.RECON_QUERY_POINTS | capi.RECON_INDEX_MAPPING
    t = benchlib.timed(lambda: f.reconstruct((half[:1], sigma[:1]), flags, query_points=pts), REPS)
    c = f.reconstruct((half[:1], sigma[:1]), flags, query_points=pts)
    emit(workload="reconstruct", map="half_empty", items=1, flags=flags, queries=100000, entries=int(c.counts.sum()), call_us=t * 1e6)
    truth = torch.from_numpy(rng.uniform(0.5, 20., (8, Y, X)).astype(np.float32)).cuda()
    for n in (1, 8):
        maps = (half[:n, 0].contiguous(), sigma[:n, 0].contiguous())
        t = benchlib.timed(lambda: f.compare(maps, truth[:n]), REPS)
        nbytes = n * X * Y * (8 + 8 + 4 + 1)
        emit(workload="compare", width=X, height=Y, items=n, call_us=t * 1e6, algorithmic_bytes=nbytes, GB_per_s=nbytes / t / 1e9,
             counts=f.compare(maps, truth[:n]).counts.tolist())
    t = benchlib.timed(lambda: f.generate_plane(*PLANE), REPS)
    emit(workload="generate_plane", width=X, height=Y, call_us=t * 1e6, pixels_inside=int((f.generate_plane(*PLANE)[0] > 0).sum()))
    f.close()
    steps, _, cloud = cloud_dump.accuracy_loop()
    for i, (_, _, _, acc) in enumerate(steps):
        emit(workload="stereo_accuracy", step=i, method="sgm" if i < 2 else "motion_stereo", baseline_m=0.05 * (i + 1),
             counts=dict(zip(depth_fusion.COMPARE_COUNTS, (int(v) for v in acc.counts))), mean_error_mm=float(acc.mean_error_mm),
             rms_error_mm=float(acc.rms_error_mm), inlier_percent=float(acc.inlier_percent), mean_distance_m=float(acc.mean_distance),
             coverage=float(acc.coverage), cloud_points=len(cloud) if i == len(steps) - 1 else None)


if __name__ == "__main__":
    main()
