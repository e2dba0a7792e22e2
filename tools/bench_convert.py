#!/usr/bin/env python3
"""One-GPU measurement of the conversion between camera models (include/visgeom_amd.h section 20; visgeom_amd/csrc/vg_convert.hpp):
kernel time from HIP events around a warmed, repeated launch.  tools only -- bench.py stays the driver's contract (the calibration
metric).

  convert_maps  vg_convert_map at 3840 x 2160 for kb -> eucm, ds -> eucm, eucm -> kb and mei -> eucm (source -> destination: the
                destination's pixels are unprojected, the source projects), next to vg_rectify_map of the same size and the same
                source model IN THE SAME RUN: the nearest kernel the library had (pinhole ray -> source projection).  8 B per pixel
                written by both
  unproject     vg_unproject of 1e6 pixels per model: 16 B read + 25 B written per pixel
  fit           vg_convert_fit kb -> eucm on the default 64 x 40 grid with the default options: wall time of the synchronous call,
                its iterations, and the time per evaluation (iterations + 2 evaluations)

usage: python tools/bench_convert.py [reps]     (ONE JSON line)
"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from visgeom_amd import capi, convert, synthetic  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
W, H = 3840, 2160
PAIRS = [("kb", "eucm"), ("ds", "eucm"), ("eucm", "kb"), ("mei", "eucm")]   # source -> destination


def camera(model):
    """synthetic.GT's camera of the 1280 x 800 image at 3840 x 2160"""
    p = np.array(synthetic.GT[model], float)
    p[-4], p[-2] = p[-4] * W / 1280, p[-2] * W / 1280
    p[-3], p[-1] = p[-3] * H / 800, p[-1] * H / 800
    return p


def timed(fn):
    """mean time (s) of fn() over REPS launches after 3 warm-up launches, HIP events on the current stream"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / REPS


def main():
    assert torch.cuda.is_available(), "bench_convert needs a GPU (there is no CPU fallback)"
    out = {"metric": "convert", "reps": REPS, "width": W, "height": H, "maps": {}, "unproject": {}}
    pinhole = [W, H, (W - 1) / 2., (H - 1) / 2., 0.55 * W]
    xi = [0., 0., 0., 0.02, -0.03, 0.01]
    # the entries are called directly on preallocated outputs: at 30 us a launch the wrappers' allocations would be measured too
    L = capi.load()
    dev = torch.device("cuda", 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    mx = torch.empty((H, W), dtype=torch.float32, device=dev)
    my = torch.empty_like(mx)
    mxp, myp = ctypes.c_void_p(mx.data_ptr()), ctypes.c_void_p(my.data_ptr())
    pa, xa = np.ascontiguousarray(pinhole, np.float64), np.ascontiguousarray(xi, np.float64)
    ra = np.ascontiguousarray(xi[3:], np.float64)
    for src, dst in PAIRS:
        ps, pd = np.ascontiguousarray(camera(src)), np.ascontiguousarray(convert.fit(src, camera(src), (W, H), dst)[0])
        ms, md = capi.MODELS[src], capi.MODELS[dst]
        t_map = timed(lambda: capi.check(L.vg_convert_map(0, st, md, pd.ctypes.data_as(_dp), ms, ps.ctypes.data_as(_dp), ra.ctypes.data_as(_dp),
                                                          W, H, mxp, myp)))
        t_rect = timed(lambda: capi.check(L.vg_rectify_map(0, st, ms, ps.ctypes.data_as(_dp), pa.ctypes.data_as(_dp), xa.ctypes.data_as(_dp),
                                                           mxp, myp)))
        capi.check(L.vg_convert_map(0, st, md, pd.ctypes.data_as(_dp), ms, ps.ctypes.data_as(_dp), ra.ctypes.data_as(_dp), W, H, mxp, myp))
        out["maps"]["%s->%s" % (src, dst)] = {"convert_map_us": round(t_map * 1e6, 2), "rectify_map_us_same_source": round(t_rect * 1e6, 2),
                                             "GBps": round(8 * W * H / t_map / 1e9, 1), "valid_fraction": round((mx != -1).float().mean().item(), 4)}
    n = 1000000
    rng = np.random.default_rng(1)
    uv = torch.from_numpy(np.column_stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)])).cuda()
    rays = torch.empty((n, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((n,), dtype=torch.uint8, device=dev)
    for model in ("eucm", "ucm", "mei", "kb", "ds"):
        p, m = np.ascontiguousarray(camera(model)), capi.MODELS[model]
        t = timed(lambda: capi.check(L.vg_unproject(0, st, m, p.ctypes.data_as(_dp), n, ctypes.c_void_p(uv.data_ptr()),
                                                    ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(ok.data_ptr()))))
        out["unproject"][model] = {"us": round(t * 1e6, 2), "Gpixels_per_s": round(n / t / 1e9, 2), "GBps": round(41 * n / t / 1e9, 1),
                                   "valid_fraction": round(ok.float().mean().item(), 4)}
    kb = np.array(synthetic.GT["kb"], float)
    convert.fit("kb", kb, (1280, 800), "eucm")   # warm
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, s = convert.fit("kb", kb, (1280, 800), "eucm")
        walls.append(time.perf_counter() - t0)
    wall = sorted(walls)[len(walls) // 2]
    out["fit"] = {"pair": "kb->eucm", "grid": [64, 40], "wall_ms_median_of_5": round(wall * 1e3, 3), "iterations": s["iterations"],
                  "us_per_evaluation": round(wall * 1e6 / (s["iterations"] + 2), 1), "rms_px": round(s["rms"], 4),
                  "max_residual_px": round(s["max_residual"], 4), "termination": s["termination"]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
