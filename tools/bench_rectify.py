#!/usr/bin/env python3
"""One-GPU measurement of the rectification kernels (include/visgeom_amd.h section 7; visgeom_amd/csrc/vg_rectify.hpp): kernel
time from HIP events around a warmed, repeated launch, algorithmic bytes from the shapes, and the fraction of the 8 TB/s HBM peak
they amount to.  tools only -- bench.py stays the driver's contract (the calibration metric).

  map    vg_rectify_map at 1920 x 1080 and 3840 x 2160 for EUCM / UCM / Mei: 8 B per pixel written (map_x, map_y)
  remap  vg_remap of N in {1, 8, 32} frames of 3840 x 2160 through a 3840 x 2160 map, u8 C = 1, u8 C = 3, f32 C = 1:
         8 B per pixel of map read + N C (in + out) bytes per pixel (each source and output element once)

regime: "cache" when everything the launch touches fits the 256 MiB Infinity Cache (and stays there between the repeated
launches), "streaming" otherwise.

usage: python tools/bench_rectify.py [reps]     (one JSON line per case)
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from visgeom_amd import capi, rectify  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
HBM_PEAK = 8.0e12
LLC_BYTES = 256 << 20
INTR = {"eucm": [0.6, 1.1, 1300., 1302., 1919.5, 1079.5], "ucm": [0.95, 1500., 1501., 1919.5, 1079.5],
        "mei": [0.9, -0.15, 0.03, -0.005, 0.0008, -0.0011, 1450., 1452., 1919.5, 1079.5]}
XI = [0.01, -0.02, 0.0, 0.02, -0.03, 0.01]


def timed(fn):
    """mean kernel time (s) of fn() over REPS launches after 3 warm-up launches, HIP events on the current stream"""
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


def emit(kind, label, seconds, nbytes, touched, **extra):
    rec = {"case": kind, "label": label, "kernel_us": round(seconds * 1e6, 2), "algorithmic_bytes": int(nbytes),
           "GBps": round(nbytes / seconds / 1e9, 1), "hbm_fraction": round(nbytes / seconds / HBM_PEAK, 3),
           "regime": "cache" if touched <= LLC_BYTES else "streaming", "reps": REPS}
    rec.update(extra)
    print(json.dumps(rec), flush=True)


def main():
    assert torch.cuda.is_available(), "bench_rectify needs a GPU (there is no CPU fallback)"
    dev = torch.device("cuda", 0)
    for w, h in ((1920, 1080), (3840, 2160)):
        pin = [w, h, (w - 1) / 2., (h - 1) / 2., 0.55 * w]
        for model in ("eucm", "ucm", "mei"):
            intr = list(INTR[model])
            intr[-2], intr[-1] = (w - 1) / 2., (h - 1) / 2.
            rectify.rectify_maps(model, intr, pin, XI)   # warm
            mx = torch.empty((h, w), dtype=torch.float32, device=dev)
            my = torch.empty_like(mx)
            L = capi.load()
            m = capi.MODELS[model]
            ia, pa, xa = (np.ascontiguousarray(v, np.float64) for v in (intr, pin, XI))
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def run():
                capi.check(L.vg_rectify_map(0, st, m, ia.ctypes.data_as(_dp), pa.ctypes.data_as(_dp), xa.ctypes.data_as(_dp),
                                            ctypes.c_void_p(mx.data_ptr()), ctypes.c_void_p(my.data_ptr())))

            nbytes = 8 * w * h
            emit("map", "%s %dx%d" % (model, w, h), timed(run), nbytes, nbytes, model=model, width=w, height=h)
            del mx, my
    w, h = 3840, 2160
    map_x, map_y = rectify.rectify_maps("eucm", INTR["eucm"], [w, h, (w - 1) / 2., (h - 1) / 2., 0.55 * w], XI)
    inside = ((map_x > -1) & (map_x < w) & (map_y > -1) & (map_y < h)).float().mean().item()
    for dt, c in (("u8", 1), ("u8", 3), ("f32", 1)):
        esz = 1 if dt == "u8" else 4
        for n in (1, 8, 32):
            shape = (n, h, w, c) if c > 1 else (n, h, w)
            if dt == "u8":
                src = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)
            else:
                src = torch.rand(shape, dtype=torch.float32, device=dev)
            out = rectify.remap(src, map_x, map_y)
            L = capi.load()
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            pt = capi.PIXEL_U8 if dt == "u8" else capi.PIXEL_F32

            def run():
                capi.check(L.vg_remap(0, st, pt, c, n, w, h, ctypes.c_void_p(src.data_ptr()), w, h,
                                      ctypes.c_void_p(map_x.data_ptr()), ctypes.c_void_p(map_y.data_ptr()), 0.,
                                      ctypes.c_void_p(out.data_ptr())))

            nbytes = 8 * w * h + n * c * 2 * esz * w * h
            t = timed(run)
            emit("remap", "%s C=%d N=%d 3840x2160" % (dt, c, n), t, nbytes, nbytes, dtype=dt, channels=c, n_images=n,
                 us_per_frame=round(t * 1e6 / n, 2), map_inside_fraction=round(inside, 4))
            del src, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
