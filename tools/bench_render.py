#!/usr/bin/env python3
"""One-GPU measurement of the scene renderer (include/visgeom_amd.h section 14; visgeom_amd/csrc/vg_render.hpp): time per call of
Renderer.render from HIP events, for 1 and 8 views at the reference's example size (1181 x 701) and at the tests' size (80 x 60),
with the work the call did counted from its own buffers: covered pixels, pixels sampled with the single bicubic tap, and the
bilinear taps of all the others (sum of nu * nv, recomputed here from index / u / v).  tools only -- bench.py stays the driver's
contract.

The world is the tests' (tests/render_scene.py: a slanted floor, a small plane, a panorama) with textures scaled to the image, so
that the footprints have the tests' spread, 1 to 24 taps a side.  The 8 views are the tests' three poses and five between them.

usage: python tools/bench_render.py [reps]     (one JSON line per case)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import render_scene as sc  # noqa: E402
from visgeom_amd import render  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
RADIUS = 2.75


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


def taps(index, u, v):
    """(bilinear taps, single-tap pixels) of a batch, from its buffers: fillImage's footprint and Texture::sample's nu, nv"""
    u, v = u.double(), v.double()

    def length(axis):
        same_lo = torch.zeros_like(index, dtype=torch.bool)
        same_hi = torch.zeros_like(index, dtype=torch.bool)
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        eq = index[tuple(lo)] == index[tuple(hi)]
        same_lo[tuple(hi)] = eq
        same_hi[tuple(lo)] = eq
        du, dv = torch.zeros_like(u), torch.zeros_like(v)
        for arr, d in ((u, du), (v, dv)):
            prev, nxt = arr.clone(), arr.clone()
            prev[tuple(hi)] = torch.where(eq, arr[tuple(lo)], arr[tuple(hi)])
            nxt[tuple(lo)] = torch.where(eq, arr[tuple(hi)], arr[tuple(lo)])
            d.copy_(nxt - prev)
        count = (same_lo.double() + same_hi.double()).clamp(min=1.)
        e = torch.sqrt((du / count) ** 2 + (dv / count) ** 2) * RADIUS
        return torch.floor(e + 0.5).clamp(1., 24.)

    nu, nv = length(2), length(1)
    covered = index >= 0
    single = covered & (nu == 1) & (nv == 1)
    return int((nu * nv)[covered & ~single].sum().item()), int(single.sum().item())


def world(width, height):
    """the tests' world with camera and textures scaled from 80 x 60 to width x height"""
    s = width / float(sc.W)
    t = height / float(sc.H)
    cam = [sc.CAM[0], sc.CAM[1], sc.CAM[2] * s, sc.CAM[3] * t, sc.CAM[4] * s + (s - 1) / 2., sc.CAM[5] * t + (t - 1) / 2.]
    k = max(1, int(round(s)))
    tex = [sc.noise(d["cols"] * k, d["rows"] * k, d["seed"]) for d in [sc.BACKGROUND] + sc.PLANES]
    planes = [(tex[1 + i], p["pose"], p["width"], p["height"]) for i, p in enumerate(sc.PLANES)]
    return cam, tex[0], planes


def views(n):
    base = np.array(sc.VIEWS)
    out = [base[0]]
    for i in range(1, n):
        a, b = base[i % 3], base[(i + 1) % 3]
        w = (i // 3) / 3.
        out.append((1 - w) * a + w * b)
    return np.array(out[:n])


def main():
    for width, height in ((1181, 701), (sc.W, sc.H)):
        cam, background, planes = world(width, height)
        r = render.Renderer(cam, width, height, background, planes)
        for n in (1, 8):
            xi = views(n)
            t_image = timed(lambda: r.render(xi), r._stream)
            t_all = timed(lambda: r.render(xi, buffers=True), r._stream)
            image, depth, index, u, v = r.render(xi, buffers=True)
            counts = r.counts.sum(axis=0)
            n_taps, n_single = taps(index, u, v)
            if n_single != int(counts[4]):   # the recount's rounding rule is floor(x + 0.5), the library's is std::round
                print("warning: %d single-tap pixels recounted, the library counted %d: bilinear_taps is approximate" % (
                    n_single, int(counts[4])), file=sys.stderr)
            rec = {"workload": "render", "width": width, "height": height, "views": n, "ms": t_image[0] * 1e3,
                   "ms_min_max": [t_image[1] * 1e3, t_image[2] * 1e3], "ms_with_buffers": t_all[0] * 1e3,
                   "ms_per_view": t_image[0] * 1e3 / n, "Mpixel_per_s": n * width * height / t_image[0] / 1e6,
                   "counts": {k: int(c) for k, c in zip(render.COUNTS, counts)}, "bilinear_taps": n_taps, "single_tap_recount": n_single,
                   "taps_per_sampled_pixel": n_taps / max(1, int(counts[2] + counts[3] - counts[4])),
                   "Gtaps_per_s": n_taps / t_image[0] / 1e9, "texture_bytes": int(background.size + sum(p[0].size for p in planes)),
                   "library": os.environ.get("VISGEOM_AMD_LIBRARY", "default"), "reps": REPS}
            print(json.dumps(rec), flush=True)
        r.close()


if __name__ == "__main__":
    main()
