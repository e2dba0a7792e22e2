#!/usr/bin/env python3
"""One-GPU measurement of the emit step and the fused Gram of one mono dataset per camera model, the Kannala-Brandt ("kb") and
double-sphere ("ds") cameras next to EUCM and Mei.  bench.py's --model takes the reference's three models
only and stays the driver's contract; this tool times the two launches a calibration step is made of for any model the library has.

Per model, n images of the 8 x 12 board, chain [DIRECT]:
  emit      vg_dataset_evaluate with every Jacobian: residuals + K + 6 Jacobian columns per row, algorithmic bytes
            16 N (1 + K + 6) written + 16 N of observations read per image
  gram_sum  vg_dataset_gram_fused_sum: per-image blocks and their sum (the persistent form from 4 096 images)
Kernel time from HIP events around warmed, repeated launches (visgeom_amd.benchlib.timed).

usage: python tools/bench_camera_models.py [images [reps [model ...]]]     (one JSON line per model)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from visgeom_amd import CalibrationProblem, benchlib, capi, synthetic  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    images = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    models = sys.argv[3:] or ["eucm", "mei", "kb", "ds"]
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    base = min(images, 500)
    for model in models:
        d = synthetic.make_mono(model, base, 2)
        rep = (images + base - 1) // base   # the kernels' work does not depend on the values: the set repeated
        corners = d["corners"].repeat(rep, axis=0)[:images]
        poses = d["init_poses"].repeat(rep, axis=0)[:images]
        p = CalibrationProblem(0)
        cam = p.add_camera(model, d["init_intrinsics"])
        seq = p.add_transform(False, poses)
        ds = p.add_dataset(cam, [(seq, 0)], d["board"], corners)
        p.finalize()
        K, N = capi.NUM_INTRINSICS[capi.MODELS[model]], d["board"].shape[0]
        res, ji, jm = p.alloc_outputs(ds)
        gram, gsum = p.alloc_gram(ds)
        p.prepare()
        t_emit = benchlib.timed(lambda: p.evaluate_dataset(ds, res, ji, jm), reps)
        t_gram = benchlib.timed(lambda: p.gram_fused_sum(ds, gram, gsum), reps)
        emit_bytes = images * N * (16 * (1 + K + 6) + 16)
        print(json.dumps({"model": model, "images": images, "K": K, "reps": reps, "emit_us": round(t_emit * 1e6, 2),
                          "emit_bytes": emit_bytes, "emit_fraction_of_hbm_peak": round(emit_bytes / t_emit / HBM_PEAK, 3),
                          "gram_sum_us": round(t_gram * 1e6, 2), "failed": p.failed_count(ds)}), flush=True)
        p.close()


if __name__ == "__main__":
    main()
