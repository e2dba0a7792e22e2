"""Timeline of the headline emit launch from per-wave wall-clock stamps (measurement build of the library):

    python -m visgeom_amd._build --variant stamps -DVG_EMIT_STAMPS
    python tools/exp/emit_stamps_probe.py [--images 10000] [--model eucm] [--out FILE.md]

Every wave of vg_emit_kernel writes stamps of the 100 MHz wall clock (0 entry, 1 after the barrier, 2 at its first store,
3 after its last store was issued; 4 chain-parameter load issued, 5 its data arrived = start of the walk, walking waves only,
6 intrinsics in registers behind the barrier) to a side buffer; the buffer keeps the LAST launch of a train of 30 back-to-back
launches.  Printed: when the launch's first store leaves, the two store-less intervals of a wave split at the new stamps (first
round and median wave), per microsecond the waves resident, the waves between their first and last store ("storing") and the
workgroups started, and when residency starts to fall.  --lib NAME reads lib/variants/libvisgeom_amd_NAME.so (default: stamps)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from visgeom_amd import _build  # noqa: E402

PER_WAVE = 8   # kEmitStampsPerWave (vg_kernels.hpp)
_variant = sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else "stamps"
_build.LIB = os.path.join(_build.LIB_DIR, "variants", "libvisgeom_amd_%s.so" % _variant)

from visgeom_amd import CalibrationProblem, capi, synthetic  # noqa: E402


def timeline(model, n_images, train=30):
    d = synthetic.make_mono(model, n_images, 1)
    p = CalibrationProblem(0)
    cam = p.add_camera(model, d["init_intrinsics"])
    seq = p.add_transform(False, d["init_poses"])
    ds = p.add_dataset(cam, [(seq, 0)], d["board"], d["corners"])
    p.finalize()
    res, ji, jm = p.alloc_outputs(ds)
    p.prepare()
    n_obs = n_images * d["board"].shape[0]
    n_wg = (n_obs + 255) // 256
    stamps = torch.zeros(n_wg * 4 * PER_WAVE, dtype=torch.int64, device="cuda:0")
    try:
        for _ in range(5):
            p.evaluate_dataset(ds, res, ji, jm)
        p.synchronize()
        capi.debug_set("emit_stamps_waves", n_wg * 4)
        capi.debug_set("emit_stamps", stamps.data_ptr())
        for _ in range(train):
            p.evaluate_dataset(ds, res, ji, jm)
        p.synchronize()
    finally:
        capi.debug_set("emit_stamps", 0)
        capi.debug_set("emit_stamps_waves", 0)
    s = stamps.cpu().numpy().reshape(-1, PER_WAVE).astype(np.int64)
    p.close()
    return s


def report(s, title, out):
    ran = s[:, 0] != 0
    s = s[ran]
    # a train overwrites the buffer: a slow straggler of launch k - 1 cannot be told from launch k, but launches of one stream do
    # not overlap, so the last launch is everything within one launch length of the latest stamp
    t_end = s.max()
    s = s[s[:, 0] > t_end - 20000]   # 200 us: far more than one launch, far less than the train
    t0 = s[:, 0].min()
    us = lambda t: (t - t0) / 100.0
    work = s[s[:, 2] != 0]
    out.append("### %s\n" % title)
    out.append("waves that ran: %d, with stores: %d; launch (first entry to last store issued): %.2f us\n" % (len(s), len(work), us(work[:, 3].max())))
    out.append("first barrier passed at %.2f us, first store of the launch at %.2f us; median wave: entry -> barrier %.2f us, "
               "barrier -> first store %.2f us, first -> last store %.2f us, whole life %.2f us\n"
               % (us(s[:, 1].min()), us(work[:, 2].min()), np.median(work[:, 1] - work[:, 0]) / 100.0, np.median(work[:, 2] - work[:, 1]) / 100.0,
                  np.median(work[:, 3] - work[:, 2]) / 100.0, np.median(work[:, 3] - work[:, 0]) / 100.0))
    first_round = work[work[:, 0] < t0 + 50]
    out.append("first round (waves entered within 0.5 us): %d waves, their first stores at %.2f / %.2f / %.2f us (min / median / max)\n"
               % (len(first_round), us(first_round[:, 2].min()), us(np.median(first_round[:, 2])), us(first_round[:, 2].max())))
    split_table(work, first_round, out)
    end = np.where(work[:, 3] != 0, work[:, 3], work[:, 2])
    n_bins = int(us(end.max())) + 1
    out.append("| us | waves resident | waves storing | waves started |\n|---|---|---|---|\n")
    resident_peak, fall = 0, None
    rows = []
    for k in range(n_bins):
        t = t0 + 100 * k + 50   # the middle of the microsecond
        resident = int(((work[:, 0] <= t) & (end > t)).sum())
        storing = int(((work[:, 2] <= t) & (end > t)).sum())
        started = int(((work[:, 0] >= t0 + 100 * k) & (work[:, 0] < t0 + 100 * (k + 1))).sum())
        rows.append((k, resident, storing, started))
        resident_peak = max(resident_peak, resident)
    steady = np.median([r[1] for r in rows[len(rows) // 4: len(rows) // 2 + 1]])
    for k, resident, storing, started in rows:
        if fall is None and k > n_bins // 2 and resident < 0.9 * steady:
            fall = k
        out.append("| %d | %d | %d | %d |\n" % (k, resident, storing, started))
    out.append("\nsteady residency (median of the second quarter) %d waves; below 0.9 of it from %s us on; last store issued at %.2f us\n\n"
               % (steady, fall, us(end.max())))


def split_table(work, first_round, out):
    """the store-less intervals of a wave, split at stamps 4-6: medians in us over the first round and over all waves; the two
    intervals around the chain-parameter data only over the waves that walk (stamp 5 set)"""
    rows = [("entry -> chain load issued", 0, 4, False), ("chain load issued -> data arrived", 4, 5, True),
            ("walk -> barrier", 5, 1, True), ("barrier -> intrinsics in registers", 1, 6, False),
            ("intrinsics in registers -> first store", 6, 2, False)]
    out.append("\n| interval (median, us) | first round | all waves |\n|---|---|---|\n")
    for name, i, j, walking in rows:
        cells = []
        for w in (first_round, work):
            w = w[(w[:, i] != 0) & (w[:, j] != 0)]
            if walking:
                w = w[w[:, 5] != 0]
            cells.append("%.2f (%d waves)" % (np.median(w[:, j] - w[:, i]) / 100.0, len(w)) if len(w) else "-")
        out.append("| %s | %s | %s |\n" % (name, cells[0], cells[1]))
    out.append("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--model", default="eucm")
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default="stamps")
    a = ap.parse_args()
    out = []
    s = timeline(a.model, a.images)
    report(s, "%s, %d images, library %s" % (a.model, a.images, a.lib), out)
    text = "".join(out)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
