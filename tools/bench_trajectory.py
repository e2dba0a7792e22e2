#!/usr/bin/env python3
"""One-GPU measurement of trajectory planning (include/visgeom_amd.h section 17; visgeom_amd/csrc/vg_trajectory.hpp): time per
call of TrajectoryPlanner.evaluate at n = 1, 21 and 21 x 64 points and of TrajectoryPlanner.optimize with 1 and 64 starts, from
HIP events on the handle's stream, with the kernel launches each call made.  tools only -- bench.py stays the driver's
contract.

The problem is the size the reference program runs: 2 trajectories of 30 poses in front of a 12 x 8 board; camera, extrinsics
and limits are those of tests/golden/trajectory_plan.json.  21 points are one numerical gradient (2 x 10 + 1), 21 x 64 the
round of 64 starts.  A call's time includes its copy up, its copy back and its synchronisation: that is what a caller waits for.

usage: python tools/bench_trajectory.py [reps]     (one JSON line per case)
"""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import trajectory_ref as tr  # noqa: E402
from visgeom_amd import trajectory  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
PLAN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "trajectory_plan.json")
STEPS = [30, 30]
START = np.array([0.2, 0.1, 0.05, 0.03, 0.02, -0.1, -0.2, -0.1, 0.02, -0.03])   # gentle arcs: all 58 poses see the board


def timed(fn, stream, reps):
    """median, min, max seconds of fn() over reps calls after two warm-ups, HIP events on `stream`"""
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
    cam, w, h, q, _, _ = tr.load_plan(PLAN)
    q = copy.deepcopy(q)
    q["board"] = dict(cols=12, rows=8, step=0.1)
    P = trajectory.TrajectoryPlanner(cam, w, h, q, STEPS)
    rng = np.random.default_rng(1)
    poses, corners = sum(STEPS) - len(STEPS), 12 * 8
    for n in (1, 21, 21 * 64):
        pts = START + 0.005 * rng.standard_normal((n, START.size))
        pts[0] = START
        before = P.launches
        cost, terms, invalid = P.evaluate(pts)
        launches = P.launches - before
        t = timed(lambda: P.evaluate(pts), P._stream, REPS)
        print(json.dumps({"workload": "trajectory_evaluate", "points": n, "trajectories": len(STEPS), "steps": STEPS, "board": [12, 8],
                          "launches_per_call": launches, "ms": t[0] * 1e3, "ms_min_max": [t[1] * 1e3, t[2] * 1e3],
                          "us_per_point": t[0] * 1e6 / n, "Mcorner_evaluations_per_s": n * poses * corners / t[0] / 1e6,
                          "invalid_points": int((invalid > 0).sum()), "cost_of_start": float(cost[0]), "reps": REPS}), flush=True)
    for n in (1, 64):
        starts = START + 0.02 * rng.standard_normal((n, START.size))
        starts[0] = START
        before = P.launches
        params, cost, iterations, termination = P.optimize(starts)
        launches = P.launches - before
        t = timed(lambda: P.optimize(starts), P._stream, max(3, REPS // 5))
        print(json.dumps({"workload": "trajectory_optimize", "starts": n, "trajectories": len(STEPS), "steps": STEPS, "board": [12, 8],
                          "launches_per_call": launches, "rounds": launches // 3, "ms": t[0] * 1e3, "ms_min_max": [t[1] * 1e3, t[2] * 1e3],
                          "ms_per_round": t[0] * 1e3 / max(1, launches // 3), "iterations_median": float(np.median(iterations)),
                          "iterations_max": int(iterations.max()), "cost_best": float(cost.min()), "cost_median": float(np.median(cost)),
                          "cost_of_start": float(P.evaluate(START)[0]),
                          "terminations": {str(k): int((termination == k).sum()) for k in sorted(set(termination.tolist()))},
                          "reps": max(3, REPS // 5)}), flush=True)
    P.close()


if __name__ == "__main__":
    main()
