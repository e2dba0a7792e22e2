#!/usr/bin/env python3
"""One-GPU measurement of the monocular odometry loop (include/visgeom_amd.h section 15; visgeom_amd/csrc/vg_mono_odom_tu.hip):
HIP-event time per feed_image call of a REFINED frame and of a KEYFRAME frame, next to the sum of the stage calls made
separately on the same inputs, at the example size (1280 x 800 images, 1181 x 701 map) and at the test size (256 x 192, 113 x
81), in the world of tests/mono_odom_scene.py rendered on the device; and the accuracy of the scene's nine frames against
the renderer's ground truth -- per frame the translation and rotation error of the composed pose, the share of map cells with
a depth and their median relative error against the exact depth buffer of the key frame.  tools only -- bench.py stays the
driver's contract.

usage: python tools/bench_mono_odom.py [reps]     (one JSON object)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import mono_odom_ref as mr  # noqa: E402
from tests import mono_odom_scene as sc  # noqa: E402
from tests import photometric_ref as pr  # noqa: E402
from visgeom_amd import depth_fusion, mono_odom, motion_stereo, photometric, render, stereo  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
EXAMPLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ex_epipolar_stereo.json")


def once(fn, stream):
    """(milliseconds by HIP events on `stream`, the result) of one fn()"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    out = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ts):
    return {"ms": float(np.median(ts)), "ms_min_max": [float(min(ts)), float(max(ts))]}


def timed(fn, stream):
    fn()
    return stats([once(fn, stream)[0] for _ in range(REPS)])


def views(cam, w, h, poses):
    bg, planes = sc.world()
    r = render.Renderer(cam, w, h, bg, planes)
    img, depth = r.render(np.array([pr.compose(xi, sc.XI_BASE_CAM) for xi in poses]), buffers=True)[:2]
    r.close()
    return img, depth


def timing(cam, p, w, h):
    true = sc.true_poses()
    img, _ = views(cam, w, h, true[:8])
    odo = mono_odom.MonoOdometry(cam, sc.XI_BASE_CAM, p)
    st = odo._stream
    for k in range(4):
        odo.feed_wheel_odometry(true[k])
        rep = odo.feed_image(img[k])
    assert rep["action"] == "SPARSE_INIT_KEYFRAME", rep
    odo.feed_wheel_odometry(true[4])
    refined, actions = [], []
    for i in range(REPS + 1):   # the same image and odometry again: every call is a full REFINED frame
        ms, rep = once(lambda: odo.feed_image(img[4]), st)
        refined.append(ms)
        actions.append(rep["action"])
    local, key, cur = odo.xi_local, img[3], img[4]
    maps = [t.clone() for t in odo.map]
    # the stages of that frame, called separately on the same inputs
    ph = photometric.Photometric(cam, p.motion, sc.XI_BASE_CAM, w, h, p.num_scales)
    ms_ = motion_stereo.MotionStereo(cam, cam, p.motion)
    fu = depth_fusion.DepthFusion(cam, p.motion)
    ms_.set_base(key)
    motion = mono_odom.camera_motion(sc.XI_BASE_CAM, local)
    stages = {"photometric_set_base": timed(lambda: ph.set_base(key, maps[0]), st), "photometric_set_targets": timed(lambda: ph.set_targets(cur), st),
              "photometric_compute_pose": timed(lambda: ph.compute_pose(local, xi_prior=local), st),
              "motion_stereo_compute": timed(lambda: ms_.compute(motion, cur, prior=maps, out=maps), st),
              "filter_noise": timed(lambda: fu.filter_noise(maps[:2], out=maps[:2]), st)}
    out = {"width": w, "height": h, "x_max": odo.x_max, "y_max": odo.y_max, "refined": stats(refined[1:]), "refined_actions": sorted(set(actions)),
           "refined_stages": stages, "refined_stage_sum_ms": sum(v["ms"] for v in stages.values())}
    # key frames: back and forth between frame 7 and frame 3, 0.2 m apart, each call a KEYFRAME
    keyframe, actions = [], []
    for i in range(REPS + 1):
        k = 7 if i % 2 == 0 else 3
        odo.feed_wheel_odometry(true[k])
        ms, rep = once(lambda: odo.feed_image(img[k]), st)
        keyframe.append(ms)
        actions.append(rep["action"])
    inv = depth_fusion.pose_inverse(motion)

    def sgm():
        s = stereo.Stereo(cam, cam, inv, p.motion.stereo)
        res = s.compute(cur, key)[:3]
        s.close()
        return res

    new = sgm()
    warped = fu.warp(motion, maps)
    kstages = {"sgm_create_compute_destroy": timed(sgm, st), "warp": timed(lambda: fu.warp(motion, maps), st),
               "merge": timed(lambda: fu.merge(warped[:2], new[:2]), st), "motion_stereo_set_base": timed(lambda: ms_.set_base(cur), st)}
    out.update({"keyframe": stats(keyframe[1:]), "keyframe_actions": sorted(set(actions)), "keyframe_stages": kstages,
                "keyframe_stage_sum_ms": sum(v["ms"] for v in kstages.values()) + sum(stages[k]["ms"] for k in stages if k.startswith("photometric"))})
    for hnd in (odo, ph, ms_, fu):
        hnd.close()
    return out


def accuracy(cam, p, w, h, grid):
    """the scene's nine frames with its odometry (one increment inflated, one pose perturbed)"""
    true, odom = sc.true_poses(), sc.odometry()
    img, depth = views(cam, w, h, true)
    odo = mono_odom.MonoOdometry(cam, sc.XI_BASE_CAM, p)
    rows, key = [], 0
    for k in range(sc.N_FRAMES):
        odo.feed_wheel_odometry(odom[k])
        rep = odo.feed_image(img[k])
        if rep["action"].endswith("KEYFRAME") or rep["action"] == "FIRST":
            key = k
        err = pr.inverse_compose(true[k], odo.xi_composed)
        row = {"frame": k, "action": rep["action"], "K": rep["K"], "iterations": rep["iterations"], "translation_error_m": float(np.linalg.norm(err[:3])),
               "rotation_error_rad": float(np.linalg.norm(err[3:]))}
        if odo.state == "READY":
            d = odo.map[0].cpu().numpy()
            want = mr.set_depth(grid, depth[key].cpu().numpy())[0]
            have = (d > 0) & (want < 1e5)
            row.update({"key_frame": key, "depth_share": float(have.mean()),
                        "depth_median_relative_error": float(np.median(np.abs(d[have] - want[have]) / want[have])) if have.any() else None})
        rows.append(row)
    odo.close()
    return rows


def main():
    ex = json.load(open(EXAMPLE))
    mp = motion_stereo.params_from_json(ex["stereo_parameters"])
    big = mono_odom.make_params(motion=mp, min_init_dist=sc.THRESHOLDS["min_init_dist"], max_dist=sc.THRESHOLDS["max_dist"])
    small = mono_odom.make_params(motion=motion_stereo.make_params(**sc.STEREO), **sc.THRESHOLDS)
    cam = list(ex["camera_params_left"])
    s = mp.stereo
    big_grid = dict(scale=s.scale, u0=s.u0, v0=s.v0, x_max=(s.u_max - 2 * s.u0) // s.scale + 1, y_max=(s.v_max - 2 * s.v0) // s.scale + 1)
    rec = {"workload": "mono_odom", "reps": REPS, "library": os.environ.get("VISGEOM_AMD_LIBRARY", "default"),
           "example_size": timing(cam, big, s.u_max, s.v_max), "test_size": timing(sc.CAM, small, sc.W, sc.H),
           "accuracy_test_size": accuracy(sc.CAM, small, sc.W, sc.H, sc.GRID),
           "accuracy_example_size": accuracy(cam, big, s.u_max, s.v_max, big_grid)}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
