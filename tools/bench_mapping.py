#!/usr/bin/env python3
"""One-GPU measurement of the photometric mapping loop (include/visgeom_amd.h section 16; visgeom_amd/csrc/vg_mapping_tu.hip):
HIP-event time per feed_image call, grouped by the action the frame took, over repeated runs of the two-pass scene of
tests/mapping_scene.py rendered on the device; the stage calls of a LOCALIZE frame made separately on the same inputs and their
sums per kind of frame; vg_photo_set_depth next to vg_photometric_set_base; the fused alignment launch; and the accuracy
of the scene's frames against the renderer's ground truth.  At the example size (1280 x 800 images, 1181 x 701 map) and at the
test size (256 x 192, 113 x 81).  tools only -- bench.py stays the driver's contract.

usage: python tools/bench_mapping.py [reps]     (one JSON object)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import mapping_scene as sc  # noqa: E402
from tests import photometric_ref as pr  # noqa: E402
from visgeom_amd import capi, depth_fusion, mapping, mono_odom, motion_stereo, photometric, render, stereo  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
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
    return {"ms": float(np.median(ts)), "ms_min_max": [float(min(ts)), float(max(ts))], "n": len(ts)}


def timed(fn, stream):
    fn()
    return stats([once(fn, stream)[0] for _ in range(max(REPS, 5))])


def views(cam, w, h):
    bg, planes = sc.world()
    r = render.Renderer(cam, w, h, bg, planes)
    img = r.render(sc.camera_poses())
    r.close()
    img[sc.N1:] = torch.from_numpy(sc.exposure(img[sc.N1:].cpu().numpy())).to(img.device)
    return img


def scene_run(cam, p, img, times=None, rows=None):
    """both passes on a fresh handle; the handle and what the test of a LOCALIZE_REFINED frame needs, taken in front of the last one"""
    h = mapping.PhotometricMapping(cam, sc.XI_BASE_CAM, p)
    odo, true, keep = sc.odometry(), sc.true_poses(), None
    for n, (first, count) in enumerate(sc.passes()):
        if n:
            h.reinit(sc.initial(n))
        actions = []
        for k in range(first, first + count):
            h.feed_odometry(odo[k])
            if h.state == "LOCALIZE":   # candidate inputs of the stage timings: the state in front of a LOCALIZE frame
                before = dict(local=h.xi_local, inter=h.xi_inter, map=[t.clone() for t in h.map], index=h.map_index, frame=k)
            ms, rep = once(lambda: h.feed_image(img[k]), h._stream)
            if rep["action"] == "LOCALIZE_REFINED" and rep["refined"]:
                keep = dict(before, inter_frame=max(j for j in range(first, k) if actions[j - first] not in ("FIRST", "WAITING", "LOCALIZE_REFINED", "SLAM_REFINED")))
            actions.append(rep["action"])
            if times is not None:
                times.setdefault(rep["action"], []).append(ms)
            if rows is not None:
                err = pr.inverse_compose(true[k], h.xi_composed)
                rows.append({"frame": k, "action": rep["action"], "warning": rep["warning"], "map_index": rep["map_index"], "iterations": rep["iterations"],
                             "mi_iterations": rep["mi_iterations"], "translation_error_m": float(np.linalg.norm(err[:3])),
                             "rotation_error_rad": float(np.linalg.norm(err[3:])),
                             "alignment_mean_abs": (lambda s: float(s[1]) / max(int(s[0]), 1))(h.alignment(img[k], err=False)[1]) if rep["state"] in ("LOCALIZE", "SLAM") else None})
    return h, keep


def size(cam, p, w, h):
    img = views(cam, w, h)
    times, rows = {}, []
    hnd, keep = scene_run(cam, p, img)   # warm-up: every pipeline's first-call allocations
    hnd.close()
    for i in range(REPS):
        hnd, keep = scene_run(cam, p, img, times, rows if i == 0 else None)
        if i < REPS - 1:
            hnd.close()
    out = {"width": w, "height": h, "x_max": hnd.x_max, "y_max": hnd.y_max, "frames_in_map": hnd.num_frames,
           "feed_image_by_action": {a: stats(t) for a, t in sorted(times.items())}, "accuracy": rows}
    st = hnd._stream
    if keep is not None:   # the stages of a LOCALIZE frame, called separately on that frame's inputs
        cur, inter, maps, local = img[keep["frame"]], img[keep["inter_frame"]], keep["map"], keep["local"]
        xi_map, map_img = hnd.get_frame(keep["index"])
        ph = photometric.Photometric(cam, p.motion, sc.XI_BASE_CAM, w, h, p.num_scales)
        ms_ = motion_stereo.MotionStereo(cam, cam, p.motion)
        fu = depth_fusion.DepthFusion(cam, p.motion)
        ms_.set_base(inter)
        base = mono_odom.camera_motion(sc.XI_BASE_CAM, local)
        inv = depth_fusion.pose_inverse(base)
        start = depth_fusion.pose_in_frame(keep["inter"], xi_map)

        def sgm():
            s = stereo.Stereo(cam, cam, inv, p.motion.stereo)
            res = s.compute(cur, inter)[:3]
            s.close()
            return res

        ph.set_base(inter, maps[0])
        stages = {"photometric_set_base": timed(lambda: ph.set_base(inter, maps[0]), st), "photometric_set_depth": timed(lambda: ph.set_depth(maps[0]), st),
                  "photometric_set_targets": timed(lambda: ph.set_targets(cur), st),
                  "photometric_compute_pose": timed(lambda: ph.compute_pose(local, xi_prior=local), st),
                  "motion_stereo_compute": timed(lambda: ms_.compute(base, cur, prior=maps), st),
                  "filter_noise": timed(lambda: fu.filter_noise(maps), st), "sgm_create_compute_destroy": timed(sgm, st),
                  "warp": timed(lambda: fu.warp(base, maps), st), "motion_stereo_set_base": timed(lambda: ms_.set_base(cur), st)}
        new, warped = sgm(), fu.warp(base, maps)
        stages["merge"] = timed(lambda: fu.merge(warped[:2], new[:2]), st)
        ph.set_targets(map_img)
        stages["mi_compute_pose"] = timed(lambda: ph.compute_pose_mi(start, xi_odom=local), st)
        photo = ["photometric_set_depth", "photometric_set_targets", "photometric_compute_pose"]
        push = ["sgm_create_compute_destroy", "filter_noise", "warp", "merge", "motion_stereo_set_base"]
        mi = ["photometric_set_base", "photometric_set_targets", "mi_compute_pose"]
        total = lambda names: sum(stages[k]["ms"] for k in names)   # noqa: E731
        out.update({"stage_inputs": {"frame": keep["frame"], "inter_frame": keep["inter_frame"], "map_frame": keep["index"]}, "stages": stages,
                    "stage_sum_ms": {"refined": total(photo + ["motion_stereo_compute", "filter_noise"]), "inter_frame_with_mi": total(photo + push + mi),
                                     "inter_frame_without_mi": total(photo + push)},
                    "set_depth_over_set_base": stages["photometric_set_depth"]["ms"] / stages["photometric_set_base"]["ms"]})
        for x in (ph, ms_, fu):
            x.close()
        # the fused alignment launch, next to the warp kernel alone (which writes the warped image and compares nothing)
        mo = mono_odom.MonoOdometry(cam, sc.XI_BASE_CAM, mono_odom.make_params(motion=p.motion, num_scales=p.num_scales))
        out["alignment"] = {"with_error_image": timed(lambda: hnd.alignment(cur, local, base=inter, depth=maps[0]), st),
                            "sums_only": timed(lambda: hnd.alignment(cur, local, base=inter, depth=maps[0], err=False), st),
                            "warp_image_alone": timed(lambda: mo.warp_image(cur, local, maps[0]), st)}
        mo.close()
    hnd.close()
    return out


def main():
    ex = json.load(open(EXAMPLE))
    mp = motion_stereo.params_from_json(ex["stereo_parameters"])
    thresholds = {k: v for k, v in sc.THRESHOLDS.items() if k != "num_scales"}
    big = mapping.make_params(motion=mp, **thresholds)
    small = mapping.make_params(motion=motion_stereo.make_params(**sc.STEREO), **sc.THRESHOLDS)
    rec = {"workload": "mapping", "reps": REPS, "library": os.environ.get("VISGEOM_AMD_LIBRARY", "default"), "test_size": size(sc.CAM, small, sc.W, sc.H)}
    try:
        rec["example_size"] = size(list(ex["camera_params_left"]), big, mp.stereo.u_max, mp.stereo.v_max)
    except capi.VisgeomError as e:   # the scene's thresholds are tuned for the test camera: report, do not hide
        rec["example_size"] = {"error": str(e)}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
