"""The two frame loops (include/visgeom_amd.h sections 15 and 16) are built on one core, visgeom_amd/csrc/vg_frame_loop.hpp.  A
MonoOdometry and a PhotometricMapping handle on one device, fed alternately frame by frame, must each do what it does alone:
every report, every pose and the final map bit for bit.  The core keeps no state outside the handle.

The frames are the first ones of tests/mapping_scene.py, which are those of tests/mono_odom_scene.py (the same world, camera and
increment); each handle gets its own scene's wheel odometry.  Both scenes push their first key / inter frame at frame 3.  Mono
odometry refines at frame 4.  Mapping's frame 4 moves the camera 5 cm of truth (7.5 cm of inflated odometry) against a
min_stereo_base of 7 cm, so its frame 5, 10 cm from the inter frame, is the one that surely refines: six frames for both."""
import numpy as np
import pytest

from tests import mapping_scene as sc
from tests import mono_odom_scene as ms

pytestmark = pytest.mark.gpu
N_FRAMES = max(ms.ACTIONS.index("REFINED") + 1, sc.ACTIONS.index("SLAM_REFINED") + 2)


def make(kind):
    """(handle, feed odometry, the scene's odometry, the names of its pose getters)"""
    from visgeom_amd import mapping, mono_odom, motion_stereo

    motion = motion_stereo.make_params(**sc.STEREO)
    if kind == "mono":
        h = mono_odom.MonoOdometry(ms.CAM, ms.XI_BASE_CAM, mono_odom.make_params(motion=motion, **ms.THRESHOLDS))
        return h, h.feed_wheel_odometry, ms.odometry(), ("xi_local", "xi_global", "xi_composed")
    h = mapping.PhotometricMapping(sc.CAM, sc.XI_BASE_CAM, mapping.make_params(motion=motion, **sc.THRESHOLDS))
    return h, h.feed_odometry, sc.odometry(), ("xi_local", "xi_inter", "xi_composed")


def drive(kinds, img, samples):
    """the handles of `kinds` side by side, one frame of each in turn: per kind the reports, the poses after every frame and
    the final map"""
    made = {k: make(k) for k in kinds}
    out = {k: dict(reports=[], poses=[]) for k in kinds}
    try:
        for n in range(N_FRAMES):
            for k, (h, feed_odometry, odo, getters) in made.items():
                feed_odometry(odo[n])
                out[k]["reports"].append(h.feed_image(img[n], samples))
                out[k]["poses"].append(np.array([getattr(h, g) for g in getters]))
        for k, (h, _, _, _) in made.items():
            out[k]["map"] = [t.clone() for t in h.map]
    finally:
        for h, _, _, _ in made.values():
            h.close()
    return out


def same_report(a, b):
    """every field bit for bit (K is not finite for a pure rotation: equal_nan)"""
    if set(a) != set(b):
        return False
    for k in a:
        if isinstance(a[k], (str, bool, int)):
            if a[k] != b[k]:
                return False
        elif not np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True):
            return False
    return True


def test_two_loops_side_by_side_equal_each_alone():
    import torch

    from visgeom_amd.render import Renderer

    assert np.array_equal(sc.true_poses()[:N_FRAMES], ms.true_poses()[:N_FRAMES]) and (sc.W, sc.H, sc.CAM) == (ms.W, ms.H, ms.CAM)
    bg, planes = sc.world()
    r = Renderer(sc.CAM, sc.W, sc.H, bg, planes)
    img = r.render(sc.camera_poses()[:N_FRAMES])
    r.close()
    samples = np.random.default_rng(5).integers(0, 1 << 20, (200, 2)).astype(np.int32)
    alone = {k: drive([k], img, samples)[k] for k in ("mono", "mapping")}
    both = drive(["mono", "mapping"], img, samples)
    # both handles got where the shared steps are: a pushed key / inter frame with its SGM map, then a refined frame
    mono, mapped = alone["mono"]["reports"], alone["mapping"]["reports"]
    assert mono[3]["action"] == "SPARSE_INIT_KEYFRAME" and any(r["action"] == "REFINED" and r["counts"].any() for r in mono[4:])
    assert mapped[3]["action"] == "INIT_SLAM" and mapped[3]["sgm"] and any(r["refined"] and r["motion_counts"].any() for r in mapped[4:])
    for k in ("mono", "mapping"):
        a, b = alone[k], both[k]
        for n in range(N_FRAMES):
            print("%s frame %d: %s" % (k, n, b["reports"][n]["action"]))
            assert same_report(a["reports"][n], b["reports"][n]), (k, n, a["reports"][n], b["reports"][n])
            assert np.array_equal(a["poses"][n], b["poses"][n]), (k, n, a["poses"][n], b["poses"][n])
        for x, y in zip(a["map"], b["map"]):
            assert torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64)), k
