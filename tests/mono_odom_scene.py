"""The scene of the monocular odometry tests: the camera, depth grid and xi_base_cam of tests/photometric_scene.py (256 x 192,
scale 2, u0 = v0 = 16, three pyramid levels: the smallest shape at which the photometric margin leaves an interior at every scale)
in a world of the renderer's kind (tests/render_scene.py's band-limited noise): a tilted wall 1.5 m ahead, a small nearer plane
and a panorama.  The base frame moves 4 cm forward and 3 cm to the left per frame with a small yaw, nine frames.  The
thresholds are shrunk through the parameters so that the nine frames reach every action:

    frame   0      1, 2     3                     4        5 (inflated)  6         7        8 (perturbed)
    action  FIRST  WAITING  SPARSE_INIT_KEYFRAME  REFINED  DISCARDED     KEYFRAME  REFINED  REFINED

Frame 5's odometry increment has its translation inflated by 1.5.  Frame 8's wheel odometry is off by
photometric_scene.START_OFFSET, whose translation is perpendicular to the motion: the odometry's step is 1.14 times the true
one, below max_scale_ratio.  Both are errors of one absolute odometry pose: the next pose is the truth again.  The perturbed
frame is the last one because the frame after it would be discarded -- the odometry then steps back by the offset while the
scale normalisation has kept the odometry's length of the step before."""
import numpy as np

from tests import mono_odom_ref as mr
from tests import photometric_ref as pr
from tests import photometric_scene as ps
from tests import render_scene

W, H, NUM_SCALES, CAM, XI_BASE_CAM = ps.W, ps.H, ps.NUM_SCALES, ps.CAM, ps.XI_BASE_CAM
GRID = dict(ps.PRM)
STEREO = dict(scale=GRID["scale"], u0=GRID["u0"], v0=GRID["v0"], u_max=W, v_max=H, x_max=GRID["x_max"], y_max=GRID["y_max"], disp_max=48,
              error_max=150, flaw_cost=25, desc_length=5, scales=[1, 2, 3, 5], desc_resp_thresh=2, use_uv_cache=0)
THRESHOLDS = dict(min_init_dist=0.11, max_dist=0.13, num_scales=NUM_SCALES)
PRM = dict(mr.DEFAULTS, **THRESHOLDS)
ZETA = [-0.03, 0., 0.04, 0., 0.004, 0.]   # the increment of the base frame per frame
N_FRAMES, PERTURBED, INFLATED, INFLATION = 9, 8, 5, 1.5
ACTIONS = ["FIRST", "WAITING", "WAITING", "SPARSE_INIT_KEYFRAME", "REFINED", "DISCARDED", "KEYFRAME", "REFINED", "REFINED"]
KEYFRAMES = (0, 3, 6)   # the frames that become key frames when every estimate is the truth
PLANES = [dict(cols=800, rows=600, seed=21, pose=[0., 0., 1.5, 0.2, 0., 0.], width=8., height=6.),
          dict(cols=100, rows=80, seed=22, pose=[-0.3, -0.1, 1.0, 0., 0.25, 0.], width=0.5, height=0.4)]
BACKGROUND = dict(cols=128, rows=64, seed=23)
_CACHE = {}


def true_poses():
    """the base frame's pose in the world at every frame, [N_FRAMES][6]"""
    if "true" not in _CACHE:
        xi, out = np.zeros(6), []
        for _ in range(N_FRAMES):
            out.append(xi)
            xi = pr.compose(xi, ZETA)
        _CACHE["true"] = np.array(out)
    return _CACHE["true"]


def odometry():
    """the wheel odometry's absolute poses, [N_FRAMES][6]: the truth but for the two frames"""
    if "odom" not in _CACHE:
        odo = true_poses().copy()
        odo[PERTURBED] = odo[PERTURBED] + np.asarray(ps.START_OFFSET)
        big = np.concatenate([INFLATION * np.asarray(ZETA[:3]), ZETA[3:]])
        odo[INFLATED] = pr.compose(odo[INFLATED - 1], big)
        _CACHE["odom"] = odo
    return _CACHE["odom"]


def camera_poses():
    """the camera's pose in the world at every frame: xi o xi_base_cam"""
    return np.array([pr.compose(xi, XI_BASE_CAM) for xi in true_poses()])


def true_local(k):
    """the true pose of frame k's base in its key frame's base (the key frame at or before k - 1)"""
    key = max(i for i in KEYFRAMES if i < k)
    return pr.inverse_compose(true_poses()[key], true_poses()[k])


def odometry_local(k):
    """xi_local in front of frame k's photometric solve when frame k - 1 ended at the truth"""
    key = max(i for i in KEYFRAMES if i < k)
    prev = pr.inverse_compose(true_poses()[key], true_poses()[k - 1])
    return mr.integrate(prev, odometry()[k - 1], odometry()[k])


def textures():
    if "tex" not in _CACHE:
        _CACHE["tex"] = [render_scene.noise(d["cols"], d["rows"], d["seed"]) for d in [BACKGROUND] + PLANES]
    return _CACHE["tex"]


def world():
    """(background, planes) as visgeom_amd.render.Renderer takes them"""
    tex = textures()
    return tex[0], [(tex[1 + i], p["pose"], p["width"], p["height"]) for i, p in enumerate(PLANES)]


def write_world(directory):
    """world.json for the render / mono_odom programs with its textures next to it; the file name"""
    import json
    import os

    tex = textures()
    render_scene.write_pgm(os.path.join(directory, "background.pgm"), tex[0])
    doc = dict(width=W, height=H, camera_params=CAM, background=dict(image_name="background.pgm"), planes=[], views=[[0.] * 6])
    for i, p in enumerate(PLANES):
        render_scene.write_pgm(os.path.join(directory, "plane_%d.pgm" % i), tex[1 + i])
        doc["planes"].append(dict(image_name="plane_%d.pgm" % i, pose=p["pose"], width=p["width"], height=p["height"]))
    with open(os.path.join(directory, "world.json"), "w") as f:
        json.dump(doc, f)
    return "world.json"


def json_parameters():
    """the keys MonoOdometry(ptree) reads, with the thresholds, for the mono_odom program and params_from_json"""
    s = STEREO
    return {"camera_params": CAM, "xi_base_camera": XI_BASE_CAM,
            "stereo_parameters": {"scale": s["scale"], "u0": s["u0"], "v0": s["v0"], "uMax": W, "vMax": H, "xMax": s["x_max"], "yMax": s["y_max"],
                                  "stereo_parameters": {"disparity_max": s["disp_max"], "error_max": s["error_max"], "hypotheses": 1,
                                                        "flaw_cost": s["flaw_cost"], "descriptor_size": s["desc_length"], "scales": s["scales"],
                                                        "descriptor_response_thresh": s["desc_resp_thresh"]},
                                  "sgm_stereo_parameters": {"use_uv_cache": False}},
            "mono_odom_parameters": dict(THRESHOLDS)}
