"""The scene of the photometric mapping tests: camera, grid, xi_base_cam and world of tests/mono_odom_scene.py (256 x 192, three
pyramid levels), two passes of the base frame through it.

Pass 1 starts on an empty map, so SLAM builds it: the base frame moves mono_odom_scene.ZETA per frame.  Pass 2's last frame, TURN,
also yaws by more than the angular threshold -- the one way an inter frame that has just been pushed into the map is not
selected again at once (the angular threshold is not scaled by K).  Pass 2 is reinit-ed near pass 1's frame START2 with a
small lateral offset, rendered with another exposure (GAIN, OFFSET), runs along the map and off its end.  The thresholds are
shrunk through the parameters so that 31 frames reach every action and every warning (tests/test_mapping_cpu.py predicts
ACTIONS on the host under "every estimate is the truth").

Frame ROTATED's wheel odometry has its rotation component 2 off by ROT_ERROR, above rotation_tolerance; frame INFLATED's
odometry increment has its translation inflated by INFLATION.  Both are errors of one absolute odometry pose: the next pose
is the truth again."""
import numpy as np

from tests import mapping_ref as mp
from tests import mono_odom_scene as ms
from tests import photometric_ref as pr
from tests import photometric_scene as ps

W, H, NUM_SCALES, CAM, XI_BASE_CAM, GRID, STEREO = ms.W, ms.H, ms.NUM_SCALES, ms.CAM, ms.XI_BASE_CAM, ms.GRID, ms.STEREO
world, write_world = ms.world, ms.write_world
THRESHOLDS = dict(new_kf_distance_thresh=0.095, new_kf_angular_thresh=0.05, min_init_dist=0.11, num_scales=NUM_SCALES)
PRM = mp.squared(**THRESHOLDS)
ZETA = np.array(ms.ZETA)
N1, N2 = 15, 16
N_FRAMES = N1 + N2
TURN, TURN_YAW = N_FRAMES - 1, 0.06   # the last frame of pass 2
START2, LATERAL = 4, [0.01, 0., 0., 0., 0., 0.]   # pass 2 starts at pass 1's frame START2 moved by LATERAL
INFLATED, INFLATION = 4, 1.5       # a SLAM_REFINED frame of pass 1
ROTATED, ROT_ERROR = N1 + 5, 0.01  # a LOCALIZE frame of pass 2
GAIN, OFFSET = 0.8, 25.            # pass 2's exposure
INITIAL_OFFSET = ps.START_OFFSET   # 2.8 cm and 0.5 degrees: what the MI tests converge from
# what the frames reach when every estimate is the truth (tests/test_mapping_cpu.py); the map then holds frames 3, 8, 13, 29
ACTIONS = ["FIRST", "WAITING", "WAITING", "INIT_SLAM", "SLAM_REFINED", "SLAM_REFINED", "SLAM_ENTERED_MAP", "LOCALIZE_MAP_FRAME_KEPT",
           "LOCALIZE_LEFT_MAP", "SLAM_REFINED", "SLAM_REFINED", "SLAM_ENTERED_MAP", "LOCALIZE_MAP_FRAME_KEPT", "LOCALIZE_LEFT_MAP", "SLAM_REFINED",
           "FIRST", "WAITING", "WAITING", "INIT_LOCALIZE", "LOCALIZE_REFINED", "LOCALIZE_REFINED", "LOCALIZE_INTER_FRAME",
           "LOCALIZE_MAP_FRAME_CHANGED", "LOCALIZE_REFINED", "LOCALIZE_REFINED", "LOCALIZE_INTER_FRAME", "LOCALIZE_REFINED",
           "LOCALIZE_MAP_FRAME_KEPT", "LOCALIZE_MAP_FRAME_KEPT", "LOCALIZE_LEFT_MAP", "SLAM_INTER_FRAME"]
FIRST_LOCALIZE = N1 + 3            # pass 2's first LOCALIZE frame: INIT_LOCALIZE, MI against a frame of pass 1
_CACHE = {}


def passes():
    """[(first frame, frame count)] of the two passes"""
    return [(0, N1), (N1, N2)]


def true_poses():
    """the base frame's pose in the world at every frame of both passes, [N_FRAMES][6]"""
    if "true" not in _CACHE:
        xi, out = np.zeros(6), []
        for k in range(N1):
            out.append(xi)
            xi = pr.compose(xi, ZETA)
        xi = pr.compose(out[START2], LATERAL)
        for k in range(N1, N_FRAMES):
            out.append(xi)
            step = ZETA.copy()
            if k + 1 == TURN:
                step[4] += TURN_YAW
            xi = pr.compose(xi, step)
        _CACHE["true"] = np.array(out)
    return _CACHE["true"]


def initial(p):
    """what reinit is given before pass p (pass 0 starts from a fresh handle): the truth moved by INITIAL_OFFSET, which the
    first relocalisation has to take out again"""
    return pr.compose(true_poses()[passes()[p][0]], INITIAL_OFFSET)


def odometry():
    """the wheel odometry's absolute poses, [N_FRAMES][6]: the truth but for the two frames"""
    if "odom" not in _CACHE:
        odo = true_poses().copy()
        odo[ROTATED] = pr.compose(odo[ROTATED], [0., 0., 0., 0., 0., ROT_ERROR])
        step = pr.inverse_compose(odo[INFLATED - 1], odo[INFLATED])
        odo[INFLATED] = pr.compose(odo[INFLATED - 1], np.concatenate([INFLATION * step[:3], step[3:]]))
        _CACHE["odom"] = odo
    return _CACHE["odom"]


def camera_poses():
    """the camera's pose in the world at every frame: xi o xi_base_cam"""
    return np.array([pr.compose(xi, XI_BASE_CAM) for xi in true_poses()])


def truth_stages():
    """the callbacks of mapping_ref.Loop under "every estimate is the truth" """
    T = true_poses()
    return dict(sparse=lambda key, k: pr.inverse_compose(T[key], T[k]), photo=lambda inter, k, start: pr.inverse_compose(T[inter], T[k]),
                mi=lambda inter, frame, start: pr.inverse_compose(T[inter], T[frame[1]]))


def predict():
    """the reports of mapping_ref.Loop on the scene with truth_stages()"""
    loop, odo, reps = mp.Loop(PRM, XI_BASE_CAM, truth_stages()), odometry(), []
    for p, (first, count) in enumerate(passes()):
        if p:
            loop.reinit(initial(p))
        for k in range(first, first + count):
            loop.feed_odometry(odo[k])
            reps.append(loop.feed_image(k))
    return reps, loop


def exposure(img):
    """pass 2's exposure of a uint8 image (numpy): GAIN * img + OFFSET, rounded half up and saturated"""
    return np.clip(np.floor(GAIN * img.astype(np.float64) + OFFSET + 0.5), 0, 255).astype(np.uint8)


SMALL = dict(w=67, h=45, cam=[0.6, 1.05, 33., 32., 33.5, 22.5])   # an odd width, a pixel count that is no multiple of 256
SMALL["grid"] = dict(scale=2, u0=5, v0=4, x_max=(SMALL["w"] - 10) // 2 + 1, y_max=(SMALL["h"] - 8) // 2 + 1)
ALIGN_POSES = [[0.02, -0.01, 0.05, 0.01, -0.02, 0.005], [0.5, 0.1, -0.3, 0.05, 0.4, -0.1]]   # the second moves part of the image outside


def alignment_case(width, height, grid, seed):
    """(base, src, depth): two random images that contain zeros, and a map with a slanted surface, holes and depths below
    MIN_DEPTH"""
    rng = np.random.default_rng(seed)
    base, src = (rng.integers(1, 256, (height, width)).astype(np.uint8) for _ in range(2))
    base[rng.random(base.shape) < 0.03] = 0
    src[rng.random(src.shape) < 0.03] = 0
    yy, xx = np.mgrid[0:grid["y_max"], 0:grid["x_max"]]
    depth = 1. + 0.8 * xx / grid["x_max"] + 0.3 * yy / grid["y_max"]
    pick = rng.random(depth.shape)
    depth[pick < 0.05] = 0.
    depth[(pick >= 0.05) & (pick < 0.08)] = 0.1
    return base, src, depth


def alignment_cases():
    """[(name, cam, grid, base, src, depth)]: the scene's size and the small odd one"""
    return [("scene", CAM, GRID) + alignment_case(W, H, GRID, 41), ("small", SMALL["cam"], SMALL["grid"]) + alignment_case(SMALL["w"], SMALL["h"], SMALL["grid"], 42)]


def json_parameters():
    """the keys PhotometricMapping(ptree) reads, with the thresholds, for the mapping program and params_from_json"""
    doc = ms.json_parameters()
    del doc["mono_odom_parameters"]
    doc["mapping_parameters"] = dict(THRESHOLDS)
    return doc
