"""The motion stereo test sequence on tests/stereo_scene.py's planes: the key frame is camera 1 at the origin, the first further
view is the rig's second camera (the pair the SGM tests use) and four more views continue along the rig's baseline with small
rotations.  Poses are xi = [t, rotvec] of the view in the key frame; the views are rendered through CAM2."""
import numpy as np

from tests import stereo_ref, stereo_scene

# parameters of the motion stereo tests (the SGM tests' BASE plus gradient_thresh) and the epipole margin per rig
BASE = dict(u_max=125, v_max=93, u0=15, v0=15, equal_margins=1, disp_max=32, error_max=150, flaw_cost=25, desc_length=5,
            scales=[1, 2, 3, 5], desc_resp_thresh=2, use_uv_cache=0, gradient_thresh=2)
EPIPOLE_MARGIN = {"sideways": 2500, "vertical": 2500, "forward": 100}
STEPS = 4
_ROT = [(0.002, -0.003, 0.001), (-0.003, 0.002, 0.002), (0.001, 0.003, -0.002), (-0.002, -0.001, 0.003)]
_CACHE = {}


def poses(rig):
    """the STEPS further poses of `rig`: the baseline grows by a quarter per step, the rotation is perturbed"""
    xi = np.array(stereo_scene.RIGS[rig], dtype=np.float64)
    out = []
    for k in range(STEPS):
        p = xi.copy()
        p[:3] *= 1. + 0.25 * (k + 1)
        p[3:] += np.array(_ROT[k])
        out.append([float(v) for v in p])
    return out


def view(xi, u_max=125, v_max=93):
    """the u8 image of CAM2 at pose xi"""
    key = (tuple(xi), u_max, v_max)
    if key not in _CACHE:
        R = np.array(stereo_ref.rotation_matrix(xi[3:], 1.)).reshape(3, 3)
        _CACHE[key] = stereo_scene.render(stereo_scene.CAM2, R, np.array(xi[:3]), u_max, v_max)
    return _CACHE[key]


def prm_of(rig, **kw):
    d = dict(BASE, epipole_margin=EPIPOLE_MARGIN[rig])
    d.update(kw)
    return d


def write_sequence(directory, rig, stereo_parameters, sgm_frames=None, n_transformations=None):
    """a sequence for the `motion_stereo` program in `directory`: key.pgm (the key frame), view_<i>.pgm (the rig's second camera,
    then the further poses), sequence.json.  Returns (json path, images, poses) with poses[0] the key frame's identity."""
    import json
    import os

    img1, img2, _, xi = stereo_scene.make_scene(rig)
    all_poses = [[0.] * 6, list(xi)] + poses(rig)
    images = [img1, img2] + [view(q) for q in poses(rig)]
    names = ["key.pgm"] + ["view_%d.pgm" % i for i in range(1, len(images))]
    for name, im in zip(names, images):
        stereo_scene.write_pgm(os.path.join(directory, name), im)
    doc = {"camera_params_left": stereo_scene.CAM1, "camera_params_right": stereo_scene.CAM2, "images": names,
           "transformations": all_poses[:n_transformations] if n_transformations else all_poses,
           "stereo_parameters": stereo_parameters}
    if sgm_frames is not None:
        doc["sgm_frames"] = sgm_frames
    path = os.path.join(directory, "sequence.json")
    with open(path, "w") as f:
        json.dump(doc, f)
    return path, images, all_poses
