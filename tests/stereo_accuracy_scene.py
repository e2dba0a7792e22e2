"""The sequence of the stereo_accuracy tests: the camera, depth grid, planes and stereo parameters of tests/mono_odom_scene.py (256 x
192, scale 2, a tilted wall 1.5 m ahead, a small nearer plane, a panorama), the camera starting at that scene's xi_base_cam and
moving by its increment, 5 cm per step: four steps, so that steps 0 and 1 run SGM and steps 2 and 3 motion stereo on the carried
map, and the cloud is written at the last one."""
import json
import os

import numpy as np

from tests import mono_odom_scene as ms

W, H, CAM, GRID, STEREO = ms.W, ms.H, ms.CAM, ms.GRID, ms.STEREO
INITIAL = list(ms.XI_BASE_CAM)
INCREMENT = list(ms.ZETA)
STEP_COUNT, CLOUD_STEP = 4, 3
NOISE_SEED = 20260928   # visgeom_amd.synthetic.BASE_SEED: the program's noise stream


def sequence(**kw):
    """the keys the stereo_accuracy program reads; kw overrides or, with a value of None, removes top-level keys"""
    doc = {"trajectory": {"initial": INITIAL, "increment": INCREMENT, "step_count": STEP_COUNT}, "camera_params": CAM,
           "stereo_parameters": ms.json_parameters()["stereo_parameters"], "render": "world.json", "noise": 0, "sgm": False,
           "filter_noise": True, "cloud_step": CLOUD_STEP}
    for k, v in kw.items():
        if v is None:
            doc.pop(k)
        else:
            doc[k] = v
    return doc


def write(directory, **kw):
    """world.json with its textures and sequence.json in `directory`; the sequence file's path"""
    ms.write_world(str(directory))
    path = os.path.join(str(directory), "sequence.json")
    with open(path, "w") as f:
        json.dump(sequence(**kw), f)
    return path


def noise_values(image, level, count):
    """floor(U level) for the pixels [0, count) of image number `image`: what the program subtracts"""
    from visgeom_amd import synthetic

    u = synthetic.uniform(NOISE_SEED, np.full(count, image, dtype=np.uint64), np.arange(count, dtype=np.uint64))
    return np.floor(u * level).astype(np.int64)
