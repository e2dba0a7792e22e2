"""The scene of the renderer's tests: an 80 x 60 fisheye camera over a steeply slanted floor (the footprint grows to the cap of 24
taps), a small plane in front of it (odd texture sides) and a panoramic background, seen from three poses; the third looks
down through the small plane onto the floor, so that the depth test decides between two planes.  Textures are band-limited noise without flat areas, so that no pixel sits on a truncation boundary of the grey value.
Reference renders are computed once per (camera, view) and shared."""
import json
import os

import numpy as np

from tests import render_ref as rr

W, H = 80, 60
CAM = [0.75, 1.6, 40., 39., 39.5, 29.5]
CAM2 = [0.6, 1.2, 45., 44., 40.5, 30.5]   # for set_camera
VIEWS = [[0., 0., 0., 0., 0., 0.], [0.2, -0.05, 0.1, 0.05, -0.3, 0.1], [-0.1, -0.6, 0.1, -0.9, 0.1, -0.1]]
PLANES = [dict(cols=160, rows=120, seed=12, pose=[0., 0.6, 1.5, 1.35, 0., 0.], width=6., height=4.),
          dict(cols=53, rows=37, seed=13, pose=[-0.15, -0.1, 0.6, 0., 0.2, 0.1], width=0.5, height=0.35)]
BACKGROUND = dict(cols=128, rows=64, seed=11)


def noise(cols, rows, seed, waves=24):
    """a sum of plane waves with periods of 5 to 20 texels and random phases, around 128"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, waves)
    freq = 2 * np.pi / rng.uniform(5., 20., waves)
    ph = rng.uniform(0, 2 * np.pi, waves)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    s = np.zeros((rows, cols))
    for i in range(waves):
        s += np.sin(freq[i] * (np.cos(ang[i]) * xx + np.sin(ang[i]) * yy) + ph[i])
    return np.clip(128. + 80. * s / np.sqrt(waves / 2.) / 2., 0, 255).astype(np.uint8)


_CACHE = {}


def textures():
    """[background, plane 1, plane 2] as uint8 arrays"""
    if "tex" not in _CACHE:
        _CACHE["tex"] = [noise(d["cols"], d["rows"], d["seed"]) for d in [BACKGROUND] + PLANES]
    return _CACHE["tex"]


def planes():
    """[(texture, pose, width, height), ...]: the planes as render_ref.world and visgeom_amd.render.Renderer take them"""
    tex = textures()
    return [(tex[1 + i], p["pose"], p["width"], p["height"]) for i, p in enumerate(PLANES)]


def objects():
    if "objects" not in _CACHE:
        _CACHE["objects"] = rr.world(textures()[0], planes())
    return _CACHE["objects"]


def reference(k, cam=None):
    """the restatement's render of view k (read only: it is shared between tests)"""
    cam = CAM if cam is None else cam
    key = ("ref", k, tuple(cam))
    if key not in _CACHE:
        _CACHE[key] = rr.render(cam, W, H, objects(), VIEWS[k])
    return _CACHE[key]


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, dtype=np.uint8).tobytes())


def write_world(directory, views=None, **override):
    """world.json in the reference's schema plus "views", with its textures as PGM files next to it; the path of the JSON"""
    tex = textures()
    write_pgm(os.path.join(directory, "background.pgm"), tex[0])
    doc = dict(width=W, height=H, camera_params=CAM, background=dict(image_name="background.pgm"), planes=[],
               views=VIEWS if views is None else views)
    for i, p in enumerate(PLANES):
        write_pgm(os.path.join(directory, "plane_%d.pgm" % i), tex[1 + i])
        doc["planes"].append(dict(image_name="plane_%d.pgm" % i, pose=p["pose"], width=p["width"], height=p["height"]))
    doc.update(override)
    doc = {k: v for k, v in doc.items() if v is not None}
    path = os.path.join(directory, "world.json")
    with open(path, "w") as f:
        json.dump(doc, f)
    return path
