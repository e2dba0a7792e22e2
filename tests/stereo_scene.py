"""Synthetic EUCM stereo pairs for the stereo tests: textured planes ray cast into both cameras with supersampling (like
board_render.py), a band-limited random texture fixed to the planes, and the true range along camera 1's rays per depth
pixel.  Three rigs: a sideways baseline, a vertical one, and a mostly forward one whose epipoles lie inside the images.
Planes, patch, texture periods and cameras are arguments whose defaults are those three rigs' world; STRIP is a fourth
scene built from them, a wide low pair in front of a near, steep wall whose disparities span 0 ... 255 (see make_strip)."""
import numpy as np

from tests import stereo_ref

CAM1 = [0.6, 1.05, 62., 61., 62.5, 46.5]
CAM2 = [0.59, 1.0, 61.5, 61.2, 62., 47.]
# xi12: the pose of camera 2 in camera 1, [t, rotvec]
RIGS = {
    "sideways": [0.2, 0.004, -0.003, 0.004, -0.006, 0.01],
    "vertical": [0.003, 0.2, 0.002, -0.005, 0.004, 0.006],
    "forward": [0.03, 0.02, 0.25, 0.003, -0.004, 0.002],
}
# planes n . X = d in camera 1's frame, nearest hit wins: a slanted wall and a closer patch
PLANES = [(np.array([0.0, -0.25, 1.0]), 1.4), (np.array([0.3, 0.0, 1.0]), 0.9)]
PATCH = (-0.35, 0.05, -0.3, 0.1)   # the second plane only where x in [a, b], y in [c, d] (camera 1 frame)
PERIODS = (0.05, 0.2)              # the texture's band: periods of its plane waves, metres

# The strip scene: 400 x 49 images, a 0.3 m baseline and one wall.  The "steep" wall n . X = 0.45 runs from 0.2 m to 2 m
# range across the depth grid (96 x 16 pixels from (292, 16)), so the winners cover the whole of [0, 256) while every
# camera-2 walk of 256 steps stays inside the image; the "flat" wall faces the cameras at 0.7 m (disparities 56 ... 67), for
# descriptors too long to match across the steep wall's foreshortening.  The "fine" texture gives descriptor step 1 nearly
# everywhere; "coarse" and "broad" have flat stretches where the descriptor falls through to the larger scales.
STRIP = {
    "cam1": [0.6, 1.05, 160., 159., 341.5, 24.5],
    "cam2": [0.59, 1.0, 159.5, 160.2, 340., 25.],
    "xi12": [0.3, 0.004, -0.003, 0.004, -0.006, 0.01],
    "planes": {"steep": [(np.array([2.2, -0.1, 1.0]), 0.45)], "flat": [(np.array([0.0, 0.0, 1.0]), 0.7)]},
    "periods": {"fine": (0.01, 0.05), "coarse": (0.03, 0.4), "broad": (0.1, 0.4)},
    "u_max": 400, "v_max": 49,
    "grid": dict(u0=292, v0=16, x_max=96, y_max=16, scale=1),
}


def reconstruct_np(c, u, v):
    alpha, beta, fu, fv, u0, v0 = c
    xn, yn = (u - u0) / fu, (v - v0) / fv
    u2 = xn * xn + yn * yn
    gamma = 1. - alpha
    det = np.maximum(1 - (alpha - gamma) * beta * u2, 0.)
    z = (1. - u2 * alpha * alpha * beta) / (gamma + alpha * np.sqrt(det))
    return np.stack([xn, yn, z], -1)


def texture(P, seed=7, k=24, periods=PERIODS):
    """band-limited random texture on world points P [..., 3]: a sum of k plane waves, periods 0.05 - 0.2 m by default"""
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(k, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    freq = 2 * np.pi / rng.uniform(periods[0], periods[1], k)
    ph = rng.uniform(0, 2 * np.pi, k)
    s = np.zeros(P.shape[:-1])
    for i in range(k):
        s += np.sin(P @ (dirs[i] * freq[i]) + ph[i])
    return 128. + 95. * s / np.sqrt(k / 2.) / 2.


def cast(origin, dirs, planes=PLANES, patch=PATCH):
    """nearest plane hit along rays origin + lam dirs (camera 1 frame): lam [...], inf where none.  `patch` bounds the
    second plane (None: unbounded)."""
    best = np.full(dirs.shape[:-1], np.inf)
    for i, (n, d) in enumerate(planes):
        den = dirs @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            lam = (d - origin @ n) / den
        ok = (den != 0) & (lam > 0)
        if i == 1 and patch is not None:
            P = origin + lam[..., None] * dirs
            ok &= (P[..., 0] >= patch[0]) & (P[..., 0] <= patch[1]) & (P[..., 1] >= patch[2]) & (P[..., 1] <= patch[3])
        best = np.where(ok & (lam < best), lam, best)
    return best


def render(cam, R, t, w, h, ss=3, planes=PLANES, patch=PATCH, periods=PERIODS):
    """u8 image [h][w] of camera `cam` at pose (R, t) in camera 1's frame, ss x ss samples per pixel"""
    acc = np.zeros((h, w))
    offs = (np.arange(ss) + 0.5) / ss - 0.5
    vv, uu = np.mgrid[0:h, 0:w].astype(float)
    for oy in offs:
        for ox in offs:
            d = reconstruct_np(cam, uu + ox, vv + oy) @ np.asarray(R).T
            lam = cast(np.asarray(t), d, planes, patch)
            P = np.asarray(t) + np.where(np.isfinite(lam), lam, 0.)[..., None] * d
            acc += np.where(np.isfinite(lam), texture(P, periods=periods), 128.)
    return np.clip(np.rint(acc / (ss * ss)), 0, 255).astype(np.uint8)


def true_range(cam1, u0, v0, x_max, y_max, scale=1, planes=PLANES, patch=PATCH):
    """the range along camera 1's ray of every depth pixel (u0 + x scale, v0 + y scale): [y_max][x_max], 0 where no plane"""
    yy, xx = np.mgrid[0:y_max, 0:x_max]
    d = reconstruct_np(cam1, (xx * scale + u0).astype(float), (yy * scale + v0).astype(float))
    lam = cast(np.zeros(3), d, planes, patch)
    rng = lam * np.linalg.norm(d, axis=-1)
    return np.where(np.isfinite(rng), rng, 0.)


def make_scene(rig, u_max=125, v_max=93, margin=15, scale=1, cam1=CAM1, cam2=CAM2, planes=PLANES, patch=PATCH, periods=PERIODS):
    """(img1, img2, true_range [y_max][x_max], xi12): the range along camera 1's ray of every depth pixel.  `rig` names an
    entry of RIGS or is xi12 itself."""
    xi = RIGS[rig] if isinstance(rig, str) else list(rig)
    R = np.array(stereo_ref.rotation_matrix(xi[3:], 1.)).reshape(3, 3)
    img1 = render(cam1, np.eye(3), np.zeros(3), u_max, v_max, planes=planes, patch=patch, periods=periods)
    img2 = render(cam2, R, np.array(xi[:3]), u_max, v_max, planes=planes, patch=patch, periods=periods)
    x_max = (u_max - 2 * margin) // scale + 1
    y_max = (v_max - 2 * margin) // scale + 1
    return img1, img2, true_range(cam1, margin, margin, x_max, y_max, scale, planes, patch), xi


def make_strip(tex="fine", wall="steep"):
    """(img1, img2, true_range over STRIP's grid, xi12) of the strip scene with one of STRIP's textures and walls"""
    S = STRIP
    planes = S["planes"][wall]
    img1, img2, _, xi = make_scene(S["xi12"], S["u_max"], S["v_max"], cam1=S["cam1"], cam2=S["cam2"], planes=planes,
                                   patch=None, periods=S["periods"][tex])
    return img1, img2, true_range(S["cam1"], planes=planes, patch=None, **S["grid"]), xi


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, dtype=np.uint8).tobytes())


def write_case(directory, rig, stereo_parameters, images=None, brightness=50):
    """an ex_epipolar_stereo.json-style case for the `stereo` program in `directory`: left.pgm, right.pgm, case.json (image
    paths relative to the JSON).  Returns the JSON path."""
    import json
    import os

    img1, img2, _, xi = images if images is not None else make_scene(rig)
    write_pgm(os.path.join(directory, "left.pgm"), img1)
    write_pgm(os.path.join(directory, "right.pgm"), img2)
    doc = {"camera_params_left": CAM1, "camera_params_right": CAM2, "stereo_transformation": list(xi),
           "image_left": "left.pgm", "image_right": "right.pgm", "brightness": brightness,
           "stereo_parameters": stereo_parameters}
    path = os.path.join(directory, "case.json")
    with open(path, "w") as f:
        json.dump(doc, f)
    return path


def read_pfm(path):
    """float32 [h][w] of a little-endian PFM written bottom row first"""
    with open(path, "rb") as f:
        data = f.read()
    head, pos = [], 0
    while len(head) < 3:
        end = data.index(b"\n", pos)
        head.append(data[pos:end].decode())
        pos = end + 1
    assert head[0] == "Pf" and float(head[2]) < 0
    w, h = map(int, head[1].split())
    return np.frombuffer(data[pos:pos + 4 * w * h], dtype="<f4").reshape(h, w)[::-1]


# the sideways scene as "stereo_parameters" of the stereo program's JSON (see tests/test_gpu_stereo.py BASE)
SCENE_JSON_PARAMS = {
    "scale": 1, "u0": 15, "v0": 15, "uMax": 125, "vMax": 93, "equal_margins": True,
    "stereo_parameters": {"disparity_max": 32, "error_max": 150, "hypotheses": 1, "flaw_cost": 25, "descriptor_size": 5,
                          "scales": [1, 2, 3, 5], "descriptor_response_thresh": 2},
    "sgm_stereo_parameters": {"step_cost": 5, "jump_cost": 32, "image_based_cost": True, "salient_points_only": True,
                              "use_uv_cache": False},
}
