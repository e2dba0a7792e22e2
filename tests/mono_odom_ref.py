"""Plain numpy restatement of what the monocular odometry loop adds to the stages it calls (include/visgeom_amd.h section 15):
the host arithmetic of the reference's MonoOdometry (src/localization/mono_odom.cpp: feedWheelOdometry, the scale normalisation
of feedImage, isNewKeyframeNeeded, getCameraMotion), MonoOdometry::setDepth and ScalePhotometric::wrapImage
(src/localization/photometric.cpp:387-415).  Written from reading the reference, with the deviations of DESIGN.md section 9
("Monocular odometry"); the pose algebra is tests/photometric_ref.py's, the camera tests/photometric_ref.py's EUCM."""
import numpy as np

from tests import photometric_ref as pr

MIN_DEPTH, SET_DEPTH_SIGMA, DEFAULT_COST = 0.25, 0.1, 5.
COORD_LIMIT = 16777216.
DEFAULTS = dict(min_init_dist=0.25, max_dist=0.4, max_angle=np.pi / 4, min_scale_length=1e-2, max_scale_ratio=1.2, num_scales=5)
ZERO = np.zeros(6)


def inverse(a):
    return pr.inverse_compose(a, ZERO)


def integrate(xi_local, xi_odom_old, xi_odom_new):
    """xi_local.composeInverse(xi_odom).compose(xi_odom_new)"""
    return pr.compose(pr.compose(xi_local, inverse(xi_odom_old)), xi_odom_new)


def camera_motion(xi_base_cam, xi):
    """xi_base_cam.inverseCompose(xi).compose(xi_base_cam)"""
    return pr.compose(pr.inverse_compose(xi_base_cam, xi), xi_base_cam)


def normalize_scale(prm, old, prior, vo):
    """(xi_local, K, discarded, length, length_prior) of the scale normalisation (mono_odom.cpp:120-139)"""
    zeta_prior, zeta = pr.inverse_compose(old, prior), pr.inverse_compose(old, vo)
    length_prior, length = float(np.linalg.norm(zeta_prior[:3])), float(np.linalg.norm(zeta[:3]))
    with np.errstate(all="ignore"):
        K = float(np.float64(length_prior) / np.float64(length))
    if length > prm["min_scale_length"]:
        if K > prm["max_scale_ratio"]:
            return pr.compose(old, zeta_prior), K, True, length, length_prior
        zeta = np.concatenate([zeta[:3] * K, zeta[3:]])
    return pr.compose(old, zeta), K, False, length, length_prior


def needs_keyframe(prm, xi_local):
    xi_local = np.asarray(xi_local, float)
    return bool(np.linalg.norm(xi_local[:3]) > prm["max_dist"] or np.linalg.norm(xi_local[3:]) > prm["max_angle"])


def c_round(x):
    """C's round(): halves away from zero"""
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def set_depth(grid, image):
    """(depth, sigma) [y_max][x_max] of setDepth: map(x, y) = image(v0 + y scale, u0 + x scale), sigma 0.1"""
    yy, xx = np.mgrid[0:grid["y_max"], 0:grid["x_max"]]
    u, v = xx * grid["scale"] + grid["u0"], yy * grid["scale"] + grid["v0"]
    inside = (u >= 0) & (u < image.shape[1]) & (v >= 0) & (v < image.shape[0])
    depth = np.where(inside, image[np.clip(v, 0, image.shape[0] - 1), np.clip(u, 0, image.shape[1] - 1)].astype(np.float64), 0.)
    return depth, np.full(depth.shape, SET_DEPTH_SIGMA)


def warp_image(cam, grid, src, depth, motion, R_inv=None):
    """(dst u8 [h][w], near [h][w]) of wrapImage for the camera motion `motion` ([t, rotvec] of the new camera in the key frame's);
    near: the projected coordinate of the pixel lies within 1e-9 of a rounding boundary.  All arithmetic FP64 in the order of
    the reference: the normalised ray times the depth of the nearest map cell, inverseTransform, project, round."""
    h, w = src.shape
    motion = np.asarray(motion, float)
    Ri = pr.rotation_matrix(motion[3:]).T if R_inv is None else np.asarray(R_inv, float).reshape(3, 3)
    t = motion[:3]
    vv, uu = np.mgrid[0:h, 0:w]
    xd = c_round((uu - grid["u0"]).astype(np.float64) / grid["scale"]).astype(np.int64)
    yd = c_round((vv - grid["v0"]).astype(np.float64) / grid["scale"]).astype(np.int64)
    valid = (xd >= 0) & (xd < grid["x_max"]) & (yd >= 0) & (yd < grid["y_max"])
    d = np.where(valid, depth[np.clip(yd, 0, grid["y_max"] - 1), np.clip(xd, 0, grid["x_max"] - 1)], 0.)
    valid &= d >= MIN_DEPTH
    X, ok = pr.reconstruct(cam, uu.astype(np.float64), vv.astype(np.float64))
    valid &= ok
    with np.errstate(all="ignore"):
        nrm = np.sqrt(X[..., 0] * X[..., 0] + X[..., 1] * X[..., 1] + X[..., 2] * X[..., 2])
        X1 = np.stack([X[..., k] / nrm * d - t[k] for k in range(3)], -1)
        X2 = np.stack([Ri[k, 0] * X1[..., 0] + Ri[k, 1] * X1[..., 1] + Ri[k, 2] * X1[..., 2] for k in range(3)], -1)
        q, ok = pr.project(cam, X2)
        valid &= ok & (np.abs(q[..., 0]) <= COORD_LIMIT) & (np.abs(q[..., 1]) <= COORD_LIMIT)
        q = np.where(valid[..., None], q, 0.)
        u, v = c_round(q[..., 0]).astype(np.int64), c_round(q[..., 1]).astype(np.int64)
        frac = np.abs(np.abs(q) - np.floor(np.abs(q)) - 0.5)
    near = valid & ((frac[..., 0] < 1e-9) | (frac[..., 1] < 1e-9))
    inside = valid & (u >= 0) & (u < w) & (v >= 0) & (v < h)
    dst = np.where(inside, src[np.clip(v, 0, h - 1), np.clip(u, 0, w - 1)], 0).astype(np.uint8)
    return dst, near
