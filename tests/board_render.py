"""Renders a checkerboard through an EUCM or UCM camera for the corner detector's tests.

Every pixel is the mean of S x S samples placed symmetrically around its centre (pixel (x, y) covers [x - 0.5, x + 0.5] x
[y - 0.5, y + 0.5]: the library's convention, where the integer coordinate is the pixel centre).  Each sample's ray is
intersected with the board plane z = 0 of the board frame (X_cam = R X_board + t).  The board has cols x rows inner corners
at (size j, size i, 0); the squares run one square beyond them, and a white margin of half a square surrounds the squares.
Ground truth is the projection of the inner corners through tests/rectify_ref.project (the library's projection restated)."""
import numpy as np

from tests import rectify_ref

MODELS = {"eucm": 0, "ucm": 1}


def rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-15:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def unproject(model, p, u, v):
    """ray directions of pixel coordinates (inverse of rectify_ref.project) -> x, y, z"""
    if model == "eucm":
        alpha, beta, fu, fv, u0, v0 = p
        mx, my = (u - u0) / fu, (v - v0) / fv
        r2 = mx * mx + my * my
        with np.errstate(invalid="ignore"):
            mz = (1 - beta * alpha * alpha * r2) / (alpha * np.sqrt(1 - (2 * alpha - 1) * beta * r2) + (1 - alpha))
        return mx, my, mz
    xi, fu, fv, u0, v0 = p
    mx, my = (u - u0) / fu, (v - v0) / fv
    r2 = mx * mx + my * my
    with np.errstate(invalid="ignore"):
        f = (xi + np.sqrt(1 + (1 - xi * xi) * r2)) / (1 + r2)
    return f * mx, f * my, f - xi


def board_points(cols, rows, size):
    j, i = np.meshgrid(np.arange(cols), np.arange(rows))
    return np.stack([size * j.ravel(), size * i.ravel(), np.zeros(cols * rows)], axis=1).astype(np.float64)


def truth(model, intr, R, t, cols, rows, size):
    """[cols rows, 2] projections of the inner corners in board order, and whether all of them project"""
    X = board_points(cols, rows, size) @ np.asarray(R).T + np.asarray(t)
    u, v, ok = rectify_ref.project(MODELS[model], list(intr), X[:, 0], X[:, 1], X[:, 2])
    return np.stack([u, v], axis=1), bool(np.all(ok))


def render(model, intr, R, t, cols, rows, size, width, height, samples=8, dark=30., light=220., background=128.,
           gradient=(0., 0.), noise=0., seed=0):
    """u8 image [height, width]; gradient = (du, dv) grey levels per pixel added linearly, noise = sigma of seeded Gaussian
    noise (grey levels)"""
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    off = (np.arange(samples) + 0.5) / samples - 0.5
    acc = np.zeros((height, width), np.float64)
    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
    # board plane in camera frame: normal n = R[:, 2], point t; ray s d hits where n . (s d - t) = 0
    n = R[:, 2]
    for oy in off:
        for ox in off:
            x, y, z = unproject(model, intr, xs + ox, ys + oy)
            den = n[0] * x + n[1] * y + n[2] * z
            with np.errstate(divide="ignore", invalid="ignore"):
                s = (n @ t) / den
                P = np.stack([s * x - t[0], s * y - t[1], s * z - t[2]], axis=-1)
                B = P @ R   # R^T (P) per sample: board coordinates
            bx, by = B[..., 0] / size, B[..., 1] / size
            hit = np.isfinite(s) & (s > 0) & np.isfinite(bx)
            bx = np.where(hit, bx, -1e9)
            by = np.where(hit, by, -1e9)
            inside = (bx >= -1) & (bx <= cols) & (by >= -1) & (by <= rows)
            margin = (bx >= -1.5) & (bx <= cols + 0.5) & (by >= -1.5) & (by <= rows + 0.5)
            parity = (np.floor(bx).astype(np.int64) + np.floor(by).astype(np.int64)) % 2 == 0
            val = np.where(inside, np.where(parity, dark, light), np.where(margin, light, background))
            acc += val
    img = acc / (samples * samples)
    img = img + gradient[0] * (xs - width / 2) + gradient[1] * (ys - height / 2)
    if noise > 0:
        img = img + np.random.default_rng(seed).normal(0., noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def look_at_pose(centre_cam, yaw=0., pitch=0., roll=0., cols=9, rows=7, size=0.05):
    """board pose with the board's centre at centre_cam (camera frame), facing the camera (board z along camera +z), turned by
    roll about the board normal and tilted by yaw / pitch"""
    Rb = rodrigues([pitch, yaw, 0.]) @ rodrigues([0., 0., roll])
    c = np.array([(cols - 1) * size / 2, (rows - 1) * size / 2, 0.])
    t = np.asarray(centre_cam, np.float64) - Rb @ c
    return Rb, t


def expected_order(corners_truth):
    """the reference's order of the detected corners in board terms: row by row from the board corner with the smaller u + v of
    the two whose rows run along the board's x axis with the board's y axis turning clockwise from them in the image (for a
    board seen from its front these are board corners 0 and N - 1); starting from N - 1 reverses the board order"""
    T = np.asarray(corners_truth)
    return T if T[0].sum() < T[-1].sum() else T[::-1]
