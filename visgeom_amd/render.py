"""Synthetic scene renderer on the GPU (include/visgeom_amd.h section 14): the reference's RenderDevice -- EUCM views of textured
planes in front of a panoramic background, with the hit buffers (range, object index, texture coordinates) behind every view.
Thin torch wrapper over a vg_render handle; library errors raise capi.VisgeomError, argument errors ValueError before the
library is called."""
import ctypes

import numpy as np

from . import capi
from ._handle import Handle, _vec

_dp = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)
COUNTS = ("not_reconstructed", "uncovered", "background", "plane", "single_tap")


def _texture(t, what):
    """a texture as a contiguous host uint8 array [rows, cols]"""
    if not isinstance(t, np.ndarray) or t.dtype != np.uint8 or t.ndim != 2:
        raise ValueError("%s must be a uint8 numpy array [rows, cols]" % what)
    if not all(capi.RENDER_MIN_SIDE <= s <= capi.RENDER_MAX_SIDE for s in t.shape):
        raise ValueError("%s: cols and rows must be in [%d, %d]" % (what, capi.RENDER_MIN_SIDE, capi.RENDER_MAX_SIDE))
    return np.ascontiguousarray(t)


def _poses(xi, what):
    """(poses as float64 [n, 6], single): host values only, finite"""
    try:
        import torch

        if isinstance(xi, torch.Tensor):
            raise ValueError("%s must be host values (a sequence or numpy array), not a tensor" % what)
    except ImportError:
        pass
    a = np.asarray(xi)
    if a.dtype.kind not in "fiu" or a.ndim not in (1, 2) or a.shape[-1] != 6:
        raise ValueError("%s must be 6 numbers [t, rotvec] or [n, 6]" % what)
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite" % what)
    return a.reshape(-1, 6), a.ndim == 1


class Renderer(Handle):
    """A vg_render handle on one device: an EUCM camera (`eucm`, 6 intrinsics) producing width x height images of a world --
    `background`, the panorama, and `planes`, a sequence of (texture, pose [t, rotvec], width, height in metres); textures are
    host uint8 numpy arrays [rows, cols].  The handle's stream is torch's current stream of the device at creation; a call is
    complete when it returns.  The counters of the last call are left in self.counts (int64 [n, 5]: COUNTS)."""

    _destroy = "vg_render_destroy"

    def __init__(self, eucm, width, height, background, planes, device=0):
        import torch

        self._c = _vec(eucm, 6, "eucm")
        if not all(isinstance(s, (int, np.integer)) and capi.RENDER_MIN_SIDE <= s <= capi.RENDER_MAX_SIDE for s in (width, height)):
            raise ValueError("width and height must be integers in [%d, %d]" % (capi.RENDER_MIN_SIDE, capi.RENDER_MAX_SIDE))
        planes = list(planes)
        if len(planes) > capi.RENDER_MAX_PLANES:
            raise ValueError("at most %d planes" % capi.RENDER_MAX_PLANES)
        self._textures = [_texture(background, "background")]   # kept alive until the library has copied them
        objs = (capi.RenderObject * (1 + len(planes)))()
        objs[0].kind = capi.RENDER_BACKGROUND
        for i, p in enumerate(planes):
            if len(p) != 4:
                raise ValueError("planes[%d] must be (texture, pose, width, height)" % i)
            self._textures.append(_texture(p[0], "planes[%d]: the texture" % i))
            pose, single = _poses(p[1], "planes[%d]: the pose" % i)
            if not single:
                raise ValueError("planes[%d]: the pose must be 6 numbers [t, rotvec]" % i)
            size = np.array([p[2], p[3]], dtype=np.float64)
            if not (np.isfinite(size).all() and (size > 0).all()):
                raise ValueError("planes[%d]: width and height must be positive" % i)
            o = objs[1 + i]
            o.kind = capi.RENDER_PLANE
            o.pose[:] = pose[0].tolist()
            o.width, o.height = float(size[0]), float(size[1])
        for o, t in zip(objs, self._textures):
            o.texture = t.ctypes.data
            o.rows, o.cols = t.shape
        self.device = torch.device("cuda", device)
        self.width, self.height = int(width), int(height)
        self.counts = None
        self._open(capi.load().vg_render_create, self._c.ctypes.data_as(_dp), self.width, self.height, len(objs), ctypes.byref(objs))
        self._textures = None

    def set_camera(self, eucm):
        """RenderDevice::setCamera: later views use these intrinsics"""
        c = _vec(eucm, 6, "eucm")
        capi.check(capi.load().vg_render_set_camera(self._h, c.ctypes.data_as(_dp)))
        self._c = c

    def render(self, xi_cam, buffers=False):
        """The view(s) at the camera pose(s) xi_cam ([6] or [n, 6] host values, [t, rotvec] of the camera in the world): a uint8
        CUDA tensor [H, W] or [n, H, W].  buffers=True: (image, depth, index, u, v) with depth, u, v float32 and index int16 --
        the range of the nearest hit (1e6 for none), the object hit (-1 none, 0 the background, k plane k) and its texture
        coordinates."""
        import torch

        xi, single = _poses(xi_cam, "xi_cam")
        n = xi.shape[0]
        if not 1 <= n <= 65535:
            raise ValueError("1 to 65535 views expected")
        shape = (n, self.height, self.width)
        image = torch.empty(shape, dtype=torch.uint8, device=self.device)
        extra = [torch.empty(shape, dtype=dt, device=self.device) for dt in (torch.float32, torch.int16, torch.float32, torch.float32)] \
            if buffers else [None] * 4
        counts = np.zeros((n, capi.RENDER_COUNTS), dtype=np.int64)
        self._enter()
        capi.check(capi.load().vg_render_views(self._h, n, xi.ctypes.data_as(_dp), image.data_ptr(),
                                               *[t.data_ptr() if t is not None else None for t in extra], counts.ctypes.data_as(_i64p)))
        self._leave(image, *extra)
        self.counts = counts
        out = (image,) + tuple(extra) if buffers else (image,)
        out = tuple(t[0] for t in out) if single else out
        return out if buffers else out[0]
