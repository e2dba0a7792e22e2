"""Fisheye line detection on the GPU (include/visgeom_amd.h section 19): the reference's hough_test -- straight 3D lines in one
unrectified EUCM image, voted for through a small EUCM accumulator camera.  Thin torch wrapper over a vg_hough handle; library
errors raise capi.VisgeomError, argument errors ValueError before the library is called."""
import ctypes

import numpy as np

from . import capi
from ._handle import Handle, _u8_images, _vec

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
COUNTS = ("selected", "not_reconstructed", "first_votes", "antipode_votes", "failed_projections", "outside")
FIELDS = {"centroid": slice(0, 2), "value": 2, "normal": slice(3, 6), "poly": slice(6, 12), "pt1": slice(12, 14), "pt2": slice(14, 16)}


def make_params(**fields):
    """vg_hough_params: the reference's constants, with the given fields replaced"""
    p = capi.HoughParams()
    capi.load().vg_hough_params_default(ctypes.byref(p))
    for k, v in fields.items():
        if k not in dict(capi.HoughParams._fields_):
            raise ValueError("vg_hough_params has no field %r" % k)
        setattr(p, k, v)
    return p


class Hough(Handle):
    """A vg_hough handle on one device: width x height images of the EUCM camera `eucm` (6 intrinsics) voting through the
    accumulator camera `acc_eucm` into an int32 accumulator [acc_h, acc_w] = [(int)(2 v0), (int)(2 u0)] of that camera.  The
    handle's stream is torch's current stream of the device at creation; a call is complete when it returns.  The counters of
    the last vote() are left in self.counts (int64 [n, 6]: COUNTS)."""

    _destroy = "vg_hough_destroy"

    def __init__(self, eucm, acc_eucm, width, height, params=None, device=0):
        import torch

        self._c, self._a = _vec(eucm, 6, "eucm"), _vec(acc_eucm, 6, "acc_eucm")
        if not all(isinstance(s, (int, np.integer)) for s in (width, height)):
            raise ValueError("width and height must be integers")
        if params is not None and not isinstance(params, capi.HoughParams):
            raise ValueError("params must be a vg_hough_params (make_params())")
        self.params = params if params is not None else make_params()
        self.device = torch.device("cuda", device)
        self.width, self.height = int(width), int(height)
        self.counts = None
        self._open(capi.load().vg_hough_create, self.width, self.height, self._c.ctypes.data_as(_dp), self._a.ctypes.data_as(_dp),
                   ctypes.byref(self.params))
        w, h = ctypes.c_int(), ctypes.c_int()
        capi.check(capi.load().vg_hough_size(self._h, ctypes.byref(w), ctypes.byref(h)))
        self.acc_w, self.acc_h = w.value, h.value

    def _images(self, images):
        img, single = _u8_images(images, self.height, self.width, "images")
        if not 1 <= img.shape[0] <= 65535:
            raise ValueError("1 to 65535 images expected")
        return img, single

    def vote(self, images):
        """Stage entry: the int32 accumulator(s) of the image(s), a CUDA tensor [acc_h, acc_w] or [n, acc_h, acc_w]"""
        import torch

        img, single = self._images(images)
        n = img.shape[0]
        acc = torch.empty((n, self.acc_h, self.acc_w), dtype=torch.int32, device=self.device)
        counts = np.zeros((n, capi.HOUGH_COUNTS), dtype=np.int64)
        self._enter()
        capi.check(capi.load().vg_hough_vote(self._h, n, img.data_ptr(), acc.data_ptr(), counts.ctypes.data_as(_i64p)))
        self._leave(img, acc)
        self.counts = counts
        return acc[0] if single else acc

    def detect(self, images, max_lines=256, blur=False):
        """The lines of the image(s): per image (lines float64 [k, 16], status int32 [k], count) with k = min(count, max_lines)
        -- a line is centroid (u, v), blurred value, unit normal, poly6, pt1, pt2 (FIELDS); status 1: no end points (NaN).
        One image gives one such tuple, a batch a list of them.  blur=True appends the blurred accumulator(s), a float32 CUDA
        tensor, to the result: (result, acc_blur)."""
        import torch

        img, single = self._images(images)
        n = img.shape[0]
        if not isinstance(max_lines, (int, np.integer)) or not 0 <= max_lines <= capi.HOUGH_MAX_LINES:
            raise ValueError("max_lines must be an integer in [0, %d]" % capi.HOUGH_MAX_LINES)
        lines = np.zeros((n, max_lines, capi.HOUGH_LINE))
        status = np.zeros((n, max_lines), dtype=np.int32)
        count = np.zeros(n, dtype=np.int32)
        acc_blur = torch.empty((n, self.acc_h, self.acc_w), dtype=torch.float32, device=self.device) if blur else None
        self._enter()
        capi.check(capi.load().vg_hough_detect(self._h, n, img.data_ptr(), int(max_lines), lines.ctypes.data_as(_dp), status.ctypes.data_as(_i32p),
                                               count.ctypes.data_as(_i32p), acc_blur.data_ptr() if blur else None))
        self._leave(img, acc_blur)
        out = [(lines[k, :min(int(count[k]), max_lines)], status[k, :min(int(count[k]), max_lines)], int(count[k])) for k in range(n)]
        out = out[0] if single else out
        return (out, acc_blur[0] if single else acc_blur) if blur else out


def polynomial(eucm, plane):
    """Host computePolynomial (vg_hough_polynomial): the conic [kuu, kuv, kvv, ku, kv, k1] of the plane's image"""
    c, p, out = _vec(eucm, 6, "eucm"), _vec(plane, 3, "plane"), np.zeros(6)
    capi.check(capi.load().vg_hough_polynomial(c.ctypes.data_as(_dp), p.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
    return out


def end_points(width, height, eucm, plane, poly):
    """Host findTerminalPoints (vg_hough_end_points): (pt4 = [pt1, pt2], status)"""
    c, p, q, out = _vec(eucm, 6, "eucm"), _vec(plane, 3, "plane"), _vec(poly, 6, "poly"), np.zeros(4)
    status = ctypes.c_int()
    capi.check(capi.load().vg_hough_end_points(int(width), int(height), c.ctypes.data_as(_dp), p.ctypes.data_as(_dp), q.ctypes.data_as(_dp),
                                               out.ctypes.data_as(_dp), ctypes.byref(status)))
    return out, status.value


def trace(poly, pt4, max_steps=capi.HOUGH_MAX_TRACE):
    """Host walk of the conic from round(pt1) until within 2 px (L1) of pt2 (vg_hough_trace): int32 [n, 2]"""
    q, p = _vec(poly, 6, "poly"), _vec(pt4, 4, "pt4")
    uv = np.zeros((max(int(max_steps), 1), 2), dtype=np.int32)
    n = ctypes.c_int()
    capi.check(capi.load().vg_hough_trace(q.ctypes.data_as(_dp), p.ctypes.data_as(_dp), int(max_steps), uv.ctypes.data_as(_i32p), ctypes.byref(n)))
    return uv[:n.value].copy()
