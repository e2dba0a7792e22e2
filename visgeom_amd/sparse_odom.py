"""Sparse visual odometry on the GPU (include/visgeom_amd.h section 13): the reference's SparseOdometry::feedData -- Harris
corners, 9 x 9 weighted patches, brute-force L1 matching with cross-check, a RANSAC of small reprojection solves with the
odometry prior, and two refinements -- from two consecutive images and the wheel odometry to the pose increment.  Thin torch
wrapper over a vg_sparse_odom handle; every stage is usable alone.  Library errors raise capi.VisgeomError, argument errors
ValueError before the library is called."""
import ctypes

import numpy as np

from . import capi
from ._handle import Handle, _f64_cuda, _is_cuda, _u8_images, _vec

_dp = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
DESC = 81
SOLVE_REPORT = ("iterations", "initial_cost", "final_cost", "termination")
RANSAC_REPORT = ("best", "inliers", "kept", "refine_cost", "refine_termination", "final_cost", "final_termination", "status")
FEED_REPORT = ("state", "keypoints", "matches", "reserved") + RANSAC_REPORT


def default_params(**changes):
    """vg_sparse_odom_params with the reference's constants; keyword arguments replace fields"""
    p = capi.SparseOdomParams()
    capi.load().vg_sparse_odom_params_default(ctypes.byref(p))
    for k, v in changes.items():
        if k not in dict(p._fields_):
            raise ValueError("vg_sparse_odom_params has no field %r" % k)
        setattr(p, k, v)
    return p


class SparseOdometry(Handle):
    """A vg_sparse_odom handle on one device: one EUCM camera, xi_base_cam and one image size.  Images are uint8 CUDA tensors
    [height, width] or [n, height, width]; rays, pixels and sizes float64 CUDA tensors; poses numpy [6] = [t, rotvec].  The
    handle's stream is torch's current stream of the device at creation; each call first makes it wait for the caller's
    current stream and is complete when it returns."""

    _destroy = "vg_sparse_odom_destroy"

    def __init__(self, eucm, xi_base_cam, width, height, params=None, device=0):
        import torch

        self._c = _vec(eucm, 6, "eucm")
        self._xbc = _vec(xi_base_cam, 6, "xi_base_cam")
        self.device = torch.device("cuda", device)
        self.params = params if params is not None else default_params()
        if not isinstance(self.params, capi.SparseOdomParams):
            raise ValueError("params must be a vg_sparse_odom_params (default_params())")
        self.width, self.height = int(width), int(height)
        self.max_features = self.params.max_features
        self._open(capi.load().vg_sparse_odom_create, self._c.ctypes.data_as(_dp), self._xbc.ctypes.data_as(_dp), self.width, self.height,
                   ctypes.byref(self.params))

    def _images(self, img):
        return _u8_images(img, self.height, self.width, "img")[0]

    def _points(self, x1, x2, p2, size=None):
        x1, x2, p2 = _f64_cuda(x1, (3,), "x1"), _f64_cuda(x2, (3,), "x2"), _f64_cuda(p2, (2,), "p2")
        m = x1.shape[0]
        if size is not None:
            size = _f64_cuda(size, (), "size")
        if x2.shape[0] != m or p2.shape[0] != m or (size is not None and size.shape[0] != m):
            raise ValueError("x1, x2, p2 and size must have the same length")
        return x1, x2, p2, size, m

    def _samples(self, samples):
        if samples is None:
            return None
        s = np.ascontiguousarray(samples, dtype=np.int32)
        if s.shape != (self.params.ransac_iterations, self.params.num_ransac_points):
            raise ValueError("samples must be [%d, %d]" % (self.params.ransac_iterations, self.params.num_ransac_points))
        return s

    def response(self, img):
        """the integer Harris map: int64 [n, height, width]"""
        import torch

        img = self._images(img)
        out = torch.empty(img.shape, dtype=torch.int64, device=self.device)
        self._enter()
        capi.check(capi.load().vg_sparse_odom_response(self._h, img.shape[0], img.data_ptr(), out.data_ptr()))
        return self._leave(out, img)[0]

    def detect(self, img):
        """(count int32 numpy [n], keypoints int32 [n, max_features, 2] as (u, v), descriptors float32 [n, max_features, 81])"""
        import torch

        img = self._images(img)
        n = img.shape[0]
        count = np.zeros(n, np.int32)
        kp = torch.empty((n, self.max_features, 2), dtype=torch.int32, device=self.device)
        desc = torch.empty((n, self.max_features, DESC), dtype=torch.float32, device=self.device)
        self._enter()
        capi.check(capi.load().vg_sparse_odom_detect(self._h, n, img.data_ptr(), count.ctypes.data_as(_i32p), kp.data_ptr(), desc.data_ptr()))
        self._leave(kp, desc, img)
        return count, kp, desc

    def match(self, count1, desc1, count2, desc2):
        """n pairs of descriptor sets ([n, max_features, 81] each, counts [n]): (match_count int32 numpy [n], matches int32
        [n, max_features, 2] ordered by the first index, distance float64 [n, max_features])"""
        import torch

        for d in (desc1, desc2):
            if not _is_cuda(d, torch.float32) or d.dim() != 3 or tuple(d.shape[1:]) != (self.max_features, DESC):
                raise ValueError("descriptors must be float32 CUDA tensors [n, %d, %d]" % (self.max_features, DESC))
        desc1, desc2 = desc1.contiguous(), desc2.contiguous()
        n = desc1.shape[0]
        c1, c2 = (np.ascontiguousarray(c, dtype=np.int32).reshape(-1) for c in (count1, count2))
        if desc2.shape[0] != n or c1.shape[0] != n or c2.shape[0] != n:
            raise ValueError("the two sides must hold the same number of sets")
        mc = np.zeros(n, np.int32)
        matches = torch.zeros((n, self.max_features, 2), dtype=torch.int32, device=self.device)
        dist = torch.zeros((n, self.max_features), dtype=torch.float64, device=self.device)
        self._enter()
        capi.check(capi.load().vg_sparse_odom_match(self._h, n, c1.ctypes.data_as(_i32p), desc1.data_ptr(), c2.ctypes.data_as(_i32p), desc2.data_ptr(),
                                                    mc.ctypes.data_as(_i32p), matches.data_ptr(), dist.data_ptr()))
        self._leave(matches, dist, desc1, desc2)
        return mc, matches, dist

    def solve(self, offsets, x1, x2, p2, size, xi_odom):
        """computeTransfSparse of the blocks [offsets[b], offsets[b + 1]) in one launch: (xi [n_blocks, 6], report [n_blocks, 4]:
        SOLVE_REPORT)"""
        x1, x2, p2, size, m = self._points(x1, x2, p2, size)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if off.shape[0] < 2 or off[0] != 0 or off[-1] > m or (np.diff(off) < 0).any():
            raise ValueError("offsets must rise from 0 to at most the number of points")
        xo = _vec(xi_odom, 6, "xi_odom")
        nb = off.shape[0] - 1
        out, rep = np.zeros((nb, 6)), np.zeros((nb, 4))
        self._enter()
        capi.check(capi.load().vg_sparse_odom_solve(self._h, nb, off.ctypes.data_as(_i64p), x1.data_ptr(), x2.data_ptr(), p2.data_ptr(), size.data_ptr(),
                                                    xo.ctypes.data_as(_dp), out.ctypes.data_as(_dp), rep.ctypes.data_as(_dp)))
        self._leave(x1, x2, p2, size)
        return out, rep

    def score(self, xi, x1, x2, p2, residuals=True):
        """the poses xi [n_hyp, 6] scored on the matches: (inliers int32 numpy [n_hyp], residual float64 [n_hyp, m] or None)"""
        import torch

        x1, x2, p2, _, m = self._points(x1, x2, p2)
        xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(-1, 6)
        n = xi.shape[0]
        res = torch.empty((n, m), dtype=torch.float64, device=self.device) if residuals else None
        inl = np.zeros(n, np.int32)
        self._enter()
        capi.check(capi.load().vg_sparse_odom_score(self._h, n, xi.ctypes.data_as(_dp), m, x1.data_ptr(), x2.data_ptr(), p2.data_ptr(),
                                                    res.data_ptr() if residuals else None, inl.ctypes.data_as(_i32p)))
        self._leave(res, x1, x2, p2)
        return inl, res

    def draw_samples(self, m):
        """the library's own sample table for m matches: int32 numpy [ransac_iterations, num_ransac_points]"""
        s = np.zeros((self.params.ransac_iterations, self.params.num_ransac_points), np.int32)
        capi.check(capi.load().vg_sparse_odom_draw_samples(self._h, int(m), s.ctypes.data_as(_i32p)))
        return s

    def ransac(self, x1, x2, p2, size, xi_odom, samples=None):
        """RANSAC and refinement of one frame pair: (xi_incr [6], mask uint8 [m] of the best hypothesis, report dict)"""
        import torch

        x1, x2, p2, size, m = self._points(x1, x2, p2, size)
        xo = _vec(xi_odom, 6, "xi_odom")
        s = self._samples(samples)
        out, rep = np.zeros(6), np.zeros(capi.SPARSE_ODOM_REPORT)
        mask = torch.zeros((m,), dtype=torch.uint8, device=self.device)
        self._enter()
        capi.check(capi.load().vg_sparse_odom_ransac(self._h, m, x1.data_ptr(), x2.data_ptr(), p2.data_ptr(), size.data_ptr(), xo.ctypes.data_as(_dp),
                                                     s.ctypes.data_as(_i32p) if s is not None else None, out.ctypes.data_as(_dp), mask.data_ptr(),
                                                     rep.ctypes.data_as(_dp)))
        self._leave(mask, x1, x2, p2, size)
        return out, mask, dict(zip(RANSAC_REPORT, rep))

    def feed(self, img, xi_odom_new, samples=None):
        """feedData: (xi_incr [6], report dict).  A given sample table is used modulo the number of matches found."""
        img = self._images(img)
        if img.shape[0] != 1:
            raise ValueError("feed takes one image")
        xo = _vec(xi_odom_new, 6, "xi_odom_new")
        s = self._samples(samples)
        out, rep = np.zeros(6), np.zeros(capi.SPARSE_ODOM_FEED_REPORT)
        self._enter()
        capi.check(capi.load().vg_sparse_odom_feed(self._h, img.data_ptr(), xo.ctypes.data_as(_dp), s.ctypes.data_as(_i32p) if s is not None else None,
                                                   out.ctypes.data_as(_dp), rep.ctypes.data_as(_dp)))
        self._leave(img)
        return out, dict(zip(FEED_REPORT, rep))

    @property
    def increment(self):
        out = np.zeros(6)
        capi.check(capi.load().vg_sparse_odom_increment(self._h, out.ctypes.data_as(_dp)))
        return out

    @property
    def integrated(self):
        out = np.zeros(6)
        capi.check(capi.load().vg_sparse_odom_integrated(self._h, out.ctypes.data_as(_dp)))
        return out
