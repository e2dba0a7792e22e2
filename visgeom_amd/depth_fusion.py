"""Depth map propagation and fusion on the GPU (include/visgeom_amd.h section 11): the reference's DepthMap::wrapDepth, merge
and filterNoise -- what its mapping loop does to a key frame's map between refinements and when the key frame changes.  Thin
torch wrapper over a vg_depth_fusion handle; library errors raise capi.VisgeomError, argument errors ValueError before the
library is called."""
import ctypes

import numpy as np

from . import capi
from ._handle import Handle, _is_cuda, _vec

_dp = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)
WARP_COUNTS = ("sources", "drop_reconstruct", "drop_project", "outside", "lost", "written")
MERGE_COUNTS = ("skipped", "copied", "fused", "replaced", "kept")
FILTER_COUNTS = ("examined", "cleared", "smoothed")


def pose_inverse(xi):
    """Transformation::inverse of [t, rotvec], with the library's arithmetic"""
    a, out = _vec(xi, 6, "xi"), np.zeros(6)
    capi.check(capi.load().vg_transform_inverse(a.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
    return out


def pose_in_frame(base, xi):
    """Transformation::inverseCompose: the pose xi re-expressed in the frame `base` (both given in one common frame)"""
    a, b, out = _vec(base, 6, "base"), _vec(xi, 6, "xi"), np.zeros(6)
    capi.check(capi.load().vg_transform_inverse_compose(a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
    return out


class DepthFusion(Handle):
    """A vg_depth_fusion handle on one device, for the maps of one EUCM camera and one ScaleParameters (`params`: a
    vg_stereo_params or vg_motion_stereo_params; only the scale fields are read).  Maps are (depth, sigma, cost) float64 CUDA
    tensors, one [y_max, x_max] map or a batch [n, y_max, x_max].  The handle's stream is torch's current stream of the device
    at creation; each call first makes it wait for the caller's current stream and is complete when it returns.  The counters
    of the last call are left in self.counts (int64 [n, 6], [n, 5] or [n, 3]: WARP_COUNTS, MERGE_COUNTS, FILTER_COUNTS)."""

    _destroy = "vg_depth_fusion_destroy"

    def __init__(self, eucm, params, device=0):
        import torch

        self._c = _vec(eucm, 6, "eucm")
        self.device = torch.device("cuda", device)
        self.params = params.stereo if isinstance(params, capi.MotionStereoParams) else params
        if not isinstance(self.params, capi.StereoParams):
            raise ValueError("params must be a vg_stereo_params or a vg_motion_stereo_params")
        self.counts = None
        L = capi.load()
        self._open(L.vg_depth_fusion_create, self._c.ctypes.data_as(_dp), ctypes.byref(self.params))
        xm, ym = ctypes.c_int(), ctypes.c_int()
        capi.check(L.vg_depth_fusion_size(self._h, ctypes.byref(xm), ctypes.byref(ym)))
        self.x_max, self.y_max = xm.value, ym.value

    def _maps(self, maps, k, what, contiguous=False):
        """k tensors as [n, y_max, x_max]: (list, single).  contiguous: refuse instead of copying (arrays written in place)"""
        import torch

        if len(maps) < k:
            raise ValueError("%s must be (%s)" % (what, ", ".join(("depth", "sigma", "cost")[:k])))
        out, single = [], None
        for t in list(maps)[:k]:
            if not _is_cuda(t, torch.float64):
                raise ValueError("%s must be float64 CUDA tensors" % what)
            one = t.dim() == 2
            if single is not None and one != single:
                raise ValueError("%s: the maps differ in shape" % what)
            single = one
            t = t[None] if one else t
            if t.dim() != 3 or tuple(t.shape[1:]) != (self.y_max, self.x_max):
                raise ValueError("%s must be [y_max, x_max] or [n, y_max, x_max] = [%d, %d]" % (what, self.y_max, self.x_max))
            if out and t.shape[0] != out[0].shape[0]:
                raise ValueError("%s: the maps differ in shape" % what)
            if contiguous and not t.is_contiguous():
                raise ValueError("%s must be contiguous (it is written in place)" % what)
            out.append(t.contiguous())
        return out, single

    def warp(self, xi12, maps):
        """DepthMap::wrapDepth: the (depth, sigma, cost) maps carried into the frame xi12 ([6] or [n, 6], [t, rotvec] of the new
        key frame in the old one), as a new triple"""
        import torch

        src, single = self._maps(maps, 3, "maps")
        n = src[0].shape[0]
        xi = np.ascontiguousarray(xi12, dtype=np.float64).reshape(-1, 6)
        if xi.shape[0] != n:
            raise ValueError("%d maps but %d transformations" % (n, xi.shape[0]))
        if not np.isfinite(xi).all():
            raise ValueError("the transformations must be finite")
        res = [torch.empty_like(src[0]) for _ in range(3)]
        counts = np.zeros((n, 6), dtype=np.int64)
        self._enter()
        capi.check(capi.load().vg_depth_warp(self._h, n, xi.ctypes.data_as(_dp), *[t.data_ptr() for t in src],
                                             *[t.data_ptr() for t in res], counts.ctypes.data_as(_i64p)))
        self._leave(*res, *src)
        self.counts = counts
        return tuple(t[0] for t in res) if single else tuple(res)

    def merge(self, maps, maps2):
        """DepthMap::merge of maps2 into maps, in place on maps' depth and sigma (contiguous); returns maps"""
        a, single = self._maps(maps, 2, "maps", contiguous=True)
        b, single2 = self._maps(maps2, 2, "maps2")
        if single != single2 or a[0].shape != b[0].shape:
            raise ValueError("maps and maps2 differ in shape")
        n = a[0].shape[0]
        counts = np.zeros((n, 5), dtype=np.int64)
        self._enter()
        capi.check(capi.load().vg_depth_merge(self._h, n, a[0].data_ptr(), a[1].data_ptr(), b[0].data_ptr(), b[1].data_ptr(),
                                              counts.ctypes.data_as(_i64p)))
        self._leave(*a, *b)
        self.counts = counts
        return maps

    def _planes(self, maps, k, hypotheses, what):
        """k float64 CUDA tensors [hypotheses, y_max, x_max] or [n, hypotheses, y_max, x_max], contiguous: (list, n, single)"""
        import torch

        hyp = int(hypotheses)
        if len(maps) < k:
            raise ValueError("%s must be (%s)" % (what, ", ".join(("depth", "sigma", "cost")[:k])))
        out = list(maps)[:k]
        tail = (hyp, self.y_max, self.x_max)
        for t in out:
            if not _is_cuda(t, torch.float64) or t.dim() not in (3, 4) or tuple(t.shape[-3:]) != tail or t.shape != out[0].shape:
                raise ValueError("%s must be float64 CUDA tensors [n, %d, %d, %d] or [%d, %d, %d]" % ((what,) + tail + tail))
            if not t.is_contiguous():
                raise ValueError("%s must be contiguous" % what)
        single = out[0].dim() == 3
        return out, 1 if single else out[0].shape[0], single

    def regularize(self, maps, hypotheses):
        """DepthMap::regularize of (depth, sigma, cost) with `hypotheses` planes each, in place: every pixel's filled planes move
        down over its empty ones; returns maps"""
        m, n, _ = self._planes(maps, 3, hypotheses, "maps")
        self._enter()
        capi.check(capi.load().vg_depth_regularize(self._h, n, int(hypotheses), *[t.data_ptr() for t in m]))
        self._leave(*m)
        return maps

    def pack_mh(self, maps, hypotheses):
        """DepthMap::reconstruct(ALL_HYPOTHESES | SIGMA_VALUE) of one map (depth, sigma) [hypotheses, y_max, x_max]: (indices int32
        [m], hyp int32 [m], cloud float64 [m, 3], sigma float64 [m]) -- per pixel with a depth in plane 0, in raster order, one
        entry per filled plane"""
        import torch

        m, _, single = self._planes(maps, 2, hypotheses, "maps")
        if not single:
            raise ValueError("maps must be one map [hypotheses, y_max, x_max]")
        L, k, cnt = capi.load(), int(hypotheses), ctypes.c_int64()
        self._enter()
        capi.check(L.vg_depth_pack_mh(self._h, k, m[0].data_ptr(), m[1].data_ptr(), ctypes.byref(cnt), None, None, None, None))
        idx, hyp = (torch.empty(cnt.value, dtype=torch.int32, device=self.device) for _ in range(2))
        cloud = torch.empty((cnt.value, 3), dtype=torch.float64, device=self.device)
        sig = torch.empty(cnt.value, dtype=torch.float64, device=self.device)
        if cnt.value:
            self._enter()
            capi.check(L.vg_depth_pack_mh(self._h, k, m[0].data_ptr(), m[1].data_ptr(), ctypes.byref(cnt), idx.data_ptr(), hyp.data_ptr(),
                                          cloud.data_ptr(), sig.data_ptr()))
        self._leave(idx, hyp, cloud, sig, *m)
        return idx, hyp, cloud, sig

    def filter_noise(self, maps, out=None):
        """DepthMap::filterNoise of (depth, sigma, ...): the filtered (depth, sigma) as new tensors, or written into out =
        (depth, sigma), which may be the inputs themselves.  A cost map given with maps is passed through untouched."""
        import torch

        src, single = self._maps(maps, 2, "maps")
        n = src[0].shape[0]
        if out is None:
            res = [torch.empty_like(src[0]) for _ in range(2)]
        else:
            res, single_out = self._maps(out, 2, "out", contiguous=True)
            if single_out != single or res[0].shape != src[0].shape:
                raise ValueError("out and maps differ in shape")
        counts = np.zeros((n, 3), dtype=np.int64)
        self._enter()
        capi.check(capi.load().vg_depth_filter_noise(self._h, n, src[0].data_ptr(), src[1].data_ptr(), res[0].data_ptr(),
                                                     res[1].data_ptr(), counts.ctypes.data_as(_i64p)))
        self._leave(*res, *src)
        self.counts = counts
        got = tuple(t[0] for t in res) if single else tuple(res)
        return got + tuple(maps[2:]) if out is None else tuple(out)
