"""Depth map propagation and fusion on the GPU (include/visgeom_amd.h section 11): the reference's DepthMap::wrapDepth, merge
and filterNoise -- what its mapping loop does to a key frame's map between refinements and when the key frame changes -- and
the map's two ends: DepthMap::reconstruct (the map as a point cloud), generatePlane (a plane as a prior map) and the accuracy
score of the reference's stereo_test against ground truth.  Thin
torch wrapper over a vg_depth_fusion handle; library errors raise capi.VisgeomError, argument errors ValueError before the
library is called."""
import collections
import ctypes

import numpy as np

from . import capi
from ._handle import Handle, _is_cuda, _vec

_dp = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)
WARP_COUNTS = ("sources", "drop_reconstruct", "drop_project", "outside", "lost", "written")
MERGE_COUNTS = ("skipped", "copied", "fused", "replaced", "kept")
FILTER_COUNTS = ("examined", "cleared", "smoothed")
COMPARE_COUNTS = ("ground_truth", "scored", "inliers")   # the reference's Ngt, Nmax, N
COMPARE_SUMS = ("err", "err2", "dist")
Cloud = collections.namedtuple("Cloud", "indices hyp points sigma index_map item valid cloud counts")


def _ratio(a, b):
    """a / b as the reference's double division leaves it for counts: NaN where the denominator is 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b == 0, np.nan, a / np.where(b == 0, 1., b))


class Accuracy:
    """What analyzeError accumulates and prints: counts int64 [3] or [n, 3] (COMPARE_COUNTS), sums float64 (COMPARE_SUMS), the
    inlier mask (uint8 CUDA, 0 / 255) and the reference's figures, NaN where a denominator is 0"""

    def __init__(self, counts, sums, inliers):
        self.counts, self.sums, self.inliers = counts, sums, inliers
        ngt, nmax, n = (counts[..., i] for i in range(3))
        err, err2, dist = (sums[..., i] for i in range(3))
        self.mean_error_mm = _ratio(err, n) * 1000           # err / N * 1000
        self.rms_error_mm = np.sqrt(_ratio(err2, n)) * 1000  # sqrt(err2 / N) * 1000
        self.inlier_percent = 100 * _ratio(n, nmax)          # 100 N / Nmax
        self.mean_distance = _ratio(dist, nmax)              # dist / Nmax
        self.coverage = _ratio(n, ngt)                       # N / Ngt

    def __repr__(self):
        return "Accuracy(counts=%s, rms_error_mm=%s, inlier_percent=%s, mean_distance=%s, coverage=%s)" % (
            np.asarray(self.counts).tolist(), self.rms_error_mm, self.inlier_percent, self.mean_distance, self.coverage)


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

    def reconstruct(self, maps, flags=0, hypotheses=1, query_points=None, query_indices=None, poses=None):
        """DepthMap::reconstruct(pack, flags) of maps = (depth, sigma) or (depth,), [hypotheses, y_max, x_max] each or a batch [n,
        hypotheses, y_max, x_max] (a plain [y_max, x_max] map is one plane): a Cloud of tensors, entries in the reference's order
        (item after item, query order, h ascending).  flags: capi.RECON_*; query_points float64 [q, 2] / query_indices int32 [q]
        CUDA tensors go with their flag; poses ([6] or [n, 6]) move item k's points by Transformation::transform.  Fields that
        the flags do not produce (sigma, index_map) are None."""
        import torch

        flags, hyp = int(flags), int(hypotheses)
        if flags & capi.RECON_IMAGE_VALUES:
            raise ValueError("IMAGE_VALUES is not provided")
        if flags & ~capi.RECON_KNOWN or flags < 0:
            raise ValueError("unknown reconstruct flags")
        if not 1 <= hyp <= 8:
            raise ValueError("hypotheses must be in [1, 8]")
        maps = tuple(maps)
        if not maps:
            raise ValueError("maps must be (depth, sigma) or (depth,)")
        if hyp == 1 and maps and hasattr(maps[0], "dim") and maps[0].dim() == 2:
            maps = tuple(t[None] for t in maps)
        need_sigma = bool(flags & (capi.RECON_SIGMA_VALUE | capi.RECON_MINMAX))
        if need_sigma and len(maps) < 2:
            raise ValueError("SIGMA_VALUE and MINMAX need maps = (depth, sigma)")
        m, n, _ = self._planes(maps, min(len(maps), 2), hyp, "maps")
        by_index, by_point = bool(flags & capi.RECON_QUERY_INDICES), bool(flags & capi.RECON_QUERY_POINTS)
        query, nq = None, 0
        if by_index:
            query = query_indices
            if not _is_cuda(query, torch.int32) or query.dim() != 1 or not query.is_contiguous():
                raise ValueError("QUERY_INDICES needs query_indices, a contiguous int32 CUDA tensor [q]")
        elif by_point:
            query = query_points
            if not _is_cuda(query, torch.float64) or query.dim() != 2 or query.shape[1] != 2 or not query.is_contiguous():
                raise ValueError("QUERY_POINTS needs query_points, a contiguous float64 CUDA tensor [q, 2]")
        elif query_points is not None or query_indices is not None:
            raise ValueError("a query needs its flag: QUERY_POINTS or QUERY_INDICES")
        if query is not None:
            nq = query.shape[0]
        if flags & capi.RECON_INDEX_MAPPING and query is None:
            raise ValueError("INDEX_MAPPING needs a query")
        xi = None
        if poses is not None:
            xi = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 6)
            if xi.shape[0] != n:
                raise ValueError("%d maps but %d poses" % (n, xi.shape[0]))
            if not np.isfinite(xi).all():
                raise ValueError("the poses must be finite")
        units, planes = (nq if query is not None else self.x_max * self.y_max), (hyp if flags & capi.RECON_ALL_HYPOTHESES else 1)
        if n * units * planes >= 1 << 31:
            raise ValueError("the entries could reach 2^31: fewer items or queries per call")
        L, counts = capi.load(), np.zeros(n, dtype=np.int64)
        args = (self._h, n, hyp, flags, m[0].data_ptr(), m[1].data_ptr() if len(m) > 1 else None, nq,
                query.data_ptr() if by_point and not by_index else None, query.data_ptr() if by_index else None,
                xi.ctypes.data_as(_dp) if xi is not None else None, counts.ctypes.data_as(_i64p))
        self._enter()
        capi.check(L.vg_depth_reconstruct(*args, None))
        total = int(counts.sum())

        def new(dtype, *tail):
            return torch.empty((total,) + tail, dtype=dtype, device=self.device)

        res = dict(indices=new(torch.int32), hyp=new(torch.int32), points=new(torch.float64, 2),
                   sigma=new(torch.float64) if flags & capi.RECON_SIGMA_VALUE else None,
                   index_map=new(torch.int32) if flags & capi.RECON_INDEX_MAPPING else None, item=new(torch.int32),
                   valid=new(torch.uint8), cloud=new(torch.float64, 2, 3) if flags & capi.RECON_MINMAX else new(torch.float64, 3))
        if total:
            out = capi.ReconOutputs(*[res[k].data_ptr() if res[k] is not None else None
                                      for k in ("indices", "hyp", "points", "sigma", "index_map", "item", "valid", "cloud")])
            self._enter()
            capi.check(L.vg_depth_reconstruct(*args, ctypes.byref(out)))
        self._leave(*[t for t in res.values() if t is not None], *m, *([query] if query is not None else []))
        self.counts = counts
        return Cloud(counts=counts, **res)

    def generate_plane(self, xi_cam_plane, polygon):
        """DepthMap::generatePlane: (depth, sigma, cost) [y_max, x_max] of the plane z = 0 of the frame xi_cam_plane ([t, rotvec] of
        the plane's frame in the camera's) inside the polygon ([k, 3] in the plane's frame, 3 <= k <= 16)"""
        import torch

        xi = _vec(xi_cam_plane, 6, "xi_cam_plane")
        poly = np.ascontiguousarray(polygon, dtype=np.float64)
        if poly.ndim != 2 or poly.shape[1] != 3 or not 3 <= poly.shape[0] <= capi.RECON_MAX_POLYGON:
            raise ValueError("polygon must be [k, 3] with 3 <= k <= 16")
        if not np.isfinite(xi).all() or not np.isfinite(poly).all():
            raise ValueError("the pose and the polygon must be finite")
        res = [torch.empty((self.y_max, self.x_max), dtype=torch.float64, device=self.device) for _ in range(3)]
        self._enter()
        capi.check(capi.load().vg_depth_generate_plane(self._h, xi.ctypes.data_as(_dp), poly.shape[0], poly.ctypes.data_as(_dp),
                                                       *[t.data_ptr() for t in res]))
        self._leave(*res)
        return tuple(res)

    def compare(self, maps, truth, sigma_max=10.):
        """analyzeError of the reference's stereo_test: maps = (depth, sigma) against truth, the renderer's depth buffer (float32
        CUDA [v_max, u_max] or [n, v_max, u_max]): an Accuracy with counts, sums, the inlier mask and the five figures"""
        import torch

        src, single = self._maps(maps, 2, "maps")
        n = src[0].shape[0]
        if not _is_cuda(truth, torch.float32) or truth.dim() != (2 if single else 3):
            raise ValueError("truth must be a float32 CUDA tensor [v_max, u_max] or [n, v_max, u_max], like the maps")
        t = (truth[None] if single else truth).contiguous()
        p = self.params
        if tuple(t.shape) != (n, p.v_max, p.u_max):
            raise ValueError("truth must be [%d, %d, %d]" % (n, p.v_max, p.u_max))
        if p.u0 < 0 or p.v0 < 0 or (self.x_max - 1) * p.scale + p.u0 >= p.u_max or (self.y_max - 1) * p.scale + p.v0 >= p.v_max:
            raise ValueError("the depth grid leaves the image: no truth to compare with")
        if sigma_max != sigma_max:
            raise ValueError("sigma_max is NaN")
        counts, sums = np.zeros((n, 3), dtype=np.int64), np.zeros((n, 3))
        inl = torch.empty((n, self.y_max, self.x_max), dtype=torch.uint8, device=self.device)
        self._enter()
        capi.check(capi.load().vg_depth_compare(self._h, n, src[0].data_ptr(), src[1].data_ptr(), t.data_ptr(), float(sigma_max),
                                                counts.ctypes.data_as(_i64p), sums.ctypes.data_as(_dp), inl.data_ptr()))
        self._leave(inl, t, *src)
        self.counts = counts
        return Accuracy(counts[0] if single else counts, sums[0] if single else sums, inl[0] if single else inl)

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
