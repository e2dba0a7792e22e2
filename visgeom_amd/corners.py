"""Checkerboard corner detection on the GPU (include/visgeom_amd.h section 8): the reference's CornerDetector for batches of
same-size 8-bit images.  Thin torch wrappers on CUDA uint8 tensors; library errors raise capi.VisgeomError."""
import ctypes

import numpy as np

from . import capi

SIGMAS = (1.4, 2.0, 1.0)


def _images(images):
    import torch

    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise ValueError("images must be a CUDA tensor")
    if images.dtype != torch.uint8:
        raise ValueError("images must be uint8")
    if images.dim() not in (2, 3):
        raise ValueError("images must be [H, W] or [N, H, W]")
    images = images.contiguous()
    batch = images.unsqueeze(0) if images.dim() == 2 else images
    return images, batch


class CornerDetector:
    """A detector for a board of cols x rows inner corners on one device; it keeps its scratch between calls (one image size
    at a time).  Runs on torch's current stream of the device at creation."""

    def __init__(self, cols, rows, improve=False, device=0):
        import torch

        self.cols, self.rows, self.improve = int(cols), int(rows), bool(improve)
        self.device = torch.device("cuda", device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L = capi.load()
        h = ctypes.c_void_p()
        capi.check(L.vg_corner_detector_create(ctypes.byref(h), self.device.index, ctypes.c_void_p(stream), self.cols,
                                               self.rows, int(self.improve)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            capi.load().vg_corner_detector_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def detect(self, images, return_sigma=False):
        """corners float64 [N, cols rows, 2] (CPU), found bool [N] (CPU), and with return_sigma the sigma that found each
        image (0 if none); a [H, W] input gives unbatched outputs"""
        import torch

        images, batch = _images(images)
        n, h, w = batch.shape
        corners = np.zeros((n, self.cols * self.rows, 2), np.float64)
        found = np.zeros(n, np.uint8)
        sigma = np.zeros(n, np.float64)
        torch.cuda.current_stream(batch.device).synchronize()
        capi.check(capi.load().vg_corner_detect(self._h, n, w, h, ctypes.c_void_p(batch.data_ptr()),
                                                corners.ctypes.data_as(capi._dp), found.ctypes.data_as(ctypes.c_void_p),
                                                sigma.ctypes.data_as(capi._dp)))
        out = [torch.from_numpy(corners), torch.from_numpy(found.astype(bool))]
        if return_sigma:
            out.append(torch.from_numpy(sigma))
        if images.dim() == 2:
            out = [t[0] for t in out]
        return tuple(out)

    def response(self, images, sigma):
        """computeResponse(0.7, sigma): dict of CUDA tensors src1, src2 (uint8), gradx, grady, imgrad, resp (float32), each
        [N, H, W], and avg (float64 numpy [N], _avgVal)"""
        import torch

        _, batch = _images(images)
        n, h, w = batch.shape
        dev = batch.device
        out = {k: torch.empty((n, h, w), dtype=torch.uint8, device=dev) for k in ("src1", "src2")}
        out.update({k: torch.empty((n, h, w), dtype=torch.float32, device=dev) for k in ("gradx", "grady", "imgrad", "resp")})
        avg = np.zeros(n, np.float64)
        torch.cuda.current_stream(dev).synchronize()
        p = [ctypes.c_void_p(out[k].data_ptr()) for k in ("src1", "src2", "gradx", "grady", "imgrad", "resp")]
        capi.check(capi.load().vg_corner_response(self._h, n, w, h, ctypes.c_void_p(batch.data_ptr()), float(sigma), *p,
                                                  avg.ctypes.data_as(capi._dp)))
        out["avg"] = avg
        return out

    def candidates(self, images, sigma):
        """selectCandidates: per image (list of int [k, 2] arrays: the accepted candidates (u, v) in descending response),
        VAL_THRESH [N] and the number of local maxima [N]"""
        import torch

        _, batch = _images(images)
        n, h, w = batch.shape
        m = 10 * self.cols * self.rows
        uv = np.zeros((n, m, 2), np.int32)
        count = np.zeros(n, np.int32)
        thresh = np.zeros(n, np.float64)
        nmax = np.zeros(n, np.int64)
        torch.cuda.current_stream(batch.device).synchronize()
        capi.check(capi.load().vg_corner_candidates(self._h, n, w, h, ctypes.c_void_p(batch.data_ptr()), float(sigma), m,
                                                    uv.ctypes.data_as(capi._i32p), count.ctypes.data_as(capi._i32p),
                                                    thresh.ctypes.data_as(capi._dp), nmax.ctypes.data_as(capi._i64p)))
        return [uv[i, :count[i]].copy() for i in range(n)], thresh, nmax

    def stats(self):
        """accumulated timings of the detect calls (vg_corner_detector_stats)"""
        s = np.zeros(8, np.float64)
        capi.check(capi.load().vg_corner_detector_stats(self._h, s.ctypes.data_as(capi._dp)))
        keys = ("gpu_s", "d2h_s", "d2h_bytes", "graph_s", "graph_images", "refine_s", "refine_corners", "calls")
        return dict(zip(keys, s.tolist()))

    def chunk(self, width, height):
        c = ctypes.c_int()
        capi.check(capi.load().vg_corner_detector_chunk(self._h, int(width), int(height), ctypes.byref(c)))
        return c.value


def detect_pattern(images, cols, rows, improve=False):
    """CornerDetector::detectPattern on [H, W] or [N, H, W] uint8 CUDA images: (corners float64 [N, cols rows, 2],
    found bool [N]), both CPU tensors, corners in the reference's order (row by row from the corner with the smallest u + v)"""
    images, _ = _images(images)
    det = CornerDetector(cols, rows, improve, device=images.device.index)
    try:
        return det.detect(images)
    finally:
        det.close()


def circle(radius):
    """getCircle around (0, 0) as the library rasterises it: int array [n, 2] of (du, dv)"""
    du = np.zeros(256, np.int32)
    dv = np.zeros(256, np.int32)
    n = ctypes.c_int()
    capi.check(capi.load().vg_corner_circle(int(radius), 256, du.ctypes.data_as(capi._i32p), dv.ctypes.data_as(capi._i32p),
                                            ctypes.byref(n)))
    return np.stack([du[:n.value], dv[:n.value]], axis=1)
