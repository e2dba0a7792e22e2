"""Conversion between camera models on the GPU (include/visgeom_amd.h section 20): pixels to unit rays for every model, the remap
maps from one camera into another (they feed rectify.remap unchanged), and a least-squares fit of a model's intrinsics to a
calibrated camera.  Thin torch wrappers: unproject and convert_maps run on torch's current stream of the device; library errors
raise capi.VisgeomError."""
import ctypes

import numpy as np

from . import capi
from .rectify import _c, _model, _ptr


def _intrinsics(m, intrinsics):
    intr = _c(intrinsics).ravel()
    if intr.size != capi.NUM_INTRINSICS[m]:
        raise ValueError("wrong number of intrinsics")
    return intr


def unproject(model, intrinsics, uv, device=0):
    """uv [n, 2] (a float64 CUDA tensor, or anything numpy takes) -> (rays [n, 3] float64, ok [n] uint8), CUDA tensors.  A pixel the
    model cannot unproject has the ray (0, 0, 0) and ok 0."""
    import torch

    m = _model(model)
    intr = _intrinsics(m, intrinsics)
    if isinstance(uv, torch.Tensor):
        if not uv.is_cuda or uv.dtype != torch.float64 or not uv.is_contiguous():
            raise ValueError("uv must be a contiguous float64 CUDA tensor")
        dev = uv.device
    else:
        dev = torch.device("cuda", device)
        uv = torch.from_numpy(_c(uv)).to(dev)
    if uv.dim() != 2 or uv.shape[1] != 2:
        raise ValueError("uv must be [n, 2]")
    n = uv.shape[0]
    rays = torch.empty((n, 3), dtype=torch.float64, device=dev)
    ok = torch.empty((n,), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = capi.load()
    capi.check(L.vg_unproject(dev.index, ctypes.c_void_p(stream), m, _ptr(intr), int(n), ctypes.c_void_p(uv.data_ptr()),
                              ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(ok.data_ptr())))
    return rays, ok


def convert_maps(dst_model, dst_intrinsics, src_model, src_intrinsics, size, rotvec=None, device=0):
    """size = (width, height) of the destination image; rotvec turns destination-frame rays into the source frame.  Returns
    (map_x, map_y), float32 CUDA tensors [height, width] like rectify.rectify_maps: rectify.remap(source_images, map_x, map_y) is
    the source camera's image seen by the destination camera; a pixel without a source maps to (-1, -1)."""
    import torch

    md, ms = _model(dst_model), _model(src_model)
    di, si = _intrinsics(md, dst_intrinsics), _intrinsics(ms, src_intrinsics)
    w, h = int(size[0]), int(size[1])
    if w != size[0] or h != size[1] or not (1 <= w <= capi.CONVERT_MAX_SIDE and 1 <= h <= capi.CONVERT_MAX_SIDE):
        raise ValueError("size is (width, height), integers in [1, 16384]")
    rot = None
    if rotvec is not None:
        rot = _c(rotvec).ravel()
        if rot.size != 3:
            raise ValueError("rotvec is a 3-vector")
    dev = torch.device("cuda", device)
    map_x = torch.empty((h, w), dtype=torch.float32, device=dev)
    map_y = torch.empty((h, w), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = capi.load()
    capi.check(L.vg_convert_map(dev.index, ctypes.c_void_p(stream), md, _ptr(di), ms, _ptr(si), None if rot is None else _ptr(rot), w, h,
                                ctypes.c_void_p(map_x.data_ptr()), ctypes.c_void_p(map_y.data_ptr())))
    return map_x, map_y


def default_start(src_model, src_intrinsics, dst_model):
    """the fit's default start: the destination model's neutral shape values at the source's paraxial focal lengths and centre"""
    ms, md = _model(src_model), _model(dst_model)
    si = _intrinsics(ms, src_intrinsics)
    out = np.empty(capi.NUM_INTRINSICS[md])
    capi.check(capi.load().vg_convert_start(ms, _ptr(si), md, _ptr(out)))
    return out


def default_options():
    o = capi.ConvertFitOptions()
    capi.load().vg_convert_fit_default_options(ctypes.byref(o))
    return o


def fit(src_model, src_intrinsics, size, dst_model, start=None, device=0, **options):
    """Fit dst_model's intrinsics to the camera (src_model, src_intrinsics) of a size = (width, height) image.  options: the fields
    of capi.ConvertFitOptions (grid_w, grid_h, max_angle, max_iterations, function_tolerance, gradient_tolerance,
    parameter_tolerance, use_bounds).  Returns (intrinsics, summary dict)."""
    import torch

    ms, md = _model(src_model), _model(dst_model)
    si = _intrinsics(ms, src_intrinsics)
    x = np.full(capi.NUM_INTRINSICS[md], np.nan) if start is None else _intrinsics(md, start).copy()
    o = default_options()
    for k, v in options.items():
        if k not in dict(capi.ConvertFitOptions._fields_):
            raise TypeError("unknown option %r" % k)
        setattr(o, k, v)
    s = capi.ConvertFitSummary()
    dev = torch.device("cuda", device)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = capi.load()
    capi.check(L.vg_convert_fit(dev.index, ctypes.c_void_p(stream), ms, _ptr(si), int(size[0]), int(size[1]), md, _ptr(x), ctypes.byref(o),
                                ctypes.byref(s)))
    summary = {k: getattr(s, k) for k, _ in capi.ConvertFitSummary._fields_}
    summary["termination"] = capi.TERMINATION[s.termination]
    return x, summary
