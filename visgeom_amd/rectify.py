"""Fisheye rectification on the GPU (include/visgeom_amd.h section 7): the pinhole -> camera undistortion maps of a calibrated
EUCM / UCM / Mei / Kannala-Brandt / double-sphere camera (the reference's `rectify` program) and a batched bilinear remap of images through them.  Thin torch
wrappers: both run on torch's current stream of the tensors' device; library errors raise capi.VisgeomError."""
import ctypes

import numpy as np

from . import capi

_dp = ctypes.POINTER(ctypes.c_double)


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _model(model):
    m = capi.MODELS[model] if isinstance(model, str) else int(model)
    if m not in capi.NUM_INTRINSICS:
        raise ValueError("unknown camera model %r" % (model,))
    return m


def rectify_maps(model, intrinsics, pinhole, xi, device=0):
    """initRemap (rectify.cpp:27-58): pinhole = [width, height, u0, v0, f], xi = the pinhole -> camera transform [t, rotvec].
    Returns (map_x, map_y), float32 CUDA tensors [height, width]; a pixel the camera cannot see maps to (-1, -1)."""
    import torch

    m = _model(model)
    intr, ph, x = _c(intrinsics).ravel(), _c(pinhole).ravel(), _c(xi).ravel()
    if intr.size != capi.NUM_INTRINSICS[m]:
        raise ValueError("wrong number of intrinsics")
    if ph.size != 5 or x.size != 6:
        raise ValueError("pinhole is [width, height, u0, v0, f] and xi a 6-vector")
    w, h = int(ph[0]), int(ph[1])
    if w != ph[0] or h != ph[1] or w < 1 or h < 1:
        raise ValueError("pinhole width and height must be positive integers")
    dev = torch.device("cuda", device)
    map_x = torch.empty((h, w), dtype=torch.float32, device=dev)
    map_y = torch.empty((h, w), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L = capi.load()
    capi.check(L.vg_rectify_map(dev.index, ctypes.c_void_p(stream), m, _ptr(intr), _ptr(ph), _ptr(x),
                                ctypes.c_void_p(map_x.data_ptr()), ctypes.c_void_p(map_y.data_ptr())))
    return map_x, map_y


def remap(images, map_x, map_y, fill=0):
    """cv::remap(INTER_LINEAR, BORDER_CONSTANT) of uint8 / float32 CUDA images [H, W], [N, H, W] or [N, H, W, C] (C = 1, 3, 4)
    through one float32 map pair [h, w], all images in one launch.  Returns a tensor of the input's dtype, shaped like the
    input with (H, W) replaced by (h, w)."""
    import torch

    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise ValueError("images must be a CUDA tensor")
    if images.dtype == torch.uint8:
        ptype = capi.PIXEL_U8
    elif images.dtype == torch.float32:
        ptype = capi.PIXEL_F32
    else:
        raise ValueError("images must be uint8 or float32")
    if not images.is_contiguous():
        raise ValueError("images must be contiguous")
    for t in (map_x, map_y):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError("map_x / map_y must be contiguous float32 tensors [h, w]")
        if t.device != images.device:
            raise ValueError("maps and images must be on the same device")
    if map_x.shape != map_y.shape:
        raise ValueError("map_x and map_y differ in shape")
    if images.dim() == 2:
        n, sh, sw, c = 1, images.shape[0], images.shape[1], 1
    elif images.dim() == 3:
        n, sh, sw, c = images.shape[0], images.shape[1], images.shape[2], 1
    elif images.dim() == 4:
        n, sh, sw, c = images.shape
    else:
        raise ValueError("images must be [H, W], [N, H, W] or [N, H, W, C]")
    mh, mw = map_x.shape
    out_shape = {2: (mh, mw), 3: (n, mh, mw), 4: (n, mh, mw, c)}[images.dim()]
    out = torch.empty(out_shape, dtype=images.dtype, device=images.device)
    stream = torch.cuda.current_stream(images.device).cuda_stream
    L = capi.load()
    capi.check(L.vg_remap(images.device.index, ctypes.c_void_p(stream), ptype, int(c), int(n), int(sw), int(sh),
                          ctypes.c_void_p(images.data_ptr()), int(mw), int(mh), ctypes.c_void_p(map_x.data_ptr()),
                          ctypes.c_void_p(map_y.data_ptr()), float(fill), ctypes.c_void_p(out.data_ptr())))
    return out
