"""What the torch wrappers of the image pipelines share (stereo, motion_stereo, depth_fusion, photometric, sparse_odom): the
life of a library handle and its stream, and the argument checks.  A new pipeline's wrapper derives from Handle."""
import ctypes

import numpy as np

from . import capi


def _vec(a, n, what):
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    if a.size != n:
        raise ValueError("%s must have %d values" % (what, n))
    return a


def _is_cuda(t, dtype):
    import torch

    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype


def _u8_images(img, height, width, what):
    """(batch, single): img as a contiguous uint8 CUDA batch [n, height, width]; single: it was one [height, width] image"""
    import torch

    if not _is_cuda(img, torch.uint8) or img.dim() not in (2, 3) or tuple(img.shape[-2:]) != (height, width):
        raise ValueError("%s must be a uint8 CUDA tensor [n, %d, %d] or [%d, %d]" % (what, height, width, height, width))
    single = img.dim() == 2
    return (img[None] if single else img).contiguous(), single


def _f64_cuda(t, shape_tail, what):
    """t as a contiguous float64 CUDA tensor [n, *shape_tail]"""
    import torch

    shape_tail = tuple(shape_tail)
    if not _is_cuda(t, torch.float64) or t.dim() != len(shape_tail) + 1 or tuple(t.shape[1:]) != shape_tail:
        raise ValueError("%s must be a float64 CUDA tensor [n%s]" % (what, "".join(", %d" % d for d in shape_tail)))
    return t.contiguous()


class Handle:
    """A library handle on self.device (set by the subclass before _open).  The handle's stream is torch's current stream of
    the device when the handle is opened, and every library call runs on it and is complete when it returns.  Around a call:
    _enter() makes that stream wait for the caller's current stream, where the inputs were produced and the outputs are
    allocated; _leave(*tensors) tells the allocator of a tensor's use on the handle's stream."""

    _destroy = None   # name of the library's destroy function

    def _open(self, create_fn, *args):
        """create_fn(&handle, device index, stream, *args)"""
        import torch

        self._stream = torch.cuda.current_stream(self.device)
        h = ctypes.c_void_p()
        capi.check(create_fn(ctypes.byref(h), self.device.index, ctypes.c_void_p(self._stream.cuda_stream), *args))
        self._h = h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            getattr(capi.load(), self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _enter(self):
        import torch

        cur = torch.cuda.current_stream(self.device)
        if cur != self._stream:
            self._stream.wait_stream(cur)

    def _leave(self, *tensors):
        import torch

        if torch.cuda.current_stream(self.device) != self._stream:
            for t in tensors:
                if t is not None:
                    t.record_stream(self._stream)
        return tensors[0] if len(tensors) == 1 else tensors
