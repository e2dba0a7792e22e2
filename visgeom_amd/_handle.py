"""What the torch wrappers share.  All ten (stereo, motion_stereo, depth_fusion, photometric, sparse_odom, render, mono_odom,
mapping, trajectory, dense_ba): the life of a library handle and its stream, and the argument checks; a new pipeline's wrapper derives from Handle.
The two frame loops built on the pipelines (mono_odom, mapping) derive from LoopHandle, which adds what a vg_mono_odom and a
vg_mapping handle have in common."""
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


def _grid_size(p):
    """(x_max, y_max) of a vg_stereo_params as the library's creates compute it: setEqualMargin under equal_margins"""
    return ((p.u_max - 2 * p.u0) // p.scale + 1, (p.v_max - 2 * p.v0) // p.scale + 1) if p.equal_margins else (p.x_max, p.y_max)


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


_dp = ctypes.POINTER(ctypes.c_double)


def _pose(xi, what):
    a = _vec(xi, 6, what)
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite" % what)
    return a


def _xi_base_camera(root):
    """the pose [6] of the JSON object's "xi_base_camera", a transform literal"""
    values = np.ascontiguousarray(root["xi_base_camera"], dtype=np.float64).ravel()
    xbc = np.zeros(6)
    capi.check(capi.load().vg_transform_from_values(values.size, values.ctypes.data_as(_dp), xbc.ctypes.data_as(_dp)))
    return xbc


def _set_pipelines(p, motion, sparse):
    """the motion= / sparse= part of a frame loop's make_params: p with p.motion and p.sparse replaced where given"""
    if motion is not None:
        if not isinstance(motion, capi.MotionStereoParams):
            raise ValueError("motion must be a vg_motion_stereo_params")
        p.motion = motion
    if sparse is not None:
        if not isinstance(sparse, capi.SparseOdomParams):
            raise ValueError("sparse must be a vg_sparse_odom_params")
        p.sparse = sparse
    return p


class LoopHandle(Handle):
    """What MonoOdometry and PhotometricMapping share: a handle made from one EUCM camera, xi_base_cam and the loop's
    parameters, whose image size is u_max x v_max of params.motion.stereo; the checks of its arguments, the frame feed and the
    getters.  The subclass names its parameter type and the library's vg_<name>_ prefix."""

    _params = None   # the ctypes type of the parameters
    _prefix = None   # "vg_<name>_"

    def __init__(self, eucm, xi_base_cam, params=None, device=0):
        import torch

        self._c = _vec(eucm, 6, "eucm")
        self._xbc = _pose(xi_base_cam, "xi_base_cam")
        self.device = torch.device("cuda", device)
        if params is None:
            params = self._params()
            self._fn("params_default")(ctypes.byref(params))
        self.params = params
        if not isinstance(self.params, self._params):
            raise ValueError("params must be a %sparams (make_params())" % self._prefix)
        sp = self.params.motion.stereo
        self.width, self.height = sp.u_max, sp.v_max
        self._open(self._fn("create"), self._c.ctypes.data_as(_dp), self._xbc.ctypes.data_as(_dp), self.width, self.height,
                   ctypes.byref(self.params))
        size = [ctypes.c_int() for _ in range(4)]
        capi.check(self._fn("size")(self._h, *[ctypes.byref(v) for v in size]))
        self.x_max, self.y_max = size[2].value, size[3].value

    def _fn(self, name):
        return getattr(capi.load(), self._prefix + name)

    def _image(self, img, what="img"):
        img, single = _u8_images(img, self.height, self.width, what)
        if not single:
            raise ValueError("%s must be one image [height, width]" % what)
        return img

    def _depth(self, depth):
        """a depth argument [y_max, x_max], contiguous, or None"""
        import torch

        if depth is None:
            return None
        if not _is_cuda(depth, torch.float64) or tuple(depth.shape) != (self.y_max, self.x_max):
            raise ValueError("depth must be a float64 CUDA tensor [y_max, x_max] = [%d, %d]" % (self.y_max, self.x_max))
        return depth.contiguous()

    def _feed_image(self, img, samples, report_len):
        """vg_<name>_feed_image: the frame's report array [report_len]"""
        img = self._image(img)
        s = None
        if samples is not None:
            s = np.ascontiguousarray(samples, dtype=np.int32)
            sp = self.params.sparse
            if s.shape != (sp.ransac_iterations, sp.num_ransac_points):
                raise ValueError("samples must be [%d, %d]" % (sp.ransac_iterations, sp.num_ransac_points))
        rep = np.zeros(report_len)
        self._enter()
        capi.check(self._fn("feed_image")(self._h, img.data_ptr(), s.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if s is not None else None,
                                          rep.ctypes.data_as(_dp)))
        self._leave(img)
        return rep

    def _get6(self, name):
        out = np.zeros(6)
        capi.check(self._fn(name)(self._h, out.ctypes.data_as(_dp)))
        return out

    def _geti(self, name):
        v = ctypes.c_int()
        capi.check(self._fn(name)(self._h, ctypes.byref(v)))
        return v.value

    @property
    def map(self):
        """a copy of the current map (of the key frame / the inter frame): (depth, sigma, cost) float64 CUDA tensors [y_max, x_max]"""
        import torch

        out = [torch.empty((self.y_max, self.x_max), dtype=torch.float64, device=self.device) for _ in range(3)]
        self._enter()
        capi.check(self._fn("get_map")(self._h, *[t.data_ptr() for t in out]))
        return self._leave(*out)
