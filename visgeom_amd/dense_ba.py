"""Photometric bundle adjustment on the GPU (include/visgeom_amd.h section 18): the reference's dense_ba_test -- the poses of up
to eight further frames and the depth of every selected key-frame cell refined together on the grey difference, with a gradient
selection, a depth prior from the depth map's own sigma and a grey sigma.  The depth block of the
normal equations is eliminated on the GPU, the 6 F pose system is solved on the host under the trust-region rule of
Photometric.compute_pose.  Thin torch wrapper over a vg_dense_ba handle; library errors raise capi.VisgeomError, argument errors
ValueError before the library is called."""
import ctypes

import numpy as np

from . import capi
from ._handle import Handle, _grid_size, _is_cuda, _u8_images, _vec

_dp = ctypes.POINTER(ctypes.c_double)
REPORT = ("iterations", "initial_cost", "final_cost", "termination")
TAIL = ("sum_d_dx2", "g_dx", "dx2", "x2", "g_max")


def make_options(sigma_grey=None, prior_weight=None, grad_thresh=None, max_iterations=None, function_tolerance=None):
    """a vg_dense_ba_options; None: the default (capi.DENSE_BA_DEFAULTS).  prior_weight=0 and grad_thresh=0 switch the prior and
    the selection off (the reference's dense_ba_test: sigma_grey=255, prior_weight=0, grad_thresh=0)."""
    o = capi.DenseBaOptions()
    for name, v in (("sigma_grey", sigma_grey), ("max_iterations", max_iterations), ("function_tolerance", function_tolerance)):
        if v is not None:
            if not v > 0:
                raise ValueError("%s must be positive" % name)
            setattr(o, name, v)
    for name, v in (("prior_weight", prior_weight), ("grad_thresh", grad_thresh)):
        if v is not None:
            if not v >= 0:
                raise ValueError("%s must not be negative" % name)
            setattr(o, name, v if v > 0 else capi.DENSE_BA_NONE)
    return o


class DenseBA(Handle):
    """A vg_dense_ba handle on one device: one EUCM camera, the depth map geometry of `params` (a vg_stereo_params or
    vg_motion_stereo_params; only the scale fields are read), xi_base_cam and the image size.  Images are uint8 CUDA tensors
    [height, width] (frames: [F, height, width], F <= 8), the maps float64 CUDA tensors [y_max, x_max]."""

    _destroy = "vg_dense_ba_destroy"

    def __init__(self, eucm, params, xi_base_cam, width, height, options=None, device=0):
        import torch

        self._c = _vec(eucm, 6, "eucm")
        self._xbc = _vec(xi_base_cam, 6, "xi_base_cam")
        self.device = torch.device("cuda", device)
        self.params = params.stereo if isinstance(params, capi.MotionStereoParams) else params
        if not isinstance(self.params, capi.StereoParams):
            raise ValueError("params must be a vg_stereo_params or a vg_motion_stereo_params")
        if options is not None and not isinstance(options, capi.DenseBaOptions):
            raise ValueError("options must be a vg_dense_ba_options (make_options())")
        self.options = options
        self.width, self.height = int(width), int(height)
        self.x_max, self.y_max = _grid_size(self.params)
        self.frames = 0
        self._open(capi.load().vg_dense_ba_create, self._c.ctypes.data_as(_dp), ctypes.byref(self.params), self._xbc.ctypes.data_as(_dp),
                   self.width, self.height, ctypes.byref(options) if options is not None else None)

    def _map(self, t, what):
        import torch

        if not _is_cuda(t, torch.float64) or tuple(t.shape) != (self.y_max, self.x_max):
            raise ValueError("%s must be a float64 CUDA tensor [y_max, x_max] = [%d, %d]" % (what, self.y_max, self.x_max))
        return t.contiguous()

    def set_base(self, img, depth, sigma=None):
        """the key frame: its image, its depth map and the depth map's sigma (needed unless the prior is off); builds the pack"""
        img, single = _u8_images(img, self.height, self.width, "img")
        if not single:
            raise ValueError("img must be [height, width]")
        depth = self._map(depth, "depth")
        sigma = self._map(sigma, "sigma") if sigma is not None else None
        self._enter()
        capi.check(capi.load().vg_dense_ba_set_base(self._h, img.data_ptr(), depth.data_ptr(), sigma.data_ptr() if sigma is not None else None))
        self._leave(img, depth, sigma)

    def set_frames(self, imgs):
        """the further frames: [F, height, width] or one [height, width]"""
        imgs, _ = _u8_images(imgs, self.height, self.width, "imgs")
        self._enter()
        capi.check(capi.load().vg_dense_ba_set_frames(self._h, imgs.shape[0], imgs.data_ptr()))
        self.frames = imgs.shape[0]
        self._leave(imgs)

    @property
    def count(self):
        m = ctypes.c_int64()
        capi.check(capi.load().vg_dense_ba_pack(self._h, ctypes.byref(m), None, None, None, None, None))
        return m.value

    def pack(self):
        """(indices int32 [m], greys [m], dirs [m, 3], d0 [m], sigma0 [m]), CUDA tensors"""
        import torch

        m = self.count
        idx = torch.empty((m,), dtype=torch.int32, device=self.device)
        out = [torch.empty(s, dtype=torch.float64, device=self.device) for s in ((m,), (m, 3), (m,), (m,))]
        self._enter()
        capi.check(capi.load().vg_dense_ba_pack(self._h, None, idx.data_ptr(), *[t.data_ptr() for t in out]))
        return self._leave(idx, *out)

    def _poses(self, xi):
        xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(-1, 6)
        if self.frames and xi.shape[0] != self.frames:
            raise ValueError("%d poses but %d frames" % (xi.shape[0], self.frames))
        return xi

    def evaluate(self, xi, depths=None, rows=True):
        """residuals and Jacobians at the poses xi [F, 6] and the depths (float64 CUDA [m]; None: the key frame's): a dict with
        cost (float), sums [F, 28] (numpy) and, with rows, residuals [F, m], jac_pose [F, m, 6], jac_depth [F, m], a [m] and
        g_depth [m] (CUDA tensors)"""
        import torch

        xi = self._poses(xi)
        F = xi.shape[0]
        out = {"residuals": None, "jac_pose": None, "jac_depth": None, "a": None, "g_depth": None}
        if depths is not None:
            if not _is_cuda(depths, torch.float64) or depths.dim() != 1:
                raise ValueError("depths must be a float64 CUDA tensor [m]")
            if depths.shape[0] != self.count:
                raise ValueError("depths must have %d values" % self.count)
            depths = depths.contiguous()
        if rows:
            m = self.count
            for k, s in (("residuals", (F, m)), ("jac_pose", (F, m, 6)), ("jac_depth", (F, m)), ("a", (m,)), ("g_depth", (m,))):
                out[k] = torch.zeros(s, dtype=torch.float64, device=self.device)
        cost, sums = ctypes.c_double(), np.zeros((F, 28))
        ptr = [out[k].data_ptr() if rows else None for k in ("residuals", "jac_pose", "jac_depth", "a", "g_depth")]
        self._enter()
        capi.check(capi.load().vg_dense_ba_evaluate(self._h, xi.ctypes.data_as(_dp), depths.data_ptr() if depths is not None else None, *ptr,
                                                    ctypes.byref(cost), sums.ctypes.data_as(_dp)))
        self._leave(depths, *out.values())
        out.update(cost=cost.value, sums=sums)
        return out

    def reduce(self, mu):
        """the reduced system of the last evaluation under the damping mu: (S [K, K], rhs [K]) numpy, K = 6 F"""
        K = 6 * self.frames
        S, rhs = np.zeros((K, K)), np.zeros(K)
        self._enter()
        capi.check(capi.load().vg_dense_ba_reduce(self._h, float(mu), S.ctypes.data_as(_dp), rhs.ctypes.data_as(_dp)))
        return S, rhs

    def back_substitute(self, mu, dp):
        """the depth step of the pose step dp [K] under mu: (candidate depths CUDA [m], tail [5] numpy: TAIL)"""
        import torch

        dp = _vec(dp, 6 * self.frames, "dp")
        cand = torch.empty((self.count,), dtype=torch.float64, device=self.device)
        tail = np.zeros(capi.DENSE_BA_TAIL)
        self._enter()
        capi.check(capi.load().vg_dense_ba_back_substitute(self._h, float(mu), dp.ctypes.data_as(_dp), cand.data_ptr(), tail.ctypes.data_as(_dp)))
        return self._leave(cand), tail

    def solve(self, xi_start):
        """the solve from the start poses [F, 6]: (poses [F, 6] numpy, depth map, sigma map (CUDA [y_max, x_max]), report [4]
        numpy: REPORT)"""
        import torch

        xi = self._poses(xi_start)
        out, report = np.zeros_like(xi), np.zeros(4)
        depth, sigma = (torch.empty((self.y_max, self.x_max), dtype=torch.float64, device=self.device) for _ in range(2))
        self._enter()
        capi.check(capi.load().vg_dense_ba_solve(self._h, xi.ctypes.data_as(_dp), out.ctypes.data_as(_dp), depth.data_ptr(), sigma.data_ptr(),
                                                 report.ctypes.data_as(_dp)))
        self._leave(depth, sigma)
        return out, depth, sigma, report
