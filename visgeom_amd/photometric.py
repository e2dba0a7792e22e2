"""Photometric pose estimation against a depth key frame on the GPU (include/visgeom_amd.h section 12): the reference's
ScalePhotometric::computePose -- a binary image pyramid with gradients, the data pack of the key frame's salient pixels with
a depth, the photometric cost with its Jacobian, and a coarse-to-fine trust-region solve; and computePoseMI, the same
localization on the mutual information of the two images' grey values, for a key frame from another pass with other exposure
and lighting: its cost with histogram and gradient, and a coarse-to-fine BFGS.  Thin torch wrapper over a
vg_photometric handle; library errors raise capi.VisgeomError, argument errors ValueError before the library is called."""
import ctypes

import numpy as np

from . import capi
from ._handle import Handle, _grid_size, _is_cuda, _u8_images, _vec

_dp = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)
REPORT = ("iterations", "initial_cost", "final_cost", "termination")


class Photometric(Handle):
    """A vg_photometric handle on one device: one EUCM camera, the depth map geometry of `params` (a vg_stereo_params or
    vg_motion_stereo_params; only the scale fields are read), xi_base_cam, the image size and num_scales pyramid levels.
    Images are uint8 CUDA tensors [height, width] (targets: [n, height, width]), the depth map a float64 CUDA tensor [y_max,
    x_max].  The handle's stream is torch's current stream of the device at creation; each call first makes it wait for the
    caller's current stream (where the inputs were produced and the outputs are allocated) and is complete when it returns."""

    _destroy = "vg_photometric_destroy"

    def __init__(self, eucm, params, xi_base_cam, width, height, num_scales=5, device=0):
        import torch

        self._c = _vec(eucm, 6, "eucm")
        self._xbc = _vec(xi_base_cam, 6, "xi_base_cam")
        self.device = torch.device("cuda", device)
        self.params = params.stereo if isinstance(params, capi.MotionStereoParams) else params
        if not isinstance(self.params, capi.StereoParams):
            raise ValueError("params must be a vg_stereo_params or a vg_motion_stereo_params")
        self.width, self.height, self.num_scales = int(width), int(height), int(num_scales)
        self.n_targets = 0
        L = capi.load()
        self._open(L.vg_photometric_create, self._c.ctypes.data_as(_dp), ctypes.byref(self.params), self._xbc.ctypes.data_as(_dp),
                   self.width, self.height, self.num_scales)
        self.sizes = []   # (width, height) per level
        for i in range(self.num_scales):
            w, hh = ctypes.c_int(), ctypes.c_int()
            capi.check(L.vg_photometric_level_size(self._h, i, ctypes.byref(w), ctypes.byref(hh)))
            self.sizes.append((w.value, hh.value))

    def set_base(self, img, depth):
        """the key frame: its image and its depth map; builds the pyramid with gradients and the data pack of every scale"""
        import torch

        img, single = _u8_images(img, self.height, self.width, "img")
        if not single:
            raise ValueError("img must be [height, width]")
        if not _is_cuda(depth, torch.float64) or depth.dim() != 2:
            raise ValueError("depth must be a float64 CUDA tensor [y_max, x_max]")
        x_max, y_max = _grid_size(self.params)
        if tuple(depth.shape) != (y_max, x_max):
            raise ValueError("depth must be [y_max, x_max] = [%d, %d]" % (y_max, x_max))
        depth = depth.contiguous()
        self._enter()
        capi.check(capi.load().vg_photometric_set_base(self._h, img.data_ptr(), depth.data_ptr()))
        self._leave(img, depth)

    def set_depth(self, depth):
        """setDepth: the key frame's image stays, its data packs are rebuilt from another depth map (float64 CUDA tensor [y_max,
        x_max]) -- the same packs as set_base(the same image, depth), without the pyramid and gradient launches.  The library
        refuses it (ERR_STATE) before a key frame exists."""
        import torch

        if not _is_cuda(depth, torch.float64) or depth.dim() != 2:
            raise ValueError("depth must be a float64 CUDA tensor [y_max, x_max]")
        x_max, y_max = _grid_size(self.params)
        if tuple(depth.shape) != (y_max, x_max):
            raise ValueError("depth must be [y_max, x_max] = [%d, %d]" % (y_max, x_max))
        depth = depth.contiguous()
        self._enter()
        capi.check(capi.load().vg_photo_set_depth(self._h, depth.data_ptr()))
        self._leave(depth)

    def set_targets(self, imgs):
        """the images the poses are estimated for: [n, height, width] or one [height, width]"""
        imgs, _ = _u8_images(imgs, self.height, self.width, "imgs")
        self._enter()
        capi.check(capi.load().vg_photometric_set_targets(self._h, imgs.shape[0], imgs.data_ptr()))
        self.n_targets = imgs.shape[0]
        self._leave(imgs)

    def level(self, scale_idx, target=None):
        """(img, grad_u, grad_v) float32 [rows, cols] of one pyramid level: the key frame's, or target image `target`'s"""
        import torch

        if not 0 <= scale_idx < self.num_scales:
            raise ValueError("scale index out of range")
        w, h = self.sizes[scale_idx]
        out = [torch.empty((h, w), dtype=torch.float32, device=self.device) for _ in range(3)]
        self._enter()
        capi.check(capi.load().vg_photometric_level(self._h, -1 if target is None else int(target), scale_idx, *[t.data_ptr() for t in out]))
        return self._leave(*out)

    def pack(self, scale_idx):
        """the data pack of a scale: (indices int32 [m], values float64 [m], cloud float64 [m, 3])"""
        import torch

        L = capi.load()
        m = ctypes.c_int64()
        capi.check(L.vg_photometric_pack(self._h, scale_idx, ctypes.byref(m), None, None, None))
        idx = torch.empty((m.value,), dtype=torch.int32, device=self.device)
        val = torch.empty((m.value,), dtype=torch.float64, device=self.device)
        cloud = torch.empty((m.value, 3), dtype=torch.float64, device=self.device)
        self._enter()
        capi.check(L.vg_photometric_pack(self._h, scale_idx, ctypes.byref(m), idx.data_ptr(), val.data_ptr(), cloud.data_ptr()))
        return self._leave(idx, val, cloud)

    def _poses(self, xi, target):
        xi = np.ascontiguousarray(xi, dtype=np.float64).reshape(-1, 6)
        tg = np.zeros(xi.shape[0], dtype=np.int32) if target is None else np.ascontiguousarray(target, dtype=np.int32).reshape(-1)
        if tg.shape[0] != xi.shape[0]:
            raise ValueError("%d poses but %d target indices" % (xi.shape[0], tg.shape[0]))
        return xi, tg

    def evaluate(self, scale_idx, xi, target=None, rows=True):
        """PhotometricCostFunction::Evaluate of the poses xi [n, 6] against target[k] (default: target 0) at one scale: a dict
        with cost [n], jtj [n, 21] (upper triangle, row-major), jtr [n, 6] (numpy) and, with rows, residuals [n, m] and
        jacobians [n, m, 6] (CUDA tensors)"""
        import torch

        xi, tg = self._poses(xi, target)
        n = xi.shape[0]
        L = capi.load()
        res = jac = None
        if rows:
            m = ctypes.c_int64()
            capi.check(L.vg_photometric_pack(self._h, scale_idx, ctypes.byref(m), None, None, None))
            res = torch.zeros((n, m.value), dtype=torch.float64, device=self.device)
            jac = torch.zeros((n, m.value, 6), dtype=torch.float64, device=self.device)
        cost, jtj, jtr = np.zeros(n), np.zeros((n, 21)), np.zeros((n, 6))
        self._enter()
        capi.check(L.vg_photometric_evaluate(self._h, scale_idx, n, xi.ctypes.data_as(_dp), tg.ctypes.data_as(_i32p),
                                             res.data_ptr() if rows else None, jac.data_ptr() if rows else None,
                                             cost.ctypes.data_as(_dp), jtj.ctypes.data_as(_dp), jtr.ctypes.data_as(_dp)))
        self._leave(res, jac)
        return {"cost": cost, "jtj": jtj, "jtr": jtr, "residuals": res, "jacobians": jac}

    def compute_pose(self, xi_start, target=None, xi_prior=None):
        """computePose from the start poses xi_start [n, 6] (or one [6]) against target[k]: (poses, report); report is
        float64 [n, num_scales, 4]: REPORT per scale.  xi_prior ([n, 6]): the motion prior's pose per start pose (the
        reference passes the start pose itself); None switches the prior off."""
        single = np.ndim(xi_start) == 1
        xi, tg = self._poses(xi_start, target)
        n = xi.shape[0]
        prior = None
        if xi_prior is not None:
            prior = np.ascontiguousarray(xi_prior, dtype=np.float64).reshape(-1, 6)
            if prior.shape[0] != n:
                raise ValueError("%d poses but %d priors" % (n, prior.shape[0]))
        out, report = np.zeros((n, 6)), np.zeros((n, self.num_scales, 4))
        self._enter()
        capi.check(capi.load().vg_photometric_compute_pose(self._h, n, xi.ctypes.data_as(_dp), tg.ctypes.data_as(_i32p),
                                                           prior.ctypes.data_as(_dp) if prior is not None else None,
                                                           out.ctypes.data_as(_dp), report.ctypes.data_as(_dp)))
        return (out[0], report[0]) if single else (out, report)

    def evaluate_mi(self, scale_idx, xi, target=None, values=True, gradient=True):
        """MutualInformation::Evaluate (8 bins, valMax 255) of the poses xi [n, 6] against target[k] (default: target 0) at one
        scale: a dict with cost [n] (the negative mutual information), hist [n, 8, 8] (the joint histogram, [bin of the
        target's sample, bin of the key frame's grey]), gradient [n, 6] or None (numpy) and values [n, m] or None (CUDA
        tensor: the target's grey at every point of the pack, 0 where the point does not project)"""
        import torch

        if not 0 <= scale_idx < self.num_scales:
            raise ValueError("scale index out of range")
        xi, tg = self._poses(xi, target)
        n = xi.shape[0]
        L = capi.load()
        val = None
        if values:
            m = ctypes.c_int64()
            capi.check(L.vg_photometric_pack(self._h, scale_idx, ctypes.byref(m), None, None, None))
            val = torch.zeros((n, m.value), dtype=torch.float64, device=self.device)
        cost, hist = np.zeros(n), np.zeros((n, capi.MI_NUM_BINS, capi.MI_NUM_BINS))
        grad = np.zeros((n, 6)) if gradient else None
        self._enter()
        capi.check(L.vg_mi_evaluate(self._h, scale_idx, n, xi.ctypes.data_as(_dp), tg.ctypes.data_as(_i32p),
                                                val.data_ptr() if values else None, hist.ctypes.data_as(_dp), cost.ctypes.data_as(_dp),
                                                grad.ctypes.data_as(_dp) if gradient else None))
        self._leave(val)
        return {"cost": cost, "hist": hist, "gradient": grad, "values": val}

    def compute_pose_mi(self, xi_start, target=None, xi_odom=None, function_tolerance=None, gradient_tolerance=None, max_iterations=None):
        """computePoseMI from the start poses xi_start [n, 6] (or one [6]) against target[k]: (poses, report); report is
        float64 [n, num_scales, 4]: REPORT per scale.  xi_odom ([n, 6]): the odometry's motion per start pose; it selects
        MutualInformationOdom, whose prior pose is the start pose; None: the plain cost.  The tolerances and the iteration cap
        (per scale) default to the reference's: capi.MI_DEFAULTS."""
        single = np.ndim(xi_start) == 1
        xi, tg = self._poses(xi_start, target)
        n = xi.shape[0]
        odom = None
        if xi_odom is not None:
            odom = np.ascontiguousarray(xi_odom, dtype=np.float64).reshape(-1, 6)
            if odom.shape[0] != n:
                raise ValueError("%d poses but %d odometry poses" % (n, odom.shape[0]))
        opt = capi.MiOptions()
        for name, v in (("function_tolerance", function_tolerance), ("gradient_tolerance", gradient_tolerance), ("max_iterations", max_iterations)):
            if v is not None:
                if not v > 0:
                    raise ValueError("%s must be positive" % name)
                setattr(opt, name, v)
        out, report = np.zeros((n, 6)), np.zeros((n, self.num_scales, 4))
        self._enter()
        capi.check(capi.load().vg_mi_compute_pose(self._h, n, xi.ctypes.data_as(_dp), tg.ctypes.data_as(_i32p),
                                                              odom.ctypes.data_as(_dp) if odom is not None else None, ctypes.byref(opt),
                                                              out.ctypes.data_as(_dp), report.ctypes.data_as(_dp)))
        return (out[0], report[0]) if single else (out, report)


def mi_odometry(xi_odom, xi_prior, xi):
    """the odometry term of MutualInformationOdom at the pose xi, host arithmetic: (cost, gradient [6])"""
    a, p, x = (_vec(v, 6, name) for v, name in ((xi_odom, "xi_odom"), (xi_prior, "xi_prior"), (xi, "xi")))
    cost, grad = ctypes.c_double(), np.zeros(6)
    capi.check(capi.load().vg_mi_odometry(a.ctypes.data_as(_dp), p.ctypes.data_as(_dp), x.ctypes.data_as(_dp), ctypes.byref(cost),
                                                      grad.ctypes.data_as(_dp)))
    return cost.value, grad
