"""Calibration trajectory planning on the GPU (include/visgeom_amd.h section 17): the reference's TrajectoryVisualQuality over
circular trajectories -- how well a set of robot trajectories in front of a calibration board makes the camera-odometry
extrinsics observable, and the trajectories that do it best.  Thin wrapper over a vg_trajectory handle: parameter points and
results are host numpy arrays, the batches run on the device.  Library errors raise capi.VisgeomError, argument errors
ValueError before the library is called."""
import ctypes

import numpy as np

from . import capi
from ._handle import Handle, _vec

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_i32p = ctypes.POINTER(ctypes.c_int32)
TERMS = ("information", "image_limits", "curvature", "distance", "normal")


def _steps(steps):
    s = np.ascontiguousarray(steps, dtype=np.intc).ravel()
    if not 1 <= s.size <= capi.TRAJECTORY_MAX:
        raise ValueError("1 to %d trajectories expected" % capi.TRAJECTORY_MAX)
    if s.min() < capi.TRAJECTORY_MIN_STEPS or s.max() > capi.TRAJECTORY_MAX_STEPS:
        raise ValueError("a trajectory's number of steps must be in [%d, %d]" % (capi.TRAJECTORY_MIN_STEPS, capi.TRAJECTORY_MAX_STEPS))
    return s


def make_quality(quality):
    """a vg_trajectory_quality from the "quality_parameters" object of a plan file"""
    if isinstance(quality, capi.TrajectoryQuality):
        return quality
    q = capi.TrajectoryQuality()
    q.xi_base_cam[:] = _vec(quality["xiBaseCam"], 6, "xiBaseCam").tolist()
    q.xi_orig_board[:] = _vec(quality["xiOrigBoard"], 6, "xiOrigBoard").tolist()
    q.turn_radius = float(quality["turn_radius"])
    q.board_cols, q.board_rows = int(quality["board"]["cols"]), int(quality["board"]["rows"])
    q.board_step = float(quality["board"]["step"])
    q.min_camera_dist = float(quality["min_camera_dist"])
    q.min_margin = float(quality["min_margin"])
    q.min_cell_size = float(quality["min_cell_size"])
    q.prior_variance[:] = _vec(quality["prior_variance"], 6, "prior_variance").tolist()
    q.feature_variance = float(quality["feature_variance"])
    return q


def trajectory_poses(params, steps):
    """CircularTrajectory::compute on the host: (xi [sum steps, 6], cov [sum steps, 6, 6]) of the trajectories of one parameter
    point [5 T], trajectory after trajectory"""
    s = _steps(steps)
    p = _vec(params, capi.TRAJECTORY_PARAMS * s.size, "params")
    total = int(s.sum())
    xi, cov = np.zeros((total, 6)), np.zeros((total, 6, 6))
    capi.check(capi.load().vg_trajectory_poses(s.size, s.ctypes.data_as(_ip), p.ctypes.data_as(_dp), xi.ctypes.data_as(_dp), cov.ctypes.data_as(_dp)))
    return xi, cov


def gradient_points(params):
    """the points of one numerical gradient as the library forms them: (points [2 P + 1, P], delta [P])"""
    p = np.ascontiguousarray(params, dtype=np.float64).ravel()
    pts, delta = np.zeros((2 * p.size + 1, p.size)), np.zeros(p.size)
    capi.check(capi.load().vg_trajectory_gradient_points(p.size, p.ctypes.data_as(_dp), pts.ctypes.data_as(_dp), delta.ctypes.data_as(_dp)))
    return pts, delta


class TrajectoryPlanner(Handle):
    """A vg_trajectory handle on one device.  camera: the 6 EUCM intrinsics; width, height: the image; quality: the
    "quality_parameters" object of a plan file (or a capi.TrajectoryQuality); steps: the number of poses of every trajectory.
    A parameter point has 5 numbers per trajectory: x0, y0, theta0, the chord and the turn of one step."""

    _destroy = "vg_trajectory_destroy"

    def __init__(self, camera, width, height, quality, steps, device=0):
        import torch

        self._c = _vec(camera, 6, "camera")
        self._q = make_quality(quality)
        self.steps = _steps(steps)
        self.n_params = capi.TRAJECTORY_PARAMS * self.steps.size
        self.device = torch.device("cuda", device)
        self._open(capi.load().vg_trajectory_create, capi.MODEL_EUCM, self._c.ctypes.data_as(_dp), int(width), int(height),
                   ctypes.byref(self._q), self.steps.size, self.steps.ctypes.data_as(_ip))

    def _points(self, params):
        a = np.ascontiguousarray(params, dtype=np.float64)
        if a.ndim not in (1, 2) or a.shape[-1] != self.n_params:
            raise ValueError("params must be [%d] or [n, %d]" % (self.n_params, self.n_params))
        if not np.isfinite(a).all():
            raise ValueError("params must be finite")
        return a.reshape(-1, self.n_params).copy(), a.ndim == 1

    def evaluate(self, params):
        """(cost [n], terms [n, 5] in the order of TERMS, invalid [n]: the number of invalid poses) at params [n, P]; a single
        point [P] gives a float, [5] and an int"""
        p, single = self._points(params)
        n = p.shape[0]
        cost, terms, invalid = np.zeros(n), np.zeros((n, capi.TRAJECTORY_TERMS)), np.zeros(n, dtype=np.int32)
        self._enter()
        capi.check(capi.load().vg_trajectory_evaluate(self._h, n, p.ctypes.data_as(_dp), cost.ctypes.data_as(_dp), terms.ctypes.data_as(_dp),
                                                      invalid.ctypes.data_as(_i32p)))
        return (float(cost[0]), terms[0], int(invalid[0])) if single else (cost, terms, invalid)

    def gradient(self, params):
        """(cost [n], gradient [n, P], invalid [n]): central differences over one batch; the gradient of a point with an invalid
        evaluation is NaN"""
        p, single = self._points(params)
        n = p.shape[0]
        cost, grad, invalid = np.zeros(n), np.zeros((n, self.n_params)), np.zeros(n, dtype=np.int32)
        self._enter()
        capi.check(capi.load().vg_trajectory_gradient(self._h, n, p.ctypes.data_as(_dp), cost.ctypes.data_as(_dp), grad.ctypes.data_as(_dp),
                                                      invalid.ctypes.data_as(_i32p)))
        return (float(cost[0]), grad[0], int(invalid[0])) if single else (cost, grad, invalid)

    def visual_cov(self, cam_poses):
        """(cov [n, 6, 6], info [n, 6, 6], invalid [n]) of the board seen from the camera poses [n, 6] ([t, rotvec] in the world)"""
        a = np.ascontiguousarray(cam_poses, dtype=np.float64)
        if a.ndim not in (1, 2) or a.shape[-1] != 6 or not np.isfinite(a).all():
            raise ValueError("cam_poses must be finite, [6] or [n, 6]")
        single = a.ndim == 1
        a = a.reshape(-1, 6).copy()
        n = a.shape[0]
        cov, info, invalid = np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), np.zeros(n, dtype=np.int32)
        self._enter()
        capi.check(capi.load().vg_trajectory_visual_cov(self._h, n, a.ctypes.data_as(_dp), cov.ctypes.data_as(_dp), info.ctypes.data_as(_dp),
                                                        invalid.ctypes.data_as(_i32p)))
        return (cov[0], info[0], int(invalid[0])) if single else (cov, info, invalid)

    def poses(self, params):
        """the integrated trajectories of one point: (xi [sum steps, 6], cov [sum steps, 6, 6]); host arithmetic"""
        return trajectory_poses(params, self.steps)

    def optimize(self, starts, options=None):
        """One minimisation per start [n, P] (or one start [P]), in lock-step: (params, cost, iterations, termination).  options:
        a capi.TrajectoryOptions or a dict of its fields over the defaults."""
        p, single = self._points(starts)
        n = p.shape[0]
        opt = capi.TrajectoryOptions()
        capi.load().vg_trajectory_default_options(ctypes.byref(opt))
        if isinstance(options, capi.TrajectoryOptions):
            opt = options
        elif options is not None:
            for k, v in dict(options).items():
                if k not in dict(capi.TrajectoryOptions._fields_):
                    raise ValueError("unknown option %r" % k)
                setattr(opt, k, v)
        cost, iterations, termination = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        self._enter()
        capi.check(capi.load().vg_trajectory_optimize(self._h, n, p.ctypes.data_as(_dp), ctypes.byref(opt), cost.ctypes.data_as(_dp),
                                                      iterations.ctypes.data_as(_i32p), termination.ctypes.data_as(_i32p)))
        return (p[0], float(cost[0]), int(iterations[0]), int(termination[0])) if single else (p, cost, iterations, termination)

    @property
    def launches(self):
        """kernel launches of the handle so far"""
        c = ctypes.c_int64()
        capi.check(capi.load().vg_trajectory_launch_count(self._h, ctypes.byref(c)))
        return c.value
