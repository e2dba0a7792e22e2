"""Monocular visual odometry on the GPU (include/visgeom_amd.h section 15): the reference's MonoOdometry -- wheel-odometry poses
and camera images in, one after the other; the pose of the base frame and a key frame depth map that improves with every
frame out.  Thin torch wrapper over a vg_mono_odom handle, which runs sparse odometry, SGM, motion stereo, the depth map
warp / merge / filter and the photometric solve on the device without a map or an image crossing to the host; library errors
raise capi.VisgeomError, argument errors ValueError before the library is called."""
import ctypes

import numpy as np

from . import capi
from . import motion_stereo as _motion
from ._handle import LoopHandle, _dp, _is_cuda, _pose, _set_pipelines, _vec, _xi_base_camera

STATES = ("BEGIN", "SPARSE_INIT", "READY")
ACTIONS = ("FIRST", "WAITING", "SPARSE_INIT_KEYFRAME", "REFINED", "KEYFRAME", "DISCARDED")
REPORT = ("state_before", "state", "action", "K", "length", "length_prior", "iterations", "final_cost", "termination", "counts", "keyframes")
_THRESHOLDS = ("min_init_dist", "max_dist", "max_angle", "min_scale_length", "max_scale_ratio")


def default_params():
    """vg_mono_odom_params with the reference's constants"""
    p = capi.MonoOdomParams()
    capi.load().vg_mono_odom_params_default(ctypes.byref(p))
    return p


def make_params(motion=None, sparse=None, **kw):
    """vg_mono_odom_params from the defaults: motion (a vg_motion_stereo_params, motion_stereo.make_params), sparse (a
    vg_sparse_odom_params, sparse_odom.default_params) and keyword overrides of the thresholds and num_scales"""
    p = _set_pipelines(default_params(), motion, sparse)
    for k, v in kw.items():
        if k in _THRESHOLDS:
            setattr(p, k, float(v))
        elif k == "num_scales":
            p.num_scales = int(v)
        else:
            raise ValueError("unknown parameter %s" % k)
    return p


def params_from_json(root):
    """MonoOdometry(ptree) (mono_odom.cpp:35-47) of the JSON object `root` (a dict): (eucm [6], xi_base_cam [6], params) from
    "camera_params", "xi_base_camera" and "stereo_parameters" (as motion_stereo.params_from_json reads it); the optional
    "mono_odom_parameters" object of the mono_odom program replaces thresholds and num_scales"""
    xbc = _xi_base_camera(root)
    p = make_params(motion=_motion.params_from_json(root["stereo_parameters"]), **root.get("mono_odom_parameters", {}))
    return _vec(root["camera_params"], 6, "camera_params"), xbc, p


def integrate(xi_local, xi_odom_old, xi_odom_new):
    """feedWheelOdometry's arithmetic: xi_local o xi_odom_old^-1 o xi_odom_new (host only)"""
    a, b, c, out = _pose(xi_local, "xi_local"), _pose(xi_odom_old, "xi_odom_old"), _pose(xi_odom_new, "xi_odom_new"), np.zeros(6)
    capi.check(capi.load().vg_mono_odom_integrate(*[v.ctypes.data_as(_dp) for v in (a, b, c, out)]))
    return out


def normalize_scale(params, xi_local_old, xi_local_prior, xi_local_vo):
    """the scale normalisation of feedImage (host only): (xi_local, K, discarded)"""
    a, b, c, out = _pose(xi_local_old, "xi_local_old"), _pose(xi_local_prior, "xi_local_prior"), _pose(xi_local_vo, "xi_local_vo"), np.zeros(6)
    K, disc = ctypes.c_double(), ctypes.c_int()
    capi.check(capi.load().vg_mono_odom_normalize_scale(ctypes.byref(params), *[v.ctypes.data_as(_dp) for v in (a, b, c, out)],
                                                        ctypes.byref(K), ctypes.byref(disc)))
    return out, K.value, bool(disc.value)


def needs_keyframe(params, xi_local):
    """isNewKeyframeNeeded (host only)"""
    a, need = _pose(xi_local, "xi_local"), ctypes.c_int()
    capi.check(capi.load().vg_mono_odom_needs_keyframe(ctypes.byref(params), a.ctypes.data_as(_dp), ctypes.byref(need)))
    return bool(need.value)


def camera_motion(xi_base_cam, xi):
    """getCameraMotion: xi_base_cam^-1 o xi o xi_base_cam (host only)"""
    a, b, out = _pose(xi_base_cam, "xi_base_cam"), _pose(xi, "xi"), np.zeros(6)
    capi.check(capi.load().vg_mono_odom_camera_motion(*[v.ctypes.data_as(_dp) for v in (a, b, out)]))
    return out


def compose(a, b):
    """Transformation::compose a o b with the library's arithmetic (host only)"""
    a, b, out = _pose(a, "a"), _pose(b, "b"), np.zeros(6)
    capi.check(capi.load().vg_mono_odom_compose(*[v.ctypes.data_as(_dp) for v in (a, b, out)]))
    return out


class MonoOdometry(LoopHandle):
    """A vg_mono_odom handle on one device: one EUCM camera, xi_base_cam and the parameters (make_params); the image size is
    u_max x v_max of params.motion.stereo.  Images are uint8 CUDA tensors [height, width], maps float64 CUDA tensors [y_max,
    x_max], poses numpy [6] = [t, rotvec].  The handle's stream is torch's current stream of the device at creation; each call
    first makes it wait for the caller's current stream and is complete when it returns."""

    _destroy = "vg_mono_odom_destroy"
    _prefix = "vg_mono_odom_"
    _params = capi.MonoOdomParams

    def feed_wheel_odometry(self, xi_odom_new):
        """feedWheelOdometry: the wheel odometry's pose of the base frame; the first call only records it"""
        xi = _pose(xi_odom_new, "xi_odom_new")
        capi.check(capi.load().vg_mono_odom_feed_wheel_odometry(self._h, xi.ctypes.data_as(_dp)))

    def feed_image(self, img, samples=None):
        """feedImage: the report of the frame as a dict (REPORT; state and action by name, counts int64 [6]).  samples: the
        RANSAC sample table for sparse odometry (int32 [ransac_iterations, num_ransac_points]) or None for the library's."""
        rep = self._feed_image(img, samples, capi.MONO_ODOM_REPORT)
        return {"state_before": STATES[int(rep[0])], "state": STATES[int(rep[1])], "action": ACTIONS[int(rep[2])], "K": rep[3],
                "length": rep[4], "length_prior": rep[5], "iterations": int(rep[6]), "final_cost": rep[7], "termination": int(rep[8]),
                "counts": rep[9:15].astype(np.int64), "keyframes": int(rep[15])}

    def set_depth(self, depth_image):
        """setDepth: seed the map from a depth image, a float32 CUDA tensor [height, width] (the renderer's depth buffer)"""
        import torch

        if not _is_cuda(depth_image, torch.float32) or tuple(depth_image.shape) != (self.height, self.width):
            raise ValueError("depth_image must be a float32 CUDA tensor [%d, %d]" % (self.height, self.width))
        d = depth_image.contiguous()
        self._enter()
        capi.check(capi.load().vg_mono_odom_set_depth(self._h, d.data_ptr()))
        self._leave(d)

    def warp_image(self, src, xi=None, depth=None):
        """wrapImage: src seen from the key frame through the depth map (None: the handle's; else float64 [y_max, x_max]) and
        the pose xi (None: the current xi_local): a uint8 CUDA tensor [height, width], 0 where nothing lands"""
        import torch

        src = self._image(src, "src")
        x = _pose(xi, "xi") if xi is not None else None
        depth = self._depth(depth)
        dst = torch.empty((self.height, self.width), dtype=torch.uint8, device=self.device)
        self._enter()
        capi.check(capi.load().vg_mono_odom_warp_image(self._h, src.data_ptr(), x.ctypes.data_as(_dp) if x is not None else None,
                                                       depth.data_ptr() if depth is not None else None, dst.data_ptr()))
        self._leave(dst, src, depth)
        return dst

    @property
    def state(self):
        return STATES[self._geti("state")]

    @property
    def xi_local(self):
        return self._get6("xi_local")

    @property
    def xi_global(self):
        return self._get6("xi_global")

    @property
    def xi_composed(self):
        """xi_global o xi_local, the pose the reference prints"""
        return self._get6("xi_composed")

    @property
    def keyframe_increments(self):
        """transfVec: float64 [key frames, 6], the pose of every key frame in the one before it"""
        n = ctypes.c_int64()
        L = capi.load()
        capi.check(L.vg_mono_odom_num_keyframes(self._h, ctypes.byref(n)))
        out = np.zeros((n.value, 6))
        for k in range(n.value):
            capi.check(L.vg_mono_odom_keyframe_increment(self._h, k, out[k].ctypes.data_as(_dp)))
        return out
