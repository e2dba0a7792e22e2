"""Photometric mapping on the GPU (include/visgeom_amd.h section 16): the reference's PhotometricMapping -- wheel-odometry poses
and camera images in, one after the other; a map of key frames (image + global pose) that SLAM builds where nothing is mapped,
and in a mapped area the pose of the base frame from mutual-information relocalisation of the inter frame against the nearest
map frame.  Thin torch wrapper over a vg_mapping handle, which runs sparse odometry, SGM, motion stereo, the depth map warp /
merge / filter, the photometric and the MI solve on the device without a map or an image crossing to the host; library errors
raise capi.VisgeomError, argument errors ValueError before the library is called."""
import ctypes

import numpy as np

from . import capi
from . import motion_stereo as _motion
from ._handle import LoopHandle, _dp, _pose, _set_pipelines, _vec, _xi_base_camera

_i64p = ctypes.POINTER(ctypes.c_int64)
STATES = ("BEGIN", "INIT", "LOCALIZE", "SLAM")
WARNINGS = ("NONE", "SCALE", "ROTATION")
ACTIONS = ("FIRST", "WAITING", "INIT_SLAM", "INIT_LOCALIZE", "LOCALIZE_REFINED", "LOCALIZE_INTER_FRAME", "LOCALIZE_MAP_FRAME_CHANGED",
           "LOCALIZE_MAP_FRAME_KEPT", "LOCALIZE_LEFT_MAP", "SLAM_REFINED", "SLAM_INTER_FRAME", "SLAM_ENTERED_MAP")
REPORT = ("state_before", "state", "action", "warning", "map_index_before", "map_index", "K", "length", "length_prior", "rot_diff",
          "iterations", "final_cost", "termination", "mi_iterations", "mi_initial_cost", "mi_final_cost", "mi_termination", "sgm", "refined",
          "motion_counts", "merge_counts", "frames")
SELECT_K = 4.   # selectMapFrame's default K; checkDistance's is 1
_SQUARED = ("new_kf_distance_thresh", "new_kf_angular_thresh")
_DOUBLES = ("min_init_dist", "min_stereo_base", "dist_thresh", "rotation_tolerance", "min_scale_length", "min_scale_ratio", "max_scale_ratio")


def default_params():
    """vg_mapping_params with the reference's constants"""
    p = capi.MappingParams()
    capi.load().vg_mapping_params_default(ctypes.byref(p))
    return p


def make_params(motion=None, sparse=None, **kw):
    """vg_mapping_params from the defaults: motion (a vg_motion_stereo_params), sparse (a vg_sparse_odom_params) and keyword
    overrides.  new_kf_distance_thresh and new_kf_angular_thresh are given as the reference's JSON gives them, a distance and an
    angle, and stored squared."""
    p = _set_pipelines(default_params(), motion, sparse)
    for k, v in kw.items():
        if k in _SQUARED:
            setattr(p, k, float(v) ** 2)
        elif k in _DOUBLES:
            setattr(p, k, float(v))
        elif k == "normalize_scale":
            p.normalize_scale = 1 if v else 0
        elif k == "num_scales":
            p.num_scales = int(v)
        else:
            raise ValueError("unknown parameter %s" % k)
    return p


def params_from_json(root):
    """PhotometricMapping(ptree) (mapping.cpp:27-43) of the JSON object `root` (a dict): (eucm [6], xi_base_cam [6], params)
    from "camera_params", "xi_base_camera", "stereo_parameters" and "mapping_parameters" (MappingParameters(ptree): the two
    new_kf thresholds are squared; the fields the reference has as literals may be given there too)"""
    xbc = _xi_base_camera(root)
    p = make_params(motion=_motion.params_from_json(root["stereo_parameters"]), **root.get("mapping_parameters", {}))
    return _vec(root["camera_params"], 6, "camera_params"), xbc, p


def check_distance(params, xi, K=1.):
    """checkDistance (host only): |rot|^2 < angular threshold and t0^2 / 5 + t1^2 + t2^2 < distance threshold * K"""
    a, ok = _pose(xi, "xi"), ctypes.c_int()
    capi.check(capi.load().vg_mapping_check_distance(ctypes.byref(params), a.ctypes.data_as(_dp), float(K), ctypes.byref(ok)))
    return bool(ok.value)


def select_frame(params, poses, xi, K=SELECT_K):
    """selectMapFrame over poses [n, 6] (host only): the index of the nearest frame that passes checkDistance, or -1"""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 6)
    if not np.isfinite(poses).all():
        raise ValueError("poses must be finite")
    a, idx = _pose(xi, "xi"), ctypes.c_int()
    capi.check(capi.load().vg_mapping_select_frame_host(ctypes.byref(params), poses.shape[0], poses.ctypes.data_as(_dp), a.ctypes.data_as(_dp),
                                                        float(K), ctypes.byref(idx)))
    return idx.value


def normalize_scale(params, xi_local_old, xi_local_prior, xi_local_vo):
    """the tail of localizePhoto (host only): a dict with xi (the new xi_local), K, length, length_prior, rot_diff and warning
    (by name)"""
    a, b, c, out = _pose(xi_local_old, "xi_local_old"), _pose(xi_local_prior, "xi_local_prior"), _pose(xi_local_vo, "xi_local_vo"), np.zeros(6)
    num = [ctypes.c_double() for _ in range(4)]
    warn = ctypes.c_int()
    capi.check(capi.load().vg_mapping_normalize_scale(ctypes.byref(params), *[v.ctypes.data_as(_dp) for v in (a, b, c, out)],
                                                      *[ctypes.byref(v) for v in num], ctypes.byref(warn)))
    return {"xi": out, "K": num[0].value, "length": num[1].value, "length_prior": num[2].value, "rot_diff": num[3].value,
            "warning": WARNINGS[warn.value]}


def relocalized_pose(xi_map, xi_fr_map):
    """localizeMI's last line (host only): the inter frame's global pose xi_map o xi_fr_map^-1"""
    a, b, out = _pose(xi_map, "xi_map"), _pose(xi_fr_map, "xi_fr_map"), np.zeros(6)
    capi.check(capi.load().vg_mapping_relocalized_pose(*[v.ctypes.data_as(_dp) for v in (a, b, out)]))
    return out


def report_dict(rep):
    """a report array [capi.MAPPING_REPORT] as a dict (REPORT): states, action and warning by name"""
    return {"state_before": STATES[int(rep[0])], "state": STATES[int(rep[1])], "action": ACTIONS[int(rep[2])], "warning": WARNINGS[int(rep[3])],
            "map_index_before": int(rep[4]), "map_index": int(rep[5]), "K": rep[6], "length": rep[7], "length_prior": rep[8], "rot_diff": rep[9],
            "iterations": int(rep[10]), "final_cost": rep[11], "termination": int(rep[12]), "mi_iterations": int(rep[13]),
            "mi_initial_cost": rep[14], "mi_final_cost": rep[15], "mi_termination": int(rep[16]), "sgm": bool(rep[17]), "refined": bool(rep[18]),
            "motion_counts": rep[19:25].astype(np.int64), "merge_counts": rep[25:30].astype(np.int64), "frames": int(rep[30])}


class PhotometricMapping(LoopHandle):
    """A vg_mapping handle on one device: one EUCM camera, xi_base_cam and the parameters (make_params); the image size is u_max
    x v_max of params.motion.stereo.  Images are uint8 CUDA tensors [height, width], maps float64 CUDA tensors [y_max, x_max],
    poses numpy [6] = [t, rotvec].  The handle's stream is torch's current stream of the device at creation; each call first
    makes it wait for the caller's current stream and is complete when it returns."""

    _destroy = "vg_mapping_destroy"
    _prefix = "vg_mapping_"
    _params = capi.MappingParams

    def feed_odometry(self, xi_odom_new):
        """feedOdometry: the wheel odometry's pose of the base frame; the first call (and the first after reinit) only records it"""
        xi = _pose(xi_odom_new, "xi_odom_new")
        capi.check(capi.load().vg_mapping_feed_odometry(self._h, xi.ctypes.data_as(_dp)))

    def reinit(self, xi):
        """reInit: a new pass starts at the global pose xi; in SLAM the inter frame goes into the map first"""
        xi = _pose(xi, "xi")
        self._enter()
        capi.check(capi.load().vg_mapping_reinit(self._h, xi.ctypes.data_as(_dp)))

    def feed_image(self, img, samples=None):
        """feedImage: the report of the frame as a dict (REPORT).  samples: the RANSAC sample table for sparse odometry (int32
        [ransac_iterations, num_ransac_points]) or None for the library's."""
        return report_dict(self._feed_image(img, samples, capi.MAPPING_REPORT))

    @property
    def num_frames(self):
        n = ctypes.c_int64()
        capi.check(capi.load().vg_mapping_num_frames(self._h, ctypes.byref(n)))
        return n.value

    def get_frame(self, k, image=True):
        """map frame k: (pose [6], image uint8 CUDA tensor [height, width] or None)"""
        import torch

        xi = np.zeros(6)
        img = torch.empty((self.height, self.width), dtype=torch.uint8, device=self.device) if image else None
        self._enter()
        capi.check(capi.load().vg_mapping_get_frame(self._h, int(k), xi.ctypes.data_as(_dp), img.data_ptr() if image else None))
        self._leave(img)
        return xi, img

    @property
    def frame_poses(self):
        """the map's poses, float64 [frames, 6]"""
        return np.array([self.get_frame(k, image=False)[0] for k in range(self.num_frames)]).reshape(-1, 6)

    def add_frame(self, xi, img):
        """an unconditional insert into the map (reloading a saved one)"""
        xi, img = _pose(xi, "xi"), self._image(img)
        self._enter()
        capi.check(capi.load().vg_mapping_add_frame(self._h, xi.ctypes.data_as(_dp), img.data_ptr()))
        self._leave(img)

    def construct_map(self, xi, img):
        """constructMap: insert when no frame lies within the K = 1 distance of xi; True when inserted"""
        xi, img, ins = _pose(xi, "xi"), self._image(img), ctypes.c_int()
        self._enter()
        capi.check(capi.load().vg_mapping_construct_map(self._h, xi.ctypes.data_as(_dp), img.data_ptr(), ctypes.byref(ins)))
        self._leave(img)
        return bool(ins.value)

    def select_frame(self, xi, K=SELECT_K):
        """selectMapFrame on the handle's map: the index or -1"""
        xi, idx = _pose(xi, "xi"), ctypes.c_int()
        capi.check(capi.load().vg_mapping_select_frame(self._h, xi.ctypes.data_as(_dp), float(K), ctypes.byref(idx)))
        return idx.value

    def alignment(self, img, xi=None, base=None, depth=None, err=True):
        """wrapImage of img at xi (None: xi_local) through depth (None: the handle's map), computeErr against base (None: the
        inter image) and the sums, one launch: (err uint8 CUDA tensor [height, width] or None, sums int64 [3] = compared
        pixels, sum |base - warped|, sum (base - warped)^2)"""
        import torch

        img = self._image(img)
        base = self._image(base, "base") if base is not None else None
        x = _pose(xi, "xi") if xi is not None else None
        depth = self._depth(depth)
        out = torch.empty((self.height, self.width), dtype=torch.uint8, device=self.device) if err else None
        sums = np.zeros(3, np.int64)
        self._enter()
        capi.check(capi.load().vg_mapping_alignment(self._h, base.data_ptr() if base is not None else None, img.data_ptr(),
                                                    x.ctypes.data_as(_dp) if x is not None else None,
                                                    depth.data_ptr() if depth is not None else None, out.data_ptr() if err else None,
                                                    sums.ctypes.data_as(_i64p)))
        self._leave(out, img, base, depth)
        return out, sums

    @property
    def state(self):
        return STATES[self._geti("state")]

    @property
    def map_index(self):
        return self._geti("map_index")

    @property
    def warning(self):
        return WARNINGS[self._geti("warning")]

    @property
    def xi_local(self):
        return self._get6("xi_local")

    @property
    def xi_inter(self):
        return self._get6("xi_inter")

    @property
    def xi_composed(self):
        """xi_inter o xi_local, the pose both reference programs log"""
        return self._get6("xi_composed")
