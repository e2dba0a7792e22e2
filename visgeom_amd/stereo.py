"""Dense fisheye stereo on the GPU (include/visgeom_amd.h section 9): the reference's EnhancedSgm, semi-global matching along
the epipolar curves of two unrectified EUCM images.  Thin torch wrapper over a vg_stereo handle; library errors raise
capi.VisgeomError."""
import ctypes

import numpy as np

from . import capi
from ._handle import Handle, _u8_images, _vec   # _vec: other modules and tests take it from here

_dp = ctypes.POINTER(ctypes.c_double)

# JSON keys of ex_epipolar_stereo.json's "stereo_parameters" object -> vg_stereo_params fields
_SCALE_KEYS = {"scale": "scale", "u0": "u0", "v0": "v0", "uMax": "u_max", "vMax": "v_max", "xMax": "x_max", "yMax": "y_max"}
_STEREO_KEYS = {"disparity_max": "disp_max", "error_max": "error_max", "verbosity": "verbosity", "hypotheses": "hypotheses",
                "hypo_difference": "hypo_difference", "flaw_cost": "flaw_cost", "descriptor_size": "desc_length",
                "descriptor_response_thresh": "desc_resp_thresh", "num_epipolar_planes": "num_epipolar_planes"}
_SGM_KEYS = {"step_cost": "step_cost", "jump_cost": "jump_cost", "image_based_cost": "image_based_cost",
             "salient_points_only": "salient_points_only", "use_uv_cache": "use_uv_cache"}


def default_params():
    """vg_stereo_params with the reference's defaults"""
    p = capi.StereoParams()
    capi.load().vg_stereo_params_default(ctypes.byref(p))
    return p


def params_from_json(sp, base=None):
    """SgmParameters(ptree) (eucm_sgm.h:43-55) of the "stereo_parameters" object `sp` (a dict): the scale keys at its top level,
    stereo keys under "stereo_parameters" (num_epipolar_planes and epipole_margin too, where the reference reads them), SGM keys
    under "sgm_stereo_parameters".  Unknown keys are ignored, like the reference."""
    p = base if base is not None else default_params()

    def put(field, val):
        setattr(p, field, int(val))

    for k, f in _SCALE_KEYS.items():
        if k in sp:
            put(f, sp[k])
    if sp.get("equal_margins"):
        p.equal_margins = 1
    inner = sp.get("stereo_parameters", {})
    if "epipole_margin" in inner:
        p.epipole_margin = int(inner["epipole_margin"]) ** 2
    for k, f in _STEREO_KEYS.items():
        if k in inner:
            put(f, inner[k])
    sc = inner.get("scales")
    if sc is not None:
        if not 1 <= len(sc) <= 8:
            raise ValueError("1 to 8 descriptor scales")
        p.n_scales = len(sc)
        for i in range(8):
            p.scales[i] = int(sc[i]) if i < len(sc) else 0
    sgm = sp.get("sgm_stereo_parameters", {})
    for k, f in _SGM_KEYS.items():
        if k in sgm:
            put(f, sgm[k])
    return p


def make_params(**kw):
    """vg_stereo_params from the defaults and keyword overrides (field names of the struct; scales=[...])"""
    p = default_params()
    for k, v in kw.items():
        if k == "scales":
            p.n_scales = len(v)
            for i in range(8):
                p.scales[i] = int(v[i]) if i < len(v) else 0
        else:
            setattr(p, k, int(v))
    return p


class Stereo(Handle):
    """A vg_stereo handle on one device: create once per calibrated pair, then compute any number of image batches.

    The handle's stream is torch's current stream of the device when the handle is created, and every later call runs on it.
    Each call first makes that stream wait for the caller's current stream, so images produced there are ready; the outputs
    are complete when a call returns (the library synchronises its stream)."""

    _destroy = "vg_stereo_destroy"

    def __init__(self, eucm1, eucm2, xi12, params, device=0):
        import torch

        self._c = [_vec(eucm1, 6, "eucm1"), _vec(eucm2, 6, "eucm2"), _vec(xi12, 6, "xi12")]
        self.device = torch.device("cuda", device)
        self.params = params
        L = capi.load()
        self._open(L.vg_stereo_create, *[c.ctypes.data_as(_dp) for c in self._c], ctypes.byref(params))
        xm, ym = ctypes.c_int(), ctypes.c_int()
        capi.check(L.vg_stereo_size(self._h, ctypes.byref(xm), ctypes.byref(ym)))
        self.x_max, self.y_max = xm.value, ym.value

    def _images(self, img1, img2):
        (a, single), (b, _) = (_u8_images(im, self.params.v_max, self.params.u_max, "images") for im in (img1, img2))
        if img1.shape != img2.shape:
            raise ValueError("the two image batches differ in shape")
        return a, b, single

    def _empty(self, n, *tail, dtype):
        import torch

        return torch.empty((n, self.y_max, self.x_max) + tail, dtype=dtype, device=self.device)

    def compute(self, img1, img2):
        """computeStereo of n pairs: (depth, sigma, cost) float64 and disparity int32, each [n, y_max, x_max] (no n for one
        [vMax, uMax] pair)"""
        import torch

        a, b, single = self._images(img1, img2)
        n = a.shape[0]
        depth, sigma, cost = (self._empty(n, dtype=torch.float64) for _ in range(3))
        disp = self._empty(n, dtype=torch.int32)
        self._enter()
        capi.check(capi.load().vg_stereo_compute(self._h, n, a.data_ptr(), b.data_ptr(), depth.data_ptr(), sigma.data_ptr(),
                                                 cost.data_ptr(), disp.data_ptr()))
        out = (depth, sigma, cost, disp)
        self._leave(*out, a, b)
        return tuple(t[0] for t in out) if single else out

    def compute_mh(self, img1, img2, hypotheses):
        """computeStereo with `hypotheses` (2 ... 8) depth hypotheses per pixel (reconstructDisparityMH): (depth, sigma, cost)
        float64, disparity and final_cost int32, each [n, hypotheses, y_max, x_max] (no n for one [vMax, uMax] pair); plane h
        holds the h-th cheapest local minimum of the aggregated cost, -1 / INT32_MAX where there is none"""
        import torch

        a, b, single = self._images(img1, img2)
        n, k = a.shape[0], int(hypotheses)
        shape = (n, k, self.y_max, self.x_max)
        depth, sigma, cost = (torch.empty(shape, dtype=torch.float64, device=self.device) for _ in range(3))
        disp, final = (torch.empty(shape, dtype=torch.int32, device=self.device) for _ in range(2))
        self._enter()
        capi.check(capi.load().vg_stereo_compute_mh(self._h, n, a.data_ptr(), b.data_ptr(), k, depth.data_ptr(), sigma.data_ptr(),
                                                    cost.data_ptr(), disp.data_ptr(), final.data_ptr()))
        out = (depth, sigma, cost, disp, final)
        self._leave(*out, a, b)
        return tuple(t[0] for t in out) if single else out

    def geometry(self):
        """the per-pixel geometry, int32 [y_max, x_max, 8] (status, pinf u, v, curve index, flags 1, flags 2, 0, 0)"""
        import torch

        g = torch.empty((self.y_max, self.x_max, 8), dtype=torch.int32, device=self.device)
        self._enter()
        capi.check(capi.load().vg_stereo_geometry(self._h, g.data_ptr()))
        return self._leave(g)

    def curve_cost(self, img1, img2):
        """computeCurveCost: err uint8 [n, y, x, disp_max], step, salient, skip uint8 [n, y, x]"""
        import torch

        a, b, _ = self._images(img1, img2)
        n = a.shape[0]
        err = self._empty(n, self.params.disp_max, dtype=torch.uint8)
        step, sal, skip = (self._empty(n, dtype=torch.uint8) for _ in range(3))
        self._enter()
        capi.check(capi.load().vg_stereo_curve_cost(self._h, n, a.data_ptr(), b.data_ptr(), err.data_ptr(), step.data_ptr(),
                                                    sal.data_ptr(), skip.data_ptr()))
        self._leave(err, step, sal, skip, a, b)
        return err, step, sal, skip

    def aggregate(self, img1, img2):
        """L + R + T + B int32 [n, y, x, disp_max] and the winner int32 [n, y, x]"""
        import torch

        a, b, _ = self._images(img1, img2)
        n = a.shape[0]
        tot = self._empty(n, self.params.disp_max, dtype=torch.int32)
        disp = self._empty(n, dtype=torch.int32)
        self._enter()
        capi.check(capi.load().vg_stereo_aggregate(self._h, n, a.data_ptr(), b.data_ptr(), tot.data_ptr(), disp.data_ptr()))
        self._leave(tot, disp, a, b)
        return tot, disp

    def chunk(self):
        c = ctypes.c_int64()
        capi.check(capi.load().vg_stereo_chunk(self._h, ctypes.byref(c)))
        return c.value


def stereo(img1, img2, eucm1, eucm2, xi12, params, device=None):
    """One-shot EnhancedSgm::computeStereo: returns (depth, sigma, cost, disparity) -- see Stereo.compute"""
    dev = img1.device.index if device is None else device
    s = Stereo(eucm1, eucm2, xi12, params, dev)
    try:
        return s.compute(img1, img2)
    finally:
        s.close()


def curve_walk(poly6, u, v, eu, ev, step_mult, steps):
    """Host CurveRasterizer walk (vg_stereo_curve_walk): int32 [|steps| + 1, 2]"""
    p = _vec(poly6, 6, "poly6")
    out = np.zeros((abs(int(steps)) + 1, 2), dtype=np.int32)
    capi.check(capi.load().vg_stereo_curve_walk(p.ctypes.data_as(_dp), int(u), int(v), int(eu), int(ev), int(step_mult), int(steps),
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return out
