"""Motion stereo on the GPU (include/visgeom_amd.h section 10): the reference's MotionStereo -- a key frame's depth map computed
or refined from a further image of a moving camera.  Thin torch wrapper over a vg_motion_stereo handle; library errors raise
capi.VisgeomError."""
import ctypes

import numpy as np

from . import capi
from . import stereo as _stereo
from ._handle import Handle, _is_cuda, _u8_images, _vec

_dp = ctypes.POINTER(ctypes.c_double)
_STEREO_FIELDS = {n for n, _ in capi.StereoParams._fields_}
STATUS = {1: "select", 2: "uncertainty", 3: "too_certain", 4: "sample", 5: "kept", 6: "updated"}
RECORD = ("status", "gstep", "gu2", "gv2", "start_u", "start_v", "end_u", "end_v", "disp_max", "inverted", "best", "best_cost", "index2")


def default_params():
    """vg_motion_stereo_params with the reference's defaults (gradient_thresh 2)"""
    p = capi.MotionStereoParams()
    capi.load().vg_motion_stereo_params_default(ctypes.byref(p))
    return p


def params_from_json(sp):
    """MotionStereoParameters(ptree) (eucm_motion_stereo.h:39-49) of the "stereo_parameters" object `sp` (a dict): what
    visgeom_amd.stereo.params_from_json reads plus "motion_stereo_parameters": {"gradient_thresh": ...}"""
    p = default_params()
    _stereo.params_from_json(sp, base=p.stereo)
    m = sp.get("motion_stereo_parameters", {})
    if "gradient_thresh" in m:
        p.gradient_thresh = int(m["gradient_thresh"])
    return p


def make_params(**kw):
    """vg_motion_stereo_params from the defaults and keyword overrides: gradient_thresh and the fields of vg_stereo_params"""
    p = default_params()
    for k, v in kw.items():
        if k == "gradient_thresh":
            p.gradient_thresh = int(v)
        elif k == "scales":
            p.stereo.n_scales = len(v)
            for i in range(8):
                p.stereo.scales[i] = int(v[i]) if i < len(v) else 0
        elif k in _STEREO_FIELDS:
            setattr(p.stereo, k, int(v))
        else:
            raise ValueError("unknown parameter %s" % k)
    return p


class MotionStereo(Handle):
    """A vg_motion_stereo handle on one device.  set_base() takes the key frame(s); compute() pairs key frame k with img2[k]
    under the pose xi12[k] and returns the new (depth, sigma, cost).  The handle's stream is torch's current stream of the
    device at creation; each call first makes it wait for the caller's current stream and is complete when it returns."""

    _destroy = "vg_motion_stereo_destroy"

    def __init__(self, eucm1, eucm2, params, device=0):
        import torch

        self._c = [_vec(eucm1, 6, "eucm1"), _vec(eucm2, 6, "eucm2")]
        self.device = torch.device("cuda", device)
        self.params = params
        self.counts = None
        self.n_base = 0
        L = capi.load()
        self._open(L.vg_motion_stereo_create, *[c.ctypes.data_as(_dp) for c in self._c], ctypes.byref(params))
        xm, ym = ctypes.c_int(), ctypes.c_int()
        capi.check(L.vg_motion_stereo_size(self._h, ctypes.byref(xm), ctypes.byref(ym)))
        self.x_max, self.y_max = xm.value, ym.value

    def _images(self, img):
        return _u8_images(img, self.params.stereo.v_max, self.params.stereo.u_max, "images")

    def set_base(self, img1):
        """setBaseImage of one key frame [vMax, uMax] or n key frames [n, vMax, uMax]"""
        a, _ = self._images(img1)
        self._enter()
        capi.check(capi.load().vg_motion_stereo_set_base(self._h, a.shape[0], a.data_ptr()))
        self._leave(a)
        self.n_base = a.shape[0]

    def _call(self, xi12, img2, prior):
        import torch

        b, single = self._images(img2)
        n = b.shape[0]
        xi = np.ascontiguousarray(xi12, dtype=np.float64).reshape(-1, 6)
        if xi.shape[0] != n:
            raise ValueError("%d images but %d transformations" % (n, xi.shape[0]))
        pr = [None, None, None]
        if prior is not None:
            if len(prior) != 3:
                raise ValueError("prior must be (depth, sigma, cost)")
            pr = []
            for t in prior:
                if not _is_cuda(t, torch.float64):
                    raise ValueError("the prior must be float64 CUDA tensors")
                t = t[None] if single and t.dim() == 2 else t
                if tuple(t.shape) != (n, self.y_max, self.x_max):
                    raise ValueError("the prior must be [n, y_max, x_max] = [%d, %d, %d]" % (n, self.y_max, self.x_max))
                pr.append(t.contiguous())
        return b, single, n, xi, pr

    def compute(self, xi12, img2, prior=None, out=None):
        """MotionStereo::compute: (depth, sigma, cost) float64 [n, y_max, x_max] (no n for one [vMax, uMax] image).  prior: the
        (depth, sigma, cost) map to refine, or None.  out: three tensors to write into (they may be the prior's).  The six
        per-item counters of the call are left in self.counts (int64 [n, 6])."""
        import torch

        b, single, n, xi, pr = self._call(xi12, img2, prior)
        if out is None:
            res = [torch.empty((n, self.y_max, self.x_max), dtype=torch.float64, device=self.device) for _ in range(3)]
        else:
            res = [t[None] if single and t.dim() == 2 else t for t in out]
            for t in res:
                if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (n, self.y_max, self.x_max):
                    raise ValueError("out must be contiguous float64 CUDA tensors [n, y_max, x_max]")
        counts = np.zeros((n, 6), dtype=np.int64)
        self._enter()
        capi.check(capi.load().vg_motion_stereo_compute(
            self._h, n, xi.ctypes.data_as(_dp), b.data_ptr(), *[t.data_ptr() if t is not None else None for t in pr],
            *[t.data_ptr() for t in res], counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        self._leave(*res, b, *pr)
        self.counts = counts
        return tuple(t[0] for t in res) if single else tuple(res)

    def mask(self):
        """the gradient mask of the key frames, uint8 [n_base, vMax, uMax] (0 / 128)"""
        import torch

        sp = self.params.stereo
        m = torch.empty((self.n_base, sp.v_max, sp.u_max), dtype=torch.uint8, device=self.device)
        self._enter()
        capi.check(capi.load().vg_motion_stereo_mask(self._h, m.data_ptr()))
        return self._leave(m)

    def select(self, xi12, img2, prior=None):
        """the per-pixel stage record, int32 [n, y_max, x_max, 16] (fields: RECORD)"""
        import torch

        b, single, n, xi, pr = self._call(xi12, img2, prior)
        rec = torch.empty((n, self.y_max, self.x_max, 16), dtype=torch.int32, device=self.device)
        self._enter()
        capi.check(capi.load().vg_motion_stereo_select(self._h, n, xi.ctypes.data_as(_dp), b.data_ptr(),
                                                       *[t.data_ptr() if t is not None else None for t in pr], rec.data_ptr()))
        self._leave(rec, b, *pr)
        return rec[0] if single else rec
