"""What the create functions of the pipelines on a depth grid refuse before HIP is touched, through the C ABI: one table of
ScaleParameters and camera inputs against vg_stereo_create, vg_motion_stereo_create, vg_depth_fusion_create,
vg_photometric_create and vg_dense_ba_create, which share the grid check (vgsh::scaled_grid) and the camera check
(vgsh::check_camera) of csrc/vg_stereo_host.hpp.  Per entry and row: the return code, a NULL handle and the text of
vg_last_error().  The codes were recorded from the library before the checks were shared; an accepted row gets as far as the
device ("no CPU fallback" without one, a handle with one), and the set of accepted rows per entry is that library's: uMax = 0
without equal_margins is accepted by the two entries that take the image size as an argument and refused by the other three."""
import ctypes
import math

import numpy as np
import pytest

from tests import stereo_scene

_dp = ctypes.POINTER(ctypes.c_double)
XBC = [0.01, -0.02, 0.03, 0.004, -0.005, 0.006]
GOOD = dict(scale=2, u0=15, v0=15, u_max=125, v_max=93, x_max=40, y_max=30, equal_margins=0, disp_max=32)

# row -> (changes of the parameters, changes of the arguments)
ROWS = {
    "plain": ({}, {}),
    "equal_margins": (dict(equal_margins=1), {}),
    "scale=0": (dict(scale=0), {}),
    "scale=16385": (dict(scale=16385), {}),
    "u0=16385": (dict(u0=16385), {}),
    "v0=-16385": (dict(v0=-16385), {}),
    "u_max=0": (dict(u_max=0), {}),
    "u_max=0,equal_margins": (dict(u_max=0, equal_margins=1), {}),
    "v_max=16385": (dict(v_max=16385), {}),
    "v_max=16385,equal_margins": (dict(v_max=16385, equal_margins=1), {}),
    "grid=0": (dict(x_max=0), {}),
    "grid=0,equal_margins": (dict(u_max=28, equal_margins=1), {}),            # (28 - 30) / 2 + 1
    "grid=16385": (dict(y_max=16385), {}),
    "grid=16385,equal_margins": (dict(scale=1, v0=0, v_max=16384, equal_margins=1), {}),
    "camera=nan": ({}, dict(cam=[0.6, math.nan, 62., 61., 62.5, 46.5])),
    "camera=inf": ({}, dict(cam=[0.6, 1.05, 62., 61., math.inf, 46.5])),
    "fu=0": ({}, dict(cam=[0.6, 1.05, 0., 61., 62.5, 46.5])),
    "fv=0": ({}, dict(cam=[0.6, 1.05, 62., 0., 62.5, 46.5])),
    "out=NULL": ({}, dict(out=None)),
    "camera=NULL": ({}, dict(cam=None)),
    "params=NULL": ({}, dict(params=None)),
}
ENTRIES = ("stereo", "motion_stereo", "depth_fusion", "photometric", "dense_ba")
ACCEPTED = "accepted"
INVALID = 1   # capi.ERR_INVALID_ARGUMENT

# row -> what every entry answers: ACCEPTED or the text of vg_last_error(); every refusal is ERR_INVALID_ARGUMENT
COMMON = {
    "plain": ACCEPTED,
    "equal_margins": ACCEPTED,
    "scale=0": "scale must be in [1, 16384]",
    "scale=16385": "scale must be in [1, 16384]",
    "u0=16385": "|u0|, |v0| must be at most 16384",
    "v0=-16385": "|u0|, |v0| must be at most 16384",
    "u_max=0": "uMax / vMax must be in [1, 16384]",
    "u_max=0,equal_margins": "uMax / vMax must be in [1, 16384]",
    "v_max=16385": "uMax / vMax must be in [1, 16384]",
    "v_max=16385,equal_margins": "uMax / vMax must be in [1, 16384]",
    "grid=0": "the scaled image is empty: xMax < 1 or yMax < 1",
    "grid=0,equal_margins": "the scaled image is empty: xMax < 1 or yMax < 1",
    "grid=16385": "xMax / yMax must be at most 16384",
    "grid=16385,equal_margins": "xMax / yMax must be at most 16384",
    "camera=nan": "camera parameters must be finite",
    "camera=inf": "camera parameters must be finite",
    "fu=0": "fu, fv must be non-zero",
    "fv=0": "fu, fv must be non-zero",
    "out=NULL": "NULL output",
    "camera=NULL": "NULL argument",
    "params=NULL": "NULL argument",
}
# where an entry answers otherwise: the image size is an argument of the last two, which read uMax / vMax under equal_margins only
IMAGE_SIZE_ARGUMENT = {"u_max=0": ACCEPTED, "v_max=16385": ACCEPTED}
PAIR = {"camera=nan": "camera parameters and transformation must be finite", "camera=inf": "camera parameters and transformation must be finite"}
EXPECTED = {"stereo": dict(COMMON, **PAIR), "motion_stereo": COMMON, "depth_fusion": COMMON,
            "photometric": dict(COMMON, **IMAGE_SIZE_ARGUMENT), "dense_ba": dict(COMMON, **IMAGE_SIZE_ARGUMENT)}


def call(lib, entry, row):
    """-> (code, handle, text)"""
    from visgeom_amd import motion_stereo, stereo

    changes, args = ROWS[row]
    kw = dict(GOOD)
    kw.update(changes)
    p = motion_stereo.make_params(**kw) if entry == "motion_stereo" else stereo.make_params(**kw)
    h = ctypes.c_void_p()
    out = ctypes.byref(h) if "out" not in args else None
    cam = args.get("cam", stereo_scene.CAM1)
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (cam if cam is not None else [0.] * 6, stereo_scene.CAM2, stereo_scene.RIGS["sideways"], XBC)]
    c1, c2, xi, xbc = [a.ctypes.data_as(_dp) for a in keep]
    if cam is None:
        c1 = None
    prm = ctypes.byref(p) if "params" not in args else None
    if entry == "stereo":
        rc = lib.vg_stereo_create(out, 0, None, c1, c2, xi, prm)
    elif entry == "motion_stereo":
        rc = lib.vg_motion_stereo_create(out, 0, None, c1, c2, prm)
    elif entry == "depth_fusion":
        rc = lib.vg_depth_fusion_create(out, 0, None, c1, prm)
    elif entry == "photometric":
        rc = lib.vg_photometric_create(out, 0, None, c1, prm, xbc, 125, 93, 3)
    else:
        rc = lib.vg_dense_ba_create(out, 0, None, c1, prm, xbc, 125, 93, None)
    return rc, h, lib.vg_last_error().decode()


@pytest.mark.parametrize("entry", ENTRIES)
def test_create_refusals(entry):
    from visgeom_amd import capi

    lib = capi.load()
    assert INVALID == capi.ERR_INVALID_ARGUMENT
    assert set(EXPECTED[entry]) == set(ROWS)
    for row, want in EXPECTED[entry].items():
        rc, h, text = call(lib, entry, row)
        print(entry, row, rc, repr(text))
        if want != ACCEPTED:
            assert (rc, h.value, text) == (INVALID, None, want), (entry, row)
        elif lib.vg_device_count() == 0:   # as far as the device
            assert rc == capi.ERR_NO_DEVICE and not h.value and "no CPU fallback" in text, (entry, row, rc, text)
        else:
            assert rc == capi.OK and h.value, (entry, row, rc, text)
            getattr(lib, "vg_%s_destroy" % entry)(h)
