"""The inputs of the dense_ba tests, on tests/photometric_scene.py's 256 x 192 scene and its scale-2 depth grid (9153 cells).
Two key frames' worth of maps:
  solve case   the true range times 1 + 0.03 N(0, 1) (seed 7), sigma0 = 0.03 d0, frames = the scene's targets, start poses
               start_pose(f, 0.1): 2.8 mm / 0.88 mrad off the truth, where compute_pose leaves a pose
  pack case    photometric_scene's own depth map (holes, far values, values below MIN_DEPTH) with a sigma map of which some
               entries are 0, negative or NaN
and the scale-1 grid (49 152 cells) of the launch-shape and reference-settings tests.  Everything is built once and left unchanged."""
import numpy as np

from tests import dense_ba_ref as br
from tests import photometric_scene as ps
from tests import stereo_scene

NOISE, SEED = 0.03, 7
PRM1 = {"scale": 1, "u0": 0, "v0": 0, "x_max": ps.W, "y_max": ps.H}
_CACHE = {}


def true_range(prm=ps.PRM):
    """the true range at every cell of the grid, 0 where the ray meets nothing"""
    key = ("range", prm["scale"])
    if key not in _CACHE:
        yy, xx = np.mgrid[0:prm["y_max"], 0:prm["x_max"]]
        d = stereo_scene.reconstruct_np(ps.CAM, (xx * prm["scale"] + prm["u0"]).astype(float), (yy * prm["scale"] + prm["v0"]).astype(float))
        rng = stereo_scene.cast(np.zeros(3), d) * np.linalg.norm(d, axis=-1)
        _CACHE[key] = np.ascontiguousarray(np.where(np.isfinite(rng), rng, 0.))
    return _CACHE[key]


def maps(prm=ps.PRM):
    """(depth, sigma) of the solve case on the grid prm"""
    key = ("maps", prm["scale"])
    if key not in _CACHE:
        noise = np.random.default_rng(SEED).standard_normal(true_range(prm).shape)
        depth = np.ascontiguousarray(true_range(prm) * (1. + NOISE * noise))
        _CACHE[key] = (depth, np.ascontiguousarray(NOISE * depth))
    return _CACHE[key]


def pack_maps():
    """(depth, sigma) of the pack case"""
    if "pack_maps" not in _CACHE:
        depth = ps.scene()["depth"]
        pick = np.random.default_rng(13).random(depth.shape)
        sigma = 0.03 * np.where(depth > 0, depth, 1.)
        sigma[pick < 0.02] = 0.
        sigma[(pick >= 0.02) & (pick < 0.04)] = -0.1
        sigma[(pick >= 0.04) & (pick < 0.05)] = np.nan
        _CACHE["pack_maps"] = (depth, np.ascontiguousarray(sigma))
    return _CACHE["pack_maps"]


def frames(F):
    """F frames: the scene's three targets, cyclically"""
    t = ps.scene()["targets"]
    return np.ascontiguousarray(np.stack([t[f % 3] for f in range(F)]))


def start_poses(F, factor=0.1):
    """start_pose(f, factor) per frame; past the third frame the targets repeat at other offsets (factor (1 + f // 3))"""
    return np.array([ps.start_pose(f % 3, factor * (1 + f // 3)) for f in range(F)])


def problem(F, prm=ps.PRM, which="solve", **options):
    """the restatement on one of the cases with F frames, built once"""
    key = ("problem", F, prm["scale"], which, tuple(sorted(options.items())))
    if key not in _CACHE:
        p = br.Problem(ps.CAM, prm, ps.XI_BASE_CAM, **options)
        depth, sigma = maps(prm) if which == "solve" else pack_maps()
        p.set_base(ps.scene()["base"], depth, sigma)
        p.set_frames(list(frames(F)))
        _CACHE[key] = p
    return _CACHE[key]


def exact(m, F=2):
    """the solve case cut down to exactly m pack points: a run of m of the pack's cells from the middle of the pack keeps its
    depth, every other cell gets 0 (tests/localization_shapes.exact's construction)"""
    key = ("exact", m, F)
    if key not in _CACHE:
        full = problem(F)
        depth, sigma = maps()
        cells = full.pack["idx"]
        first = (len(cells) - m) // 2
        cut = np.zeros_like(depth)
        keep = cells[first:first + m]
        cut.flat[keep] = depth.flat[keep]
        p = br.Problem(ps.CAM, ps.PRM, ps.XI_BASE_CAM)
        p.set_base(ps.scene()["base"], cut, sigma)
        p.set_frames(list(frames(F)))
        assert len(p.pack["idx"]) == m
        _CACHE[key] = p
    return _CACHE[key]


def errors(xi, depths, pack, prm=ps.PRM):
    """(largest translation error in metres, largest rotation error in radians over the frames, median relative depth error)"""
    e = [ps.pose_error(x, f % 3) for f, x in enumerate(np.asarray(xi).reshape(-1, 6))]
    truth = true_range(prm).ravel()[pack["idx"]]
    return max(t for t, _ in e), max(r for _, r in e), float(np.median(np.abs(depths - truth) / truth))


def reference_solve(F, factor=0.1, **options):
    """the restatement's solve of the solve case from start_poses(F, factor), cached"""
    key = ("solved", F, factor, tuple(sorted(options.items())))
    if key not in _CACHE:
        _CACHE[key] = problem(F, **options).solve(start_poses(F, factor))
    return _CACHE[key]
