"""Plain numpy restatement of what the photometric mapping loop adds to the stages it calls (include/visgeom_amd.h section 16):
the host arithmetic of the reference's PhotometricMapping (src/localization/mapping.cpp: checkDistance, selectMapFrame, the tail
of localizePhoto), computeErr of its two programs (test/localization/map_test.cpp) with the saturation of DESIGN.md section 9,
and the state machine of feedImage itself with the stages replaced by callbacks -- tests/test_mapping_cpu.py runs it with "every
estimate is the truth".  Written from reading the reference; the pose algebra is tests/photometric_ref.py's."""
import numpy as np

from tests import mono_odom_ref as mr
from tests import photometric_ref as pr

DEFAULTS = dict(new_kf_distance_thresh=0.03, new_kf_angular_thresh=0.25, min_init_dist=0.1, min_stereo_base=0.07, dist_thresh=5.,
                normalize_scale=1, rotation_tolerance=0.005, min_scale_length=1e-2, min_scale_ratio=0.8, max_scale_ratio=1.2, num_scales=5)
SELECT_K = 4.
ZERO = np.zeros(6)
ACTIONS = ("FIRST", "WAITING", "INIT_SLAM", "INIT_LOCALIZE", "LOCALIZE_REFINED", "LOCALIZE_INTER_FRAME", "LOCALIZE_MAP_FRAME_CHANGED",
           "LOCALIZE_MAP_FRAME_KEPT", "LOCALIZE_LEFT_MAP", "SLAM_REFINED", "SLAM_INTER_FRAME", "SLAM_ENTERED_MAP")
WARNINGS = ("NONE", "SCALE", "ROTATION")


def squared(**kw):
    """DEFAULTS with overrides; the two new_kf thresholds are given unsquared, as the reference's JSON gives them"""
    p = dict(DEFAULTS)
    for k, v in kw.items():
        p[k] = float(v) ** 2 if k in ("new_kf_distance_thresh", "new_kf_angular_thresh") else v
    return p


def compose_inverse(a, b):
    """a o b^-1"""
    return pr.compose(a, mr.inverse(b))


def check_distance(prm, xi, K=1.):
    xi = np.asarray(xi, float)
    r = xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]
    d = xi[0] * xi[0] / 5 + xi[1] * xi[1] + xi[2] * xi[2]
    return bool(r < prm["new_kf_angular_thresh"] and d < prm["new_kf_distance_thresh"] * K)


def select_frame(prm, poses, xi, K=SELECT_K):
    res, best = -1, 1e15
    for i, pose in enumerate(poses):
        delta = pr.inverse_compose(xi, pose)
        if not check_distance(prm, delta, K):
            continue
        score = float(delta[3:] @ delta[3:] + delta[:3] @ delta[:3])
        if score < best:
            res, best = i, score
    return res


def normalize_scale(prm, old, prior, vo):
    """dict(xi, K, length, length_prior, rot_diff, warning) of localizePhoto's tail (mapping.cpp:420-459)"""
    out = dict(xi=np.array(vo, float), K=0., length=0., length_prior=0., rot_diff=0., warning="NONE")
    if not prm["normalize_scale"]:
        return out
    zeta_prior, zeta = pr.inverse_compose(old, prior), pr.inverse_compose(old, vo)
    out["length_prior"], out["length"] = float(np.linalg.norm(zeta_prior[:3])), float(np.linalg.norm(zeta[:3]))
    out["rot_diff"] = float(abs(zeta[5] - zeta_prior[5]))
    with np.errstate(all="ignore"):
        out["K"] = K = float(np.float64(out["length_prior"]) / np.float64(out["length"]))
    if out["rot_diff"] > prm["rotation_tolerance"]:
        out["xi"], out["warning"] = pr.compose(old, zeta_prior), "ROTATION"
    elif out["length"] > prm["min_scale_length"]:
        if K < prm["min_scale_ratio"] or K > prm["max_scale_ratio"]:
            out["xi"], out["warning"] = pr.compose(old, zeta_prior), "SCALE"
        else:
            out["xi"] = pr.compose(old, np.concatenate([zeta[:3] * K, zeta[3:]]))
    return out


def compute_err(base, warped):
    """computeErr: 0 where either pixel is 0, else 127 + base - warped, saturated to [0, 255] (the reference's conversion wraps)"""
    b, w = base.astype(np.int64), warped.astype(np.int64)
    return np.where((b == 0) | (w == 0), 0, np.clip(127 + b - w, 0, 255)).astype(np.uint8)


def alignment_sums(base, warped):
    """int64 [3]: compared pixels, sum |base - warped|, sum (base - warped)^2"""
    b, w = base.astype(np.int64), warped.astype(np.int64)
    both = (b != 0) & (w != 0)
    d = (b - w)[both]
    return np.array([both.sum(), np.abs(d).sum(), (d * d).sum()], np.int64)


class Loop:
    """feedOdometry / feedImage / reInit of mapping.cpp on the host.  The stages are the callbacks of `stages`:
        sparse(key, k)              the sparse increment between frames key and k (frame numbers as given to feed_image)
        photo(inter, k, start)      the photometric pose of frame k in inter frame `inter`'s base
        mi(inter, map_pose, start)  xiFrMap of localizeMI for inter frame `inter`
    and the loop keeps no image: frames are numbers.  What a frame did is returned as a dict."""

    def __init__(self, prm, xi_base_cam, stages):
        self.prm, self.xbc, self.stages = prm, np.asarray(xi_base_cam, float), stages
        self.state, self.warning, self.map_idx = "BEGIN", "NONE", -1
        self.local, self.old, self.xi_odom, self.zeta_odom = ZERO, ZERO, None, ZERO
        self.inter_xi, self.inter_frame = ZERO, None
        self.frames = []   # (pose, frame number)

    def feed_odometry(self, xi):
        if self.xi_odom is not None:
            self.local = mr.integrate(self.local, self.xi_odom, xi)
        self.xi_odom = np.array(xi, float)

    def reinit(self, xi):
        if self.state == "SLAM":
            self.frames.append((self.inter_xi, self.inter_frame))
        self.state, self.local, self.old, self.xi_odom = "BEGIN", np.array(xi, float), np.array(xi, float), None

    def select(self, xi, K=SELECT_K):
        return select_frame(self.prm, [f[0] for f in self.frames], xi, K)

    def push_inter_frame(self, k, rep):
        if self.state == "SLAM":
            self.frames.append((self.inter_xi, self.inter_frame))
        base = mr.camera_motion(self.xbc, self.local)
        if np.linalg.norm(base[:3]) > self.prm["min_stereo_base"]:
            rep["sgm"] = True
        elif self.state == "INIT":
            raise RuntimeError("INIT below min_stereo_base")
        self.inter_xi, self.inter_frame = pr.compose(self.inter_xi, self.local), k
        self.zeta_odom, self.local, self.old = self.local, ZERO, ZERO

    def improve_stereo(self, rep):
        base = mr.camera_motion(self.xbc, self.local)
        rep["refined"] = bool(np.linalg.norm(base[:3]) >= self.prm["min_stereo_base"])

    def localize_photo(self, k, rep):
        prior = self.local
        vo = self.stages["photo"](self.inter_frame, k, prior)
        n = normalize_scale(self.prm, self.old, prior, vo)
        self.local = n["xi"]
        if self.prm["normalize_scale"]:
            self.old, self.warning = self.local, n["warning"]
        rep.update({key: n[key] for key in ("K", "length", "length_prior", "rot_diff")})

    def localize_mi(self, rep):
        xi_map = self.frames[self.map_idx][0]
        out = self.stages["mi"](self.inter_frame, self.frames[self.map_idx], pr.inverse_compose(self.inter_xi, xi_map))
        self.inter_xi = compose_inverse(xi_map, out)
        rep["mi"] = True

    def feed_image(self, k):
        rep = dict(state_before=self.state, action="WAITING", map_index_before=self.map_idx, sgm=False, refined=False, mi=False, K=0., length=0.,
                   length_prior=0., rot_diff=0.)
        if self.state == "BEGIN":
            self.inter_xi, self.local, self.inter_frame = self.local, ZERO, k
            self.state, rep["action"] = "INIT", "FIRST"
        elif self.state == "INIT":
            if not np.linalg.norm(self.local[:3]) < self.prm["min_init_dist"]:
                self.local = self.stages["sparse"](self.inter_frame, k)
                self.push_inter_frame(k, rep)
                self.map_idx = self.select(self.inter_xi)
                if self.map_idx == -1:
                    self.state, rep["action"] = "SLAM", "INIT_SLAM"
                else:
                    self.state, rep["action"] = "LOCALIZE", "INIT_LOCALIZE"
                    self.localize_mi(rep)
        elif self.state == "LOCALIZE":
            self.localize_photo(k, rep)
            inter_ok = check_distance(self.prm, self.local)
            xi_map_fr = pr.inverse_compose(self.frames[self.map_idx][0], self.inter_xi)
            map_ok = check_distance(self.prm, pr.compose(xi_map_fr, self.local))
            if not map_ok:
                self.push_inter_frame(k, rep)
                old_idx, self.map_idx = self.map_idx, self.select(self.inter_xi)
                if self.map_idx != -1 and self.map_idx != old_idx:
                    rep["action"] = "LOCALIZE_MAP_FRAME_CHANGED"
                    self.localize_mi(rep)
                elif self.map_idx == -1:
                    self.state, rep["action"] = "SLAM", "LOCALIZE_LEFT_MAP"
                else:
                    rep["action"] = "LOCALIZE_MAP_FRAME_KEPT"
            elif not inter_ok:
                self.push_inter_frame(k, rep)
                rep["action"] = "LOCALIZE_INTER_FRAME"
                self.localize_mi(rep)
            else:
                rep["action"] = "LOCALIZE_REFINED"
                self.improve_stereo(rep)
        else:
            self.localize_photo(k, rep)
            if not check_distance(self.prm, self.local):
                self.push_inter_frame(k, rep)
                self.map_idx = self.select(self.inter_xi)
                rep["action"] = "SLAM_INTER_FRAME"
                if self.map_idx != -1:
                    self.state, rep["action"] = "LOCALIZE", "SLAM_ENTERED_MAP"
                    self.localize_mi(rep)
            else:
                rep["action"] = "SLAM_REFINED"
                self.improve_stereo(rep)
        rep.update(state=self.state, warning=self.warning, map_index=self.map_idx, frames=len(self.frames))
        return rep
