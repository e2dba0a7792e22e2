"""Calibration trajectory planning restated in numpy: TrajectoryVisualQuality (src/calibration/trajectory_generation.cpp:86-281)
with CircularTrajectory::compute (test/calibration/trajectory.cpp:27-82), on the Transformation / Quaternion / rotationMatrix
arithmetic of include/geometry and the EUCM projection and its Jacobian (include/projection/eucm.h).  Written from reading the
reference; loops as written there (corners summed one after the other, poses trajectory-major and step-ascending).

Every function takes its numbers in `dtype`.  With np.float64 the 6 x 6 inverses are numpy's (LAPACK's partial-pivot LU, what
Eigen's inverse() is) and the log-determinant comes from the singular values as in the reference; with np.longdouble, which
LAPACK does not take, the inverse is the Gauss-Jordan elimination below and the log-determinant a Cholesky factor's.  The spread
between the two is the restatement's own error.

Where the library departs from the reference ("Trajectory planning") this file follows the library: a pose
with a corner that does not project, or with a matrix whose inverse is not finite, is invalid and makes the cost +inf; every
trajectory reads its own odometry covariances."""
import json

import numpy as np

P = 5                      # parameters of one trajectory: x0, y0, theta0, d, alpha
DIFF_EPS = 1e-8
COV_ABS, COV_VW = 1e-2, 1e-4


def _a(v, dtype):
    return np.asarray(v, dtype=dtype)


def hat(v):
    z = v.dtype.type(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=v.dtype)


def quat(rot):
    """Quaternion(rot) (quaternion.h:31-50): [x, y, z, w]"""
    th = np.sqrt((rot * rot).sum())
    if abs(th) < 1e-6:
        return np.concatenate([rot / 2, [rot.dtype.type(1)]]).astype(rot.dtype)
    return np.concatenate([rot / th * np.sin(th / 2), [np.cos(th / 2)]]).astype(rot.dtype)


def quat_rotate(q, v):
    x, y, z, w = q
    t1, t2, t3, t4, t5, t6, t7, t8, t9 = w * x, w * y, w * z, -x * x, x * y, x * z, -y * y, y * z, -z * z
    return np.array([2 * ((t7 + t9) * v[0] + (t5 - t3) * v[1] + (t2 + t6) * v[2]) + v[0],
                     2 * ((t3 + t5) * v[0] + (t4 + t9) * v[1] + (t8 - t1) * v[2]) + v[1],
                     2 * ((t6 - t2) * v[0] + (t1 + t8) * v[1] + (t4 + t7) * v[2]) + v[2]], dtype=v.dtype)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], dtype=a.dtype)


def quat_inv(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], dtype=q.dtype)


def quat_to_rotvec(q):
    s = np.sqrt((q[:3] * q[:3]).sum())
    if s < 1e-5:
        return q[:3] * 2
    pi = q.dtype.type(np.pi)
    th = 2 * np.arctan2(s, q[3])
    if th > pi:
        th = th - 2 * pi
    elif th < -pi:
        th = th + 2 * pi
    return q[:3] / s * th


def rot_mat(v):
    """rotationMatrix(v) (geometry_core.h:40-76)"""
    th = np.sqrt((v * v).sum())
    one = v.dtype.type(1)
    if th < 1e-5:
        return np.array([[one, -v[2], v[1]], [v[2], one, -v[0]], [-v[1], v[0], one]], dtype=v.dtype)
    u = v * (one / th)
    s, c = np.sin(th), one - np.cos(th)
    return np.array([[one + c * (u[0] * u[0] - one), -s * u[2] + c * u[0] * u[1], s * u[1] + c * u[0] * u[2]],
                     [s * u[2] + c * u[1] * u[0], one + c * (u[1] * u[1] - one), -s * u[0] + c * u[1] * u[2]],
                     [-s * u[1] + c * u[2] * u[0], s * u[0] + c * u[2] * u[1], one + c * (u[2] * u[2] - one)]], dtype=v.dtype)


def compose(a, b):
    q1, q2 = quat(a[3:]), quat(b[3:])
    return np.concatenate([quat_rotate(q1, b[:3]) + a[:3], quat_to_rotvec(quat_mul(q1, q2))])


def inverse_compose(a, b):
    q1i, q2 = quat_inv(quat(a[3:])), quat(b[3:])
    return np.concatenate([quat_rotate(q1i, b[:3] - a[:3]), quat_to_rotvec(quat_mul(q1i, q2))])


def screw_transf_inv(xi):
    R = rot_mat(-xi[3:])
    L = np.zeros((6, 6), dtype=xi.dtype)
    L[:3, :3] = R
    L[:3, 3:] = -R @ hat(xi[:3])
    L[3:, 3:] = R
    return L


def inverse(A):
    """float64: LAPACK; otherwise Gauss-Jordan with partial pivoting"""
    if A.dtype == np.float64:
        with np.errstate(all="ignore"):
            try:
                return np.linalg.inv(A)
            except np.linalg.LinAlgError:
                return np.full_like(A, np.nan)
    n = A.shape[0]
    M = np.concatenate([A.copy(), np.eye(n, dtype=A.dtype)], axis=1)
    with np.errstate(all="ignore"):
        for k in range(n):
            p = k + int(np.argmax(np.abs(M[k:, k])))
            M[[k, p]] = M[[p, k]]
            M[k] = M[k] / M[k, k]
            for r in range(n):
                if r != k:
                    M[r] = M[r] - M[r, k] * M[k]
    return M[:, n:]


def neg_log_det(H):
    """-sum log sigma_k(H).  float64: the singular values; otherwise twice the logs of a Cholesky factor's diagonal"""
    if H.dtype == np.float64:
        return -np.log(np.linalg.svd(H, compute_uv=False)).sum()
    n = H.shape[0]
    L = np.zeros_like(H)
    for j in range(n):
        L[j, j] = np.sqrt(H[j, j] - (L[j, :j] * L[j, :j]).sum())
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return -2 * np.log(np.diag(L)).sum()


def eucm_project(cam, X):
    """(uv, ok): EnhancedProjector (eucm.h:29-63)"""
    alpha, beta, fu, fv, u0, v0 = cam
    x, y, z = X
    one = X.dtype.type(1)
    rho = np.sqrt(z * z + beta * (x * x + y * y))
    eta = alpha * rho + (one - alpha) * z
    with np.errstate(all="ignore"):
        uv = np.array([fu * (x / eta) + u0, fv * (y / eta) + v0], dtype=X.dtype)
        ok = not eta < 1e-3
        if ok and alpha > 0.5 and z / eta < (alpha - one) / (alpha + alpha - one):
            ok = False
    return uv, ok


def eucm_jacobian(cam, X):
    """projectionJacobian (eucm.h:115-167): rows du/dX, dv/dX of a point that projects"""
    alpha, beta, fu, fv, u0, v0 = cam
    x, y, z = X
    one = X.dtype.type(1)
    rho = np.sqrt(z * z + beta * (x * x + y * y))
    gamma = one - alpha
    eta = alpha * rho + gamma * z
    k = one / eta / eta
    abrho = alpha * beta / rho
    Jxy = k * abrho * x * y
    Jz = k * (gamma + alpha * z / rho)
    Jx = gamma * z + alpha * rho
    return np.array([[fu * k * (Jx - abrho * x * x), -fu * Jxy, -fu * x * Jz],
                     [-fv * Jxy, fv * k * (Jx - abrho * y * y), -fv * y * Jz]], dtype=X.dtype)


def trajectory(params, steps, dtype=np.float64):
    """CircularTrajectory::compute: (xi [steps, 6], cov [steps, 6, 6])"""
    p = _a(params, dtype)
    dist, alpha = p[3], p[4]
    half = dtype(0.5)
    ca, sa = np.cos(alpha * half), np.sin(alpha * half)
    z = dtype(0)
    xi0 = np.array([p[0], p[1], z, z, z, p[2]], dtype=dtype)
    dxi = np.array([-dist * sa, dist * ca, z, z, z, alpha], dtype=dtype)
    dxidu = np.zeros((6, 2), dtype=dtype)
    dxidu[0] = [-sa, -dist / 2 * ca]
    dxidu[1] = [ca, -dist / 2 * sa]
    dxidu[5, 1] = 1
    cov_abs = np.eye(6, dtype=dtype) * dtype(COV_ABS)
    cov_incr = dxidu @ (np.eye(2, dtype=dtype) * dtype(COV_VW)) @ dxidu.T
    L = screw_transf_inv(dxi)
    xi, cov = [xi0], [cov_abs]
    cov_odom = cov_incr
    for _ in range(1, steps):
        xi.append(compose(xi[-1], dxi))
        cov_odom = L @ cov_odom @ L.T + cov_incr
        cov.append(cov_odom + cov_abs)
    return np.array(xi), np.array(cov)


class Quality:
    """TrajectoryVisualQuality.  camera: 6 EUCM intrinsics; quality: the "quality_parameters" object of a plan file; steps: the
    number of poses of every trajectory."""

    def __init__(self, camera, width, height, quality, steps, dtype=np.float64):
        self.dtype = dtype
        self.cam = _a(camera, dtype)
        self.width, self.height = dtype(width), dtype(height)
        self.xi_cam = _a(quality["xiBaseCam"], dtype)
        self.xi_board = _a(quality["xiOrigBoard"], dtype)
        self.kappa_max = dtype(1) / dtype(quality["turn_radius"])
        self.nx, self.ny = int(quality["board"]["cols"]), int(quality["board"]["rows"])
        step = dtype(quality["board"]["step"])
        self.board = np.array([[step * i, step * j, 0] for j in range(self.ny) for i in range(self.nx)], dtype=dtype)
        self.min_dist = dtype(quality["min_camera_dist"])
        self.margin = dtype(quality["min_margin"])
        self.min_cell = dtype(quality["min_cell_size"])
        self.hess_prior = np.diag(dtype(1) / _a(quality["prior_variance"], dtype))
        self.stiffness = np.sqrt(dtype(1) / dtype(quality["feature_variance"]))   # both diagonal entries of the LLT's matrixU
        self.steps = [int(s) for s in steps]

    def board_in_camera(self, cam_pose):
        xi = inverse_compose(_a(cam_pose, self.dtype), self.xi_board)
        return xi, self.board @ rot_mat(xi[3:]).T + xi[:3]

    def visual_cov(self, cam_pose):
        """(cov, JtJ, JtCJ, valid)"""
        dt = self.dtype
        _, pts = self.board_in_camera(cam_pose)
        JtJ, JtCJ = np.zeros((6, 6), dtype=dt), np.zeros((6, 6), dtype=dt)
        valid = True
        for X in pts:
            _, ok = eucm_project(self.cam, X)
            if not ok:
                valid = False
                continue
            dxdxi = np.concatenate([-np.eye(3, dtype=dt), hat(X)], axis=1)
            dpdxi = eucm_jacobian(self.cam, X) @ dxdxi
            JtJ += dpdxi.T @ dpdxi
            JtCJ += (dpdxi.T * self.stiffness) @ dpdxi
        inf = np.full((6, 6), np.inf, dtype=dt)
        if not valid:
            return inf, inf, JtCJ, False
        inv = inverse(JtCJ)
        cov = inv.T @ JtJ @ inv
        if not np.isfinite(cov).all():
            return inf, inf, JtCJ, False
        return cov, JtJ, JtCJ, True

    def projections(self, cam_pose):
        """(uv [N, 2], ok [N])"""
        _, pts = self.board_in_camera(cam_pose)
        res = [eucm_project(self.cam, X) for X in pts]
        return np.array([r[0] for r in res]), np.array([r[1] for r in res])

    def image_limits_cost(self, cam_pose):
        dt = self.dtype
        uv, _ = self.projections(cam_pose)
        center = self.cam[4:6]
        r = (self.cam[4] + self.cam[5]) / 2
        zero, ten = dt(0), dt(10)
        res = zero
        for pt in uv:
            dx = max(self.margin - min(pt[0], self.width - pt[0]), zero)
            dy = max(self.margin - min(pt[1], self.height - pt[1]), zero)
            dr = max(np.sqrt(((pt - center) ** 2).sum()) - r, zero)
            res += (max(dx, max(dy, dr)) / ten) ** 2
        nx, ny = self.nx, self.ny
        for i in range(nx - 1):
            for j in range(ny):
                d = uv[nx * j + i] - uv[nx * j + i + 1]
                res += (max(self.min_cell - np.sqrt((d * d).sum()), zero) / ten) ** 2
        for i in range(nx):
            for j in range(ny - 1):
                d = uv[nx * j + i] - uv[nx * (j + 1) + i]
                res += (max(self.min_cell - np.sqrt((d * d).sum()), zero) / ten) ** 2
        return res

    def curvature_cost(self, xi1, xi2):
        zeta = inverse_compose(xi1, xi2)
        v, w = np.sqrt((zeta[:3] ** 2).sum()), np.sqrt((zeta[3:] ** 2).sum())
        with np.errstate(all="ignore"):
            return (max(self.dtype(0), w / v - self.kappa_max) * 10) ** 2

    def distance_cost(self, cam_pose):
        xi, _ = self.board_in_camera(cam_pose)
        return max(self.min_dist - np.sqrt((xi[:3] ** 2).sum()), self.dtype(0)) ** 2

    def normal_cost(self, cam_pose):
        xi, _ = self.board_in_camera(cam_pose)
        ez = rot_mat(xi[3:])[:, 2]
        d = xi[:3] / np.sqrt((xi[:3] ** 2).sum())
        cr = np.array([d[1] * ez[2] - d[2] * ez[1], d[2] * ez[0] - d[0] * ez[2], d[0] * ez[1] - d[1] * ez[0]], dtype=self.dtype)
        return (max(np.sqrt((cr * cr).sum()) - self.dtype(np.pi) / 6, self.dtype(0)) * 10) ** 2

    def camera_poses(self, params):
        """the camera poses xiOdom_i o xiCam of every pose i >= 1, trajectory-major"""
        p = _a(params, self.dtype)
        out = []
        for t, n in enumerate(self.steps):
            xi, _ = trajectory(p[P * t:P * t + P], n, self.dtype)
            out += [compose(xi[i], self.xi_cam) for i in range(1, n)]
        return np.array(out)

    def evaluate(self, params, detail=False):
        """(cost, terms [information, image limits, curvature, distance, normal], invalid poses); detail=True adds a list with
        one dict per pose"""
        dt = self.dtype
        p = _a(params, dt)
        H = self.hess_prior.copy()
        res = dt(0)
        pen = np.zeros(4, dtype=dt)
        invalid = 0
        poses = []
        I6 = np.eye(6, dtype=dt)
        L_cam = screw_transf_inv(self.xi_cam)
        for t, n in enumerate(self.steps):
            xi, cov = trajectory(p[P * t:P * t + P], n, dt)
            for i in range(1, n):
                cam_pose = compose(xi[i], self.xi_cam)
                V, JtJ, JtCJ, ok = self.visual_cov(cam_pose)
                C = V + L_cam @ cov[i] @ L_cam.T
                Cinv = inverse(C) if ok else C
                ok = ok and bool(np.isfinite(Cinv).all())
                if not ok:
                    invalid += 1
                    poses.append(dict(valid=False))
                    continue
                J = screw_transf_inv(inverse_compose(self.xi_cam, inverse_compose(xi[0], cam_pose))) - I6
                H += J.T @ Cinv @ J
                four = [self.image_limits_cost(cam_pose), self.curvature_cost(xi[i - 1], xi[i]), self.distance_cost(cam_pose),
                        self.normal_cost(cam_pose)]
                for k in range(4):
                    res += four[k]
                    pen[k] += four[k]
                poses.append(dict(valid=True, penalties=four, JtCJ=JtCJ, C=C))
        if invalid:
            inf = dt(np.inf)
            out = (inf, np.concatenate([[inf], pen]), invalid)
        else:
            info = neg_log_det(H)
            out = (res + info, np.concatenate([[info], pen]), 0)
        return out + (poses,) if detail else out

    def gradient_points(self, params):
        """(points [2 P T, P T], delta [P T]) in float64 exactly as Evaluate forms them: row 2 i is orig_i + delta_i, row
        2 i + 1 orig_i - delta_i"""
        p = np.asarray(params, dtype=np.float64)
        delta = np.maximum(np.abs(p) * DIFF_EPS, DIFF_EPS * DIFF_EPS)
        pts = np.repeat(p[None], 2 * p.size, axis=0)
        for i in range(p.size):
            pts[2 * i, i] = p[i] + delta[i]
            pts[2 * i + 1, i] = p[i] - delta[i]
        return pts, delta

    def gradient(self, params):
        """central differences of evaluate() at the float64 points of gradient_points(): (gradient, delta)"""
        pts, delta = self.gradient_points(params)
        c = np.array([self.evaluate(q)[0] for q in pts], dtype=self.dtype)
        return (c[0::2] - c[1::2]) / (2 * _a(delta, self.dtype)), delta


def load_plan(path):
    """(camera, width, height, quality, steps, start) of a plan file in the program's format"""
    with open(path) as fh:
        root = json.load(fh)
    names = []
    while "trajectory%d" % (len(names) + 1) in root:
        names.append("trajectory%d" % (len(names) + 1))
    start = [root[n][k] for n in names for k in ("x_0", "y_0", "theta_0", "v", "w")]
    steps = [root[n]["number_steps"] for n in names]
    return root["camera_params"], root["camera_width"], root["camera_height"], root["quality_parameters"], steps, start
