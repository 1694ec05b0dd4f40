"""Optimizer::PoseOptimization (ORB_SLAM2 Optimizer.cc:239-451) and the parts of its vendored g2o that it runs, restated in numpy float64 by reading:
OptimizationAlgorithmLevenberg::solve / computeLambdaInit / computeScale, SparseOptimizer::optimize / initializeOptimization(level) / activeRobustChi2 /
push / pop, BaseUnaryEdge::constructQuadraticForm, RobustKernelHuber, BlockSolver::setLambda, LinearSolverDense, the two ...OnlyPose edges,
VertexSE3Expmap::oplusImpl, SE3Quat (exp, map, operator*, normalizeRotation) and Converter::toSE3Quat / toCvMat.

NOT pinned against g2o: the reference cannot be built where this was written (g2o needs Eigen).  What pins it is tests/test_pose_opt_model.py: the
Jacobians against central differences of the model's own error, recovery of a known pose, a vanishing gradient at the result, the short-case rules.
Where Eigen's own operation order is not visible from g2o's sources (products inside constructQuadraticForm, LDLT's pivoting) the order here is the
plain one; orders of SUMS over edges are the model's `perm` argument, and their effect is what tests/golden/pose_opt_spread.npz records.

Points the restatement keeps (all from the sources above):
  * inputs are float, widened to double; invSigma2 is a float read from mvInvLevelSigma2; everything else is double; the pose comes out rounded to float;
  * the stereo edge's cam_project rounds 1/z to FLOAT (`const float invz = 1.0f/trans_xyz[2]`), the monocular one divides in double; the Jacobians of
    both use the double 1/z;
  * Huber delta = (float)sqrt(5.991) / (float)sqrt(7.815), dsqr = delta * delta in double; the classification compares (float)chi2 > 5.991f / 7.815f;
  * every round restarts from the initial pose; rounds carry only the levels; the kernel is off in the last round only;
  * a level-0 edge is classified by the error the round's last computeActiveErrors left - after a rejected last trial that is the REJECTED pose's error
    (pop() restores the estimate, not the errors); a level-1 edge gets a fresh computeError at the estimate;
  * robustInformation is rho_1 * Omega (the second-order term is commented out in this g2o); activeRobustChi2 sums rho_0;
  * lambda_0 = 1e-5 max|H_jj| at iteration 0 of every optimize(); a non-finite tempChi is a failed trial; Terminate on qmax == 10 or rho == 0; the added
    stop criterion (iniChi - currentChi) * 1e3 < iniChi three times running; a failed solve makes tempChi DBL_MAX and leaves x as it was;
  * fewer than 3 correspondences: 0, nothing written; fewer than 10 edges: one round; no level-0 edge: optimize() returns at once.
"""
import numpy as np

DELTA = (float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815))))        # mono, stereo
TH = (np.float32(5.991), np.float32(7.815))
DBL_MAX = np.finfo(np.float64).max
_IDX = [(j, k) for j in range(6) for k in range(j, 6)]                                 # the 21 upper entries of H, row by row


# ------------------------------------------------------------------------------------------------ SE3Quat: (q = x, y, z, w; t)
def quat_of_matrix(m):
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)
    if t > 0.0:
        t = np.sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t; q[1] = (m[0, 2] - m[2, 0]) * t; q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t; t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t; q[j] = (m[j, i] + m[i, j]) * t; q[k] = (m[k, i] + m[i, k]) * t
    return q


def normalize_rotation(q):
    if q[3] < 0:
        q = -q
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def rotate(q, X, Y, Z):
    """Eigen's Quaternion * Vector3 (works on arrays of points)"""
    ux = q[1] * Z - q[2] * Y; uy = q[2] * X - q[0] * Z; uz = q[0] * Y - q[1] * X
    ux = ux + ux; uy = uy + uy; uz = uz + uz
    return (X + q[3] * ux + (q[1] * uz - q[2] * uy), Y + q[3] * uy + (q[2] * ux - q[0] * uz), Z + q[3] * uz + (q[0] * uy - q[1] * ux))


def rotation_matrix(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def to_se3quat(Tcw):
    """Converter::toSE3Quat"""
    T = np.asarray(Tcw, np.float32).reshape(4, 4).astype(np.float64)
    return normalize_rotation(quat_of_matrix(T[:3, :3])), T[:3, 3].copy()


def to_cvmat(pose):
    """Converter::toCvMat(SE3Quat)"""
    q, t = pose
    M = np.eye(4)
    M[:3, :3] = rotation_matrix(q); M[:3, 3] = t
    return M.astype(np.float32)


def oplus(u, pose):
    """SE3Quat::exp(u) * pose, u = (omega, upsilon)"""
    ox, oy, oz = u[0], u[1], u[2]
    theta = np.sqrt(ox * ox + oy * oy + oz * oz)
    O = np.array([[0.0, -oz, oy], [oz, 0.0, -ox], [-oy, ox, 0.0]])
    O2 = np.array([[O[i, 0] * O[0, j] + O[i, 1] * O[1, j] + O[i, 2] * O[2, j] for j in range(3)] for i in range(3)])
    I = np.eye(3)
    if theta < 0.00001:
        R = (I + O) + O2; V = R
    else:
        a = np.sin(theta) / theta; c = (1.0 - np.cos(theta)) / (theta * theta); d = (theta - np.sin(theta)) / theta ** 3.0
        R = (I + a * O) + c * O2
        V = (I + c * O) + d * O2
    qe = quat_of_matrix(R)
    te = np.array([V[i, 0] * u[3] + V[i, 1] * u[4] + V[i, 2] * u[5] for i in range(3)])
    qe = normalize_rotation(qe)
    q2, t2 = pose
    rx, ry, rz = rotate(qe, t2[0], t2[1], t2[2])
    t = np.array([te[0] + rx, te[1] + ry, te[2] + rz])
    ax, ay, az, aw = qe; bx, by, bz, bw = q2
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])
    return normalize_rotation(q), t


# ------------------------------------------------------------------------------------------------ the edges
class Problem:
    """cam = (fx, fy, cx, cy, bf) float32; obs[n, 7] float32 = u, v, u_right (< 0: monocular), inv_sigma2, X, Y, Z"""

    def __init__(self, cam, obs):
        self.cam = np.asarray(cam, np.float32).astype(np.float64)
        o = np.asarray(obs, np.float32).reshape(-1, 7)
        self.n = len(o)
        self.stereo = ~(o[:, 2] < 0)
        self.o = o.astype(np.float64)


def errors(P, pose, float_invz=True):
    """computeError of every edge at pose: (e[n, 3] (third entry 0 on a monocular edge), chi2[n], camera-frame x, y, z).
    float_invz=False is the smooth function the analytic Jacobian differentiates (the stereo edge's float 1/z left in double)."""
    fx, fy, cx, cy, bf = P.cam
    q, t = pose
    o = P.o
    x, y, z = rotate(q, o[:, 4], o[:, 5], o[:, 6])
    x = x + t[0]; y = y + t[1]; z = z + t[2]
    w = o[:, 3]
    with np.errstate(all="ignore"):
        e = np.zeros((P.n, 3))
        e[:, 0] = o[:, 0] - (x / z * fx + cx)
        e[:, 1] = o[:, 1] - (y / z * fy + cy)
        invz = 1.0 / z
        if float_invz:
            invz = invz.astype(np.float32).astype(np.float64)
        pu = x * invz * fx + cx
        s = P.stereo
        e[s, 0] = (o[:, 0] - pu)[s]
        e[s, 1] = (o[:, 1] - (y * invz * fy + cy))[s]
        e[s, 2] = (o[:, 2] - (pu - bf * invz))[s]
        chi2 = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
        chi2 = np.where(s, chi2 + e[:, 2] * (w * e[:, 2]), chi2)
    return e, chi2, x, y, z


def jacobians(P, x, y, z):
    """linearizeOplus of both edge classes: A[n, 3, 6] (row 2 only meaningful on stereo edges)"""
    fx, fy, cx, cy, bf = P.cam
    with np.errstate(all="ignore"):
        invz = 1.0 / z; invz_2 = invz * invz
        A = np.zeros((len(x), 3, 6))
        A[:, 0, 0] = x * y * invz_2 * fx; A[:, 0, 1] = -(1.0 + (x * x * invz_2)) * fx; A[:, 0, 2] = y * invz * fx; A[:, 0, 3] = -invz * fx; A[:, 0, 5] = x * invz_2 * fx
        A[:, 1, 0] = (1.0 + y * y * invz_2) * fy; A[:, 1, 1] = -x * y * invz_2 * fy; A[:, 1, 2] = -x * invz * fy; A[:, 1, 4] = -invz * fy; A[:, 1, 5] = y * invz_2 * fy
        A[:, 2, 0] = A[:, 0, 0] - bf * y * invz_2; A[:, 2, 1] = A[:, 0, 1] + bf * x * invz_2; A[:, 2, 2] = A[:, 0, 2]; A[:, 2, 3] = A[:, 0, 3]; A[:, 2, 5] = A[:, 0, 5] - bf * invz_2
    return A


def evaluate(P, pose, active, robust, perm=None):
    """computeActiveErrors + activeRobustChi2 + buildSystem at pose over the level-0 edges: (H[21], b[6], chi).  The sums over edges run one edge after
    the other in index order, or in the order `perm` (a permutation of range(n)) gives."""
    e, chi2, x, y, z = errors(P, pose)
    A = jacobians(P, x, y, z)
    w = P.o[:, 3]
    with np.errstate(all="ignore"):
        rho0 = chi2.copy(); rho1 = np.ones(P.n)
        if robust:
            delta = np.where(P.stereo, DELTA[1], DELTA[0]); dsqr = delta * delta
            out = ~(chi2 <= dsqr)
            sq = np.sqrt(chi2)
            rho0 = np.where(out, 2.0 * sq * delta - dsqr, chi2); rho1 = np.where(out, delta / sq, 1.0)
        wr = rho1 * w
        s = P.stereo
        terms = np.zeros((P.n, 28))
        for c, (j, k) in enumerate(_IDX):
            t = (A[:, 0, j] * wr) * A[:, 0, k] + (A[:, 1, j] * wr) * A[:, 1, k]
            terms[:, c] = np.where(s, t + (A[:, 2, j] * wr) * A[:, 2, k], t)
        for j in range(6):
            g = A[:, 0, j] * (w * e[:, 0]) + A[:, 1, j] * (w * e[:, 1])
            terms[:, 21 + j] = rho1 * np.where(s, g + A[:, 2, j] * (w * e[:, 2]), g)
        terms[:, 27] = rho0
        order = np.arange(P.n) if perm is None else np.asarray(perm)
        order = order[active[order]]
        tot = np.cumsum(terms[order], axis=0)[-1] if len(order) else np.zeros(28)       # cumsum adds one row after the other (np.sum would add pairwise)
    return tot[:21].copy(), -tot[21:27], tot[27]


def solve(H, b, lam, x):
    """(H + lam I) x = b by LDL^T without pivoting; a negative pivot: (False, x unchanged)"""
    Hf = np.zeros((6, 6))
    for c, (j, k) in enumerate(_IDX):
        Hf[j, k] = Hf[k, j] = H[c]
    L = np.zeros((6, 6)); d = np.zeros(6); yv = np.zeros(6)
    with np.errstate(all="ignore"):
        for j in range(6):
            s = Hf[j, j] + lam
            for k in range(j):
                s -= L[j, k] * L[j, k] * d[k]
            d[j] = s
            if s < 0.0:
                return False, x
            for i in range(j + 1, 6):
                v = Hf[j, i]
                for k in range(j):
                    v -= L[i, k] * L[j, k] * d[k]
                L[i, j] = v / s
        for i in range(6):
            v = b[i]
            for k in range(i):
                v -= L[i, k] * yv[k]
            yv[i] = v
        xn = np.zeros(6)
        for i in range(5, -1, -1):
            v = yv[i] / d[i]
            for k in range(i + 1, 6):
                v -= L[k, i] * xn[k]
            xn[i] = v
    return True, xn


def optimize(P, init, active, robust, perm, trace):
    """setEstimate(init); initializeOptimization(0); optimize(10): (estimate, pose of the last computeActiveErrors)"""
    cur = last = init
    if not active.any():
        return cur, last
    H, b, chi = evaluate(P, cur, active, robust, perm)
    x = np.zeros(6)
    lam = ni = 0.0; n_bad = 0
    for it in range(10):
        last = cur; ini_chi = chi
        if it == 0:
            lam = 1e-5 * max(0.0, *(abs(H[_IDX.index((j, j))]) for j in range(6))); ni = 2.0; n_bad = 0
        rho = 0.0; qmax = 0
        for q in range(10):
            ok2, x = solve(H, b, lam, x)
            trial = oplus(x, cur); last = trial
            Ht, bt, temp_chi = evaluate(P, trial, active, robust, perm)
            if not ok2:
                temp_chi = DBL_MAX
            with np.errstate(all="ignore"):
                rho = chi - temp_chi
                scale = 0.0
                for j in range(6):
                    scale += x[j] * (lam * x[j] + b[j])
                scale += 1e-3
                rho = rho / scale
            if rho > 0 and np.isfinite(temp_chi):
                alpha = 1.0 - (2 * rho - 1) ** 3.0
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha); ni = 2.0
                chi = temp_chi; cur = trial; H, b = Ht, bt
                trace["accepted"] += 1
            else:
                lam *= ni; ni *= 2.0
                trace["rejected"] += 1
            qmax = q + 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            trace["terminate_trials"] += 1
            break
        n_bad = n_bad + 1 if (ini_chi - chi) * 1e3 < ini_chi else 0
        if n_bad >= 3:
            trace["three_strikes"] += 1
            break
    return cur, last


def classify(P, flags, cur, last, fresh=False):
    """(new flags, chi2 used per edge): level-1 edges at the estimate, level-0 edges at the pose of the round's last computeActiveErrors"""
    _, c_cur, _, _, _ = errors(P, cur)
    _, c_last, _, _, _ = errors(P, last)
    chi2 = c_cur if fresh else np.where(flags, c_cur, c_last)
    with np.errstate(all="ignore"):
        new = np.where(P.stereo, chi2.astype(np.float32) > TH[1], chi2.astype(np.float32) > TH[0])
    return new, chi2


def pose_optimization(cam, Tcw, obs, perm=None, want_trace=False):
    """Returns (Tcw float32 4x4, outlier bool[n], n_inliers) [, trace].  n < 3: (the input pose, no flag set, 0)."""
    P = Problem(cam, obs)
    Tcw = np.asarray(Tcw, np.float32).reshape(4, 4)
    trace = {"accepted": 0, "rejected": 0, "terminate_trials": 0, "three_strikes": 0, "round_ends_rejected": 0, "flags": [], "chi2": None, "stale_matters": False, "pose": None}
    if P.n < 3:
        r = (Tcw.copy(), np.zeros(P.n, bool), 0)
        return r + (trace,) if want_trace else r
    init = to_se3quat(Tcw)
    flags = np.zeros(P.n, bool)
    cur = init
    for rnd in range(4):
        cur, last = optimize(P, init, ~flags, rnd < 3, perm, trace)
        if last is not cur:
            trace["round_ends_rejected"] += 1
        new, chi2 = classify(P, flags, cur, last)
        if (classify(P, flags, cur, last, fresh=True)[0] != new).any():
            trace["stale_matters"] = True
        flags = new
        trace["flags"].append(flags.copy()); trace["chi2"] = chi2
        if P.n < 10:
            break
    trace["pose"] = cur
    r = (to_cvmat(cur), flags, int(P.n - flags.sum()))
    return r + (trace,) if want_trace else r


def last_round_gradient(cam, obs, pose, flags_before_last_round, robust):
    """b of the system the last round would build at pose (= minus half the gradient of its cost), and H's diagonal for scale"""
    P = Problem(cam, obs)
    H, b, _ = evaluate(P, pose, ~np.asarray(flags_before_last_round, bool), robust)
    return b, np.array([H[_IDX.index((j, j))] for j in range(6)])
