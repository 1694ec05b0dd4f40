"""Optimizer::OptimizeSim3 (ORB_SLAM2 Optimizer.cc:1046-1241) and the parts of its vendored g2o that it runs, restated in float64 by reading:
g2o::Sim3 (both constructors that take a rotation, the exponential Sim3(Vector7d) with its four branches, map, inverse, operator*),
VertexSim3Expmap::oplusImpl / cam_map1 / cam_map2, project, EdgeSim3ProjectXYZ::computeError and EdgeInverseSim3ProjectXYZ::computeError,
BaseBinaryEdge::linearizeOplus (the NUMERICAL Jacobian: neither edge type defines its own) and constructQuadraticForm with a fixed first vertex,
RobustKernelHuber, and the Levenberg-Marquardt driver as tests/pose_opt_model.py restates it (OptimizationAlgorithmLevenberg::solve,
SparseOptimizer::optimize, LinearSolverDense).

NOT pinned against g2o: the reference cannot be built where this was written (g2o needs Eigen).  What pins it is tests/test_sim3_opt_model.py: the
numerical Jacobians against the closed-form derivative of the model's own error, recovery of a known Sim3, a vanishing gradient at the result, the fixed
scale, the early return, the unnormalised quaternion.  Where Eigen's own operation order is not visible from g2o's sources the order here is the plain one.
On a machine with Eigen: build Optimizer.cc + g2o, record S12, flags and returns for the cases of tests/sim3_opt_cases.py and make this file reproduce them
(DESIGN.md section 9, item 11).

Points the restatement keeps (all from the sources above):
  * the pairs and the cameras are float, widened to double; the information is the float invSigma2 widened; S12 is double and is taken as given:
    neither Sim3(Quaterniond, ...) nor Sim3(Matrix3d, ...) nor operator* normalises the quaternion; inverse() is built from the conjugate;
  * every pair has a forward edge obs1 - cam_map1(project(S12.map(X2))) and an inverse edge obs2 - cam_map2(project(S12.inverse().map(X1))), active in that
    order; both carry a Huber kernel of delta (double)(float)sqrt(th2) in BOTH phases;
  * Jacobian column d = scalar * (e(Sim3(+delta e_d) * estimate) - e(Sim3(-delta e_d) * estimate)), delta = 1e-9, scalar = 1.0 / (2 * delta); every
    last-bit difference of a perturbed transform is multiplied by 5e8; _error is restored afterwards;
  * fix_scale: oplusImpl sets update[6] = 0 in the CALLER's array before Sim3(update): column 6 of every Jacobian is exactly 0, H66 is lambda alone, the
    solver's x[6] is 0 when computeScale reads it, and the scale keeps its bits (exp(0) * s);
  * optimize(5); a pair is removed as a whole if either edge's chi2 > (double)th2, read from the errors the phase's last computeActiveErrors left (after a
    rejected last trial: the REJECTED estimate's errors); optimize(10) if a pair was removed, optimize(5) otherwise; the estimate is NOT reset between the
    phases; fewer than 10 pairs left after the first check: return 0 with g2oS12 untouched; the second check removes matches and counts the rest;
  * the LM driver's points are those of tests/pose_opt_model.py: lambda_0 = 1e-5 max|H_jj| at iteration 0 of every optimize(); a non-finite tempChi is a
    failed trial; Terminate on qmax == 10 or rho == 0; the stop criterion (iniChi - currentChi) * 1e3 < iniChi three times running; a failed solve makes
    tempChi DBL_MAX and leaves x as it was.

exp / sin / cos are math's (the C library's), called once per Sim3(update).  `perm` is the order of the sums over the 2n edges (edge 2i: pair i's forward
edge, 2i + 1: its inverse edge); `tree` = T replaces it by the kernel's own order at workgroup size T (_sum_rows).  `jitter` (a seed, or None) moves each result of exp / sin / cos by -1, 0 or +1 ulp, drawn per call; exp(0) = 1, exact in every library, stays."""
import math

import numpy as np

DBL_MAX = np.finfo(np.float64).max
DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
_IDX = [(j, k) for j in range(7) for k in range(j, 7)]                                 # the 28 upper entries of H, row by row
_DIAG = [_IDX.index((j, j)) for j in range(7)]


class Jitter:
    def __init__(self, seed=None):
        self.rng = None if seed is None else np.random.default_rng(seed)

    def __call__(self, f, x):
        v = f(x)
        if self.rng is None or (f is math.exp and x == 0.0):
            return v
        k = int(self.rng.integers(-1, 2))
        return v if k == 0 else float(np.nextafter(v, math.inf if k > 0 else -math.inf))


NO_JITTER = Jitter()


# ------------------------------------------------------------------------------------------------ g2o::Sim3: (q = x, y, z, w; t; s)
def quat_of_matrix(m):
    """Eigen's Quaternion(Matrix3); nothing normalises the result"""
    t = m[0][0] + m[1][1] + m[2][2]
    q = [0.0] * 4
    if t > 0.0:
        t = math.sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t
        q[0] = (m[2][1] - m[1][2]) * t; q[1] = (m[0][2] - m[2][0]) * t; q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t; t = 0.5 / t
        q[3] = (m[k][j] - m[j][k]) * t; q[j] = (m[j][i] + m[i][j]) * t; q[k] = (m[k][i] + m[i][k]) * t
    return tuple(q)


def sim3_of_matrix(R, t, s):
    """Sim3(const Matrix3d&, const Vector3d&, double): LoopClosing.cc:325 calls it with Converter::toMatrix3d of a float matrix"""
    R = np.asarray(R, np.float64)
    return (quat_of_matrix([[float(R[i, j]) for j in range(3)] for i in range(3)]), tuple(float(v) for v in t), float(s))


def rotate(q, X, Y, Z):
    """Eigen's Quaternion * Vector3 (scalars or arrays of points)"""
    ux = q[1] * Z - q[2] * Y; uy = q[2] * X - q[0] * Z; uz = q[0] * Y - q[1] * X
    ux = ux + ux; uy = uy + uy; uz = uz + uz
    return (X + q[3] * ux + (q[1] * uz - q[2] * uy), Y + q[3] * uy + (q[2] * ux - q[0] * uz), Z + q[3] * uz + (q[0] * uy - q[1] * ux))


def smap(S, X, Y, Z):
    """Sim3::map: s * (r * xyz) + t"""
    q, t, s = S
    x, y, z = rotate(q, X, Y, Z)
    return s * x + t[0], s * y + t[1], s * z + t[2]


def inverse(S):
    """Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)"""
    q, t, s = S
    qc = (-q[0], -q[1], -q[2], q[3])
    k = -1.0 / s
    return (qc, rotate(qc, k * t[0], k * t[1], k * t[2]), 1.0 / s)


def mul(A, B):
    """Sim3::operator*: r = r1 * r2 (not normalised), t = s1 * (r1 * t2) + t1, s = s1 * s2"""
    (ax, ay, az, aw), ta, sa = A
    (bx, by, bz, bw), tb, sb = B
    q = (aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz)
    rx, ry, rz = rotate(A[0], tb[0], tb[1], tb[2])
    return (q, (sa * rx + ta[0], sa * ry + ta[1], sa * rz + ta[2]), sa * sb)


def sim3_exp(u, jit=NO_JITTER):
    """Sim3(const Vector7d& update): omega | upsilon | sigma"""
    ox, oy, oz = u[0], u[1], u[2]
    sigma = u[6]
    theta = math.sqrt(ox * ox + oy * oy + oz * oz)
    O = [[0.0, -oz, oy], [oz, 0.0, -ox], [-oy, ox, 0.0]]
    O2 = [[O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j] for j in range(3)] for i in range(3)]
    s = jit(math.exp, sigma)
    eps = 0.00001
    small = theta < eps
    if not small:
        sn = jit(math.sin, theta); cs = jit(math.cos, theta)
    if abs(sigma) < eps:
        C = 1.0
        if small:
            A = 1.0 / 2.0; B = 1.0 / 6.0
        else:
            theta2 = theta * theta
            A = (1.0 - cs) / theta2; B = (theta - sn) / (theta2 * theta)
    else:
        C = (s - 1.0) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma)
        else:
            a = s * sn; b = s * cs; theta2 = theta * theta; sigma2 = sigma * sigma; c = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2
    I = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    if small:
        R = [[(I[i][j] + O[i][j]) + O2[i][j] for j in range(3)] for i in range(3)]
    else:
        a = sn / theta; c = (1.0 - cs) / (theta * theta)
        R = [[(I[i][j] + a * O[i][j]) + c * O2[i][j] for j in range(3)] for i in range(3)]
    W = [[(A * O[i][j] + B * O2[i][j]) + C * I[i][j] for j in range(3)] for i in range(3)]
    t = tuple(W[i][0] * u[3] + W[i][1] * u[4] + W[i][2] * u[5] for i in range(3))
    return (quat_of_matrix(R), t, s)


def oplus(u, S, fix_scale, jit=NO_JITTER):
    """VertexSim3Expmap::oplusImpl: u[6] = 0 under fix_scale (in the caller's list), then Sim3(u) * estimate"""
    if fix_scale:
        u[6] = 0.0
    return mul(sim3_exp(u, jit), S)


def to_sim3(S12):
    v = [float(x) for x in np.asarray(S12, np.float64).reshape(8)]
    return (tuple(v[:4]), tuple(v[4:7]), v[7])


def to_array(S):
    return np.array(list(S[0]) + list(S[1]) + [S[2]], np.float64)


# ------------------------------------------------------------------------------------------------ the edges
class Problem:
    """cams = (fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2) float32; pairs[n, 12] float32 = u1, v1, inv_sigma2_1, u2, v2, inv_sigma2_2, X1c, X2c"""

    def __init__(self, cams, pairs, th2=10.0, fix_scale=False):
        self.cam = [float(v) for v in np.asarray(cams, np.float32).reshape(8)]
        self.p = np.asarray(pairs, np.float32).reshape(-1, 12).astype(np.float64)
        self.n = len(self.p)
        self.th2 = float(np.float32(th2))
        self.delta = float(np.float32(np.sqrt(np.float64(np.float32(th2)))))      # const float deltaHuber = sqrt(th2)
        self.fix_scale = bool(fix_scale)


def edge_errors(P, S, Sinv):
    """computeError of both edges of every pair: (e12[n, 2], e21[n, 2])"""
    p = P.p
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = P.cam
    with np.errstate(all="ignore"):
        x, y, z = smap(S, p[:, 9], p[:, 10], p[:, 11])
        e12 = np.stack([p[:, 0] - (x / z * fx1 + cx1), p[:, 1] - (y / z * fy1 + cy1)], 1)
        x, y, z = smap(Sinv, p[:, 6], p[:, 7], p[:, 8])
        e21 = np.stack([p[:, 3] - (x / z * fx2 + cx2), p[:, 4] - (y / z * fy2 + cy2)], 1)
    return e12, e21


def chi2s(P, S):
    """chi2() of both edges of every pair at S: (chi12[n], chi21[n])"""
    e12, e21 = edge_errors(P, S, inverse(S))
    w1, w2 = P.p[:, 2], P.p[:, 5]
    with np.errstate(all="ignore"):
        return e12[:, 0] * (w1 * e12[:, 0]) + e12[:, 1] * (w1 * e12[:, 1]), e21[:, 0] * (w2 * e21[:, 0]) + e21[:, 1] * (w2 * e21[:, 1])


def numeric_jacobians(P, S, jit=NO_JITTER):
    """BaseBinaryEdge::linearizeOplus for the Sim3 vertex: (J12[n, 2, 7], J21[n, 2, 7])"""
    J12 = np.zeros((P.n, 2, 7)); J21 = np.zeros((P.n, 2, 7))
    for d in range(7):
        add = [0.0] * 7
        add[d] = DELTA
        Sp = oplus(add, S, P.fix_scale, jit)
        p12, p21 = edge_errors(P, Sp, inverse(Sp))
        add[d] = -DELTA
        Sm = oplus(add, S, P.fix_scale, jit)
        m12, m21 = edge_errors(P, Sm, inverse(Sm))
        with np.errstate(all="ignore"):
            J12[:, :, d] = SCALAR * (p12 - m12); J21[:, :, d] = SCALAR * (p21 - m21)
    return J12, J21


def _sum_rows(terms, active, perm, tree):
    """the sum of the active pairs' edge rows (2n rows: pair i's forward edge 2i, inverse edge 2i + 1).  tree=None: one row after the other in the order
    perm (default: index order).  tree=T: the order of k_sim3_opt<T> - thread t adds the rows of its pairs t, t + T, ... (forward, then inverse) to 0.0,
    a wave adds its 64 threads by the xor butterfly 32, 16, ..., 1 (lane 0's value), the waves are added in the fixed pairwise tree."""
    n2, k = terms.shape
    active = np.asarray(active, bool)
    if tree is None:
        order = np.arange(n2) if perm is None else np.asarray(perm)
        order = order[active[order // 2]]
        return np.cumsum(terms[order], axis=0)[-1] if len(order) else np.zeros(k)      # cumsum adds one row after the other
    T = int(tree)
    n = n2 // 2
    acc = np.zeros((T, k))
    for start in range(0, n, T):
        idx = np.arange(start, min(start + T, n))
        live = active[idx]
        for side in (0, 1):
            acc[:len(idx)] = np.where(live[:, None], acc[:len(idx)] + terms[2 * idx + side], acc[:len(idx)])
    lanes = np.arange(64)
    part = []
    for w in range(T // 64):
        v = acc[64 * w:64 * w + 64]
        for m in (32, 16, 8, 4, 2, 1):
            v = v + v[lanes ^ m]
        part.append(v[0])
    s = 1
    while s < len(part):
        for a in range(0, len(part) - s, 2 * s):
            part[a] = part[a] + part[a + s]
        s *= 2
    return part[0]


def evaluate(P, S, active, perm=None, jit=NO_JITTER, tree=None):
    """computeActiveErrors + activeRobustChi2 + buildSystem at S over the edges of the active pairs: (H[28], b[7], chi)"""
    e12, e21 = edge_errors(P, S, inverse(S))
    J12, J21 = numeric_jacobians(P, S, jit)
    n = P.n
    e = np.empty((2 * n, 2)); J = np.empty((2 * n, 2, 7)); w = np.empty(2 * n)
    e[0::2] = e12; e[1::2] = e21; J[0::2] = J12; J[1::2] = J21; w[0::2] = P.p[:, 2]; w[1::2] = P.p[:, 5]
    with np.errstate(all="ignore"):
        chi2 = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
        dsqr = P.delta * P.delta
        out = ~(chi2 <= dsqr)
        sq = np.sqrt(chi2)
        rho0 = np.where(out, 2.0 * sq * P.delta - dsqr, chi2); rho1 = np.where(out, P.delta / sq, 1.0)
        wr = rho1 * w
        terms = np.zeros((2 * n, 36))
        for c, (j, k) in enumerate(_IDX):
            terms[:, c] = (J[:, 0, j] * wr) * J[:, 0, k] + (J[:, 1, j] * wr) * J[:, 1, k]
        for j in range(7):
            terms[:, 28 + j] = rho1 * (J[:, 0, j] * (w * e[:, 0]) + J[:, 1, j] * (w * e[:, 1]))
        terms[:, 35] = rho0
        tot = _sum_rows(terms, active, perm, tree)
    return tot[:28].copy(), -tot[28:35], float(tot[35])


def solve(H, b, lam, x):
    """(H + lam I) x = b by LDL^T without pivoting; a negative pivot: (False, x unchanged)"""
    Hf = np.zeros((7, 7))
    for c, (j, k) in enumerate(_IDX):
        Hf[j, k] = Hf[k, j] = H[c]
    L = np.zeros((7, 7)); d = np.zeros(7); yv = np.zeros(7)
    with np.errstate(all="ignore"):
        for j in range(7):
            s = Hf[j, j] + lam
            for k in range(j):
                s -= L[j, k] * L[j, k] * d[k]
            d[j] = s
            if s < 0.0:
                return False, x
            for i in range(j + 1, 7):
                v = Hf[j, i]
                for k in range(j):
                    v -= L[i, k] * L[j, k] * d[k]
                L[i, j] = v / s
        for i in range(7):
            v = b[i]
            for k in range(i):
                v -= L[i, k] * yv[k]
            yv[i] = v
        xn = [0.0] * 7
        for i in range(6, -1, -1):
            v = yv[i] / d[i]
            for k in range(i + 1, 7):
                v -= L[k, i] * xn[k]
            xn[i] = float(v)
    return True, xn


def optimize(P, cur, active, iterations, perm, jit, trace, tree=None):
    """initializeOptimization(); optimize(iterations) from the estimate cur: (estimate, estimate of the last computeActiveErrors)"""
    last = cur
    x = [0.0] * 7
    lam = ni = 0.0; n_bad = 0
    H, b, chi = evaluate(P, cur, active, perm, jit, tree)
    for it in range(iterations):
        if it:
            H, b, chi = evaluate(P, cur, active, perm, jit, tree)                          # g2o rebuilds errors and system at the estimate every iteration
        last = cur; ini_chi = chi
        if it == 0:
            lam = 1e-5 * max(0.0, *(abs(H[c]) for c in _DIAG)); ni = 2.0; n_bad = 0
        rho = 0.0; qmax = 0
        for q in range(10):
            ok2, x = solve(H, b, lam, x)
            x = list(x)
            trial = oplus(x, cur, P.fix_scale, jit); last = trial
            temp_chi = evaluate_chi(P, trial, active, perm, tree)
            if not ok2:
                temp_chi = DBL_MAX
            with np.errstate(all="ignore"):
                rho = np.float64(chi) - np.float64(temp_chi)
                scale = np.float64(0.0)
                for j in range(7):
                    scale += np.float64(x[j]) * (np.float64(lam) * x[j] + b[j])
                scale += 1e-3
                rho = rho / scale
            if rho > 0 and math.isfinite(temp_chi):
                alpha = 1.0 - (2 * rho - 1) ** 3.0
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha); ni = 2.0
                chi = temp_chi; cur = trial
                trace["accepted"] += 1
            else:
                lam *= ni; ni *= 2.0
                trace["rejected"] += 1
            qmax = q + 1
            if not (rho < 0 and qmax < 10):
                break
        trace["iterations"][-1] += 1
        if qmax == 10 or rho == 0:
            trace["terminate_trials"] += 1
            break
        n_bad = n_bad + 1 if (ini_chi - chi) * 1e3 < ini_chi else 0
        if n_bad >= 3:
            trace["three_strikes"] += 1
            break
    return cur, last


def evaluate_chi(P, S, active, perm=None, tree=None):
    """activeRobustChi2 at S alone: the last of evaluate()'s sums, added in the same order"""
    c12, c21 = chi2s(P, S)
    chi2 = np.empty(2 * P.n); chi2[0::2] = c12; chi2[1::2] = c21
    with np.errstate(all="ignore"):
        dsqr = P.delta * P.delta
        rho0 = np.where(~(chi2 <= dsqr), 2.0 * np.sqrt(chi2) * P.delta - dsqr, chi2)
        return float(_sum_rows(rho0[:, None], active, perm, tree)[0])


def optimize_sim3(cams, S12, pairs, th2=10.0, fix_scale=False, perm=None, jitter=None, want_trace=False, tree=None):
    """Returns (S12_out float64[8], removed uint8[n], n_inliers) [, trace].  Where the member returns 0 early S12_out is S12 bit for bit."""
    P = Problem(cams, pairs, th2, fix_scale)
    S_in = np.asarray(S12, np.float64).reshape(8).copy()
    jit = Jitter(jitter)
    trace = {"accepted": 0, "rejected": 0, "terminate_trials": 0, "three_strikes": 0, "phase_ends_rejected": 0, "iterations": [], "n_bad": 0, "early": False,
             "chi2": [], "estimate": None, "second_iterations": None}
    removed = np.zeros(P.n, np.uint8)
    if P.n == 0:
        r = (S_in, removed, 0)
        return r + (trace,) if want_trace else r
    cur = to_sim3(S_in)
    trace["iterations"].append(0)
    cur, last = optimize(P, cur, removed == 0, 5, perm, jit, trace, tree)
    trace["phase_ends_rejected"] += last is not cur
    c12, c21 = chi2s(P, last)
    trace["chi2"].append((c12, c21, removed == 0))
    with np.errstate(all="ignore"):
        bad = (c12 > P.th2) | (c21 > P.th2)
    removed[bad] = 1
    n_bad = int(bad.sum())
    trace["n_bad"] = n_bad; trace["estimate"] = cur
    if P.n - n_bad < 10:
        trace["early"] = True
        r = (S_in, removed, 0)
        return r + (trace,) if want_trace else r
    more = 10 if n_bad > 0 else 5
    trace["second_iterations"] = more
    trace["iterations"].append(0)
    live = removed == 0
    cur, last = optimize(P, cur, live, more, perm, jit, trace, tree)
    trace["phase_ends_rejected"] += last is not cur
    c12, c21 = chi2s(P, last)
    trace["chi2"].append((c12, c21, live))
    with np.errstate(all="ignore"):
        bad = live & ((c12 > P.th2) | (c21 > P.th2))
    removed[bad] = 1
    trace["estimate"] = cur
    r = (to_array(cur), removed, int((live & ~bad).sum()))
    return r + (trace,) if want_trace else r


# ------------------------------------------------------------------------------------------------ for the tests
def analytic_jacobians(P, S):
    """the closed-form derivative of the two errors with respect to the update of oplus at 0 (rotation | translation | log scale): with y = S.map(X2),
    d y / d u = [-[y]x | I | y]; with y2 = S^-1.map(X1), S^-1 = (R^T / s, ...), d y2 / d u = -(R^T / s) [-[X1]x | I | X1]; e = obs - K pi(y).
    (fix_scale: column 6 is 0.)  R^T / s stands for the linear part of inverse(), taken as the images of the unit vectors: right for any quaternion."""
    q, t, s = S
    p = P.p
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = P.cam
    R = np.stack(rotate(q, *np.eye(3)), 0)                                             # the linear map v -> q * v, columns = images of the unit vectors

    def skew(v):
        z = np.zeros(len(v))
        return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1), np.stack([-v[:, 1], v[:, 0], z], 1)], 1)

    def dproj(y, fx, fy):
        z = np.zeros(len(y))
        return np.stack([np.stack([fx / y[:, 2], z, -fx * y[:, 0] / y[:, 2] ** 2], 1), np.stack([z, fy / y[:, 2], -fy * y[:, 1] / y[:, 2] ** 2], 1)], 1)

    y = np.stack(smap(S, p[:, 9], p[:, 10], p[:, 11]), 1)
    G = np.concatenate([-skew(y), np.broadcast_to(np.eye(3), (P.n, 3, 3)), y[:, :, None]], 2)
    J12 = -np.einsum("nij,njk->nik", dproj(y, fx1, fy1), G)
    Si = inverse(S)
    Ri = np.stack(rotate(Si[0], *np.eye(3)), 0) * Si[2]
    X1 = p[:, 6:9]
    y2 = np.stack(smap(Si, X1[:, 0], X1[:, 1], X1[:, 2]), 1)
    G2 = -np.einsum("ij,njk->nik", Ri, np.concatenate([-skew(X1), np.broadcast_to(np.eye(3), (P.n, 3, 3)), X1[:, :, None]], 2))
    J21 = -np.einsum("nij,njk->nik", dproj(y2, fx2, fy2), G2)
    if P.fix_scale:
        J12[:, :, 6] = 0.0; J21[:, :, 6] = 0.0
    return J12, J21
