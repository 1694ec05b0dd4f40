"""A numpy restatement of DESIGN.md H18: PnPsolver (src/PnPsolver.cc of the reference) as orb_slam2_amd/csrc/orbhip_pnp.hip computes it, written from
reading the reference.  NOT pinned against OpenCV: cvSVD, cvSolve(CV_SVD), cvInvert(CV_SVD) and cvMulTransposed do not exist where this project is
developed, and each has a stated replacement here (H18 lists them).

Rounding: doubles throughout EPnP, np.float32 where CheckInliers holds a float.  Every operation is written out one rounding at a time, in the kernel's
order; EPnP needs +, -, *, / and sqrt only, all correctly rounded on both sides, so the kernel gives these bits under emulation and on the device.

A sum over the correspondences of a set is the kernel's: 64 partial sums - partial l adds positions l, l + 64, .. in rising order from 0.0 - and the
tree p[l] + p[l + 32], then + 16 .. + 1.  A position is the rank in the drawn quadruple (a hypothesis) or the correspondence's index (a refine over a
mask); positions outside the set add nothing.  Per-point expressions are evaluated on arrays (one IEEE operation per element, as in the kernel)."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
JACOBI_SWEEPS = 24
HEST_SWEEPS = 30
HEST_EPS = 1e-15
RANK_TOL = 1e-12
MAX_HYP = 4096


# ------------------------------------------------------------------------------------------------ the eigen-solver (orbhip_jacobi.h), many matrices at once
def jacobi_batch(A):
    """the cyclic Jacobi of orbhip_jacobi.h on H symmetric n x n matrices in lockstep: (w (H, n), V (H, n, n)), column i of V[h] the eigenvector of
    w[h, i]; nothing is sorted.  Each matrix gets exactly the operations of the one-matrix statement (tests/sim3_model.py: jacobi)."""
    A = np.array(A, f64, copy=True)
    H, n, _ = A.shape
    V = np.broadcast_to(np.eye(n), (H, n, n)).copy()
    active = np.ones(H, bool)
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            off = np.zeros(H)
            for p in range(n):
                for q in range(p + 1, n):
                    off = off + np.abs(A[:, p, q])
            active &= ~(off == 0.0)
            if not active.any():
                break
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = A[:, p, q].copy()
                    nz = active & ~(apq == 0.0)
                    if not nz.any():
                        continue
                    dpp, dqq = A[:, p, p].copy(), A[:, q, q].copy()
                    g, app, aqq = 100.0 * np.abs(apq), np.abs(dpp), np.abs(dqq)
                    neg = nz & (app + g == app) & (aqq + g == aqq)
                    A[neg, p, q] = 0.0; A[neg, q, p] = 0.0
                    rot = nz & ~neg
                    if not rot.any():
                        continue
                    theta = (dqq - dpp) / (2.0 * apq)
                    t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    t = np.where(theta < 0.0, -t, t)
                    t = np.where(np.abs(theta) > 1e150, 1.0 / (2.0 * theta), t)
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    c, s, R = c[:, None], s[:, None], rot[:, None]
                    xp, xq = A[:, :, p].copy(), A[:, :, q].copy()
                    A[:, :, p] = np.where(R, c * xp - s * xq, xp); A[:, :, q] = np.where(R, s * xp + c * xq, xq)
                    xp, xq = A[:, p, :].copy(), A[:, q, :].copy()
                    A[:, p, :] = np.where(R, c * xp - s * xq, xp); A[:, q, :] = np.where(R, s * xp + c * xq, xq)
                    xp, xq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p] = np.where(R, c * xp - s * xq, xp); V[:, :, q] = np.where(R, s * xp + c * xq, xq)
                    A[rot, p, q] = 0.0; A[rot, q, p] = 0.0
    return A[:, np.arange(n), np.arange(n)].copy(), V


def note(trace, arm):
    """count one passage through the named arm in `trace` (a dict, or None: nothing is recorded).  A trace changes no arithmetic: tests/pnp_checks.py asks
    it which arms a case reached, so that no test passes by emptiness"""
    if trace is not None:
        trace[arm] = trace.get(arm, 0) + 1


def sort_desc(w):
    """indices of w in descending order by insertion with a strict `>`: equal values keep their index order"""
    o = list(range(len(w)))
    for i in range(1, len(w)):
        j = i
        while j > 0 and w[o[j]] > w[o[j - 1]]:
            o[j], o[j - 1] = o[j - 1], o[j]
            j -= 1
    return o


# ------------------------------------------------------------------------------------------------ sums over a set
class Set:
    """the correspondences of one EPnP: P (r x 3) and uv (r x 2) in double by position, valid (r,) which positions take part"""

    def __init__(self, corr, quad=None, mask=None):
        corr = np.asarray(corr, f32).reshape(-1, 6)
        rows = corr if quad is None else corr[np.asarray(quad, np.int64)]
        self.P, self.uv = rows[:, 0:3].astype(f64), rows[:, 3:5].astype(f64)
        self.valid = np.ones(len(rows), bool) if mask is None else np.asarray(mask, bool).copy()
        self.m = int(self.valid.sum())
        self.first = int(np.flatnonzero(self.valid)[0]) if self.m else 0


def reduce(valid, vals):
    vals = np.asarray(vals, f64)
    if vals.ndim == 1:
        vals = vals[:, None]
    part = np.zeros((64, vals.shape[1]))
    for r0 in range(0, len(vals), 64):
        chunk, v = vals[r0:r0 + 64], valid[r0:r0 + 64]
        part[:len(chunk)] = np.where(v[:, None], part[:len(chunk)] + chunk, part[:len(chunk)])
    for d in (32, 16, 8, 4, 2, 1):
        part[:d] = part[:d] + part[d:2 * d]
    return part[0].copy()


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def alphas(P, ci, c0):
    """compute_barycentric_coordinates on the points P (r x 3): r x 4"""
    d0, d1, d2 = P[:, 0] - c0[0], P[:, 1] - c0[1], P[:, 2] - c0[2]
    a = np.zeros((len(P), 4))
    for j in range(3):
        a[:, 1 + j] = (ci[3 * j] * d0 + ci[3 * j + 1] * d1) + ci[3 * j + 2] * d2
    a[:, 0] = ((1.0 - a[:, 1]) - a[:, 2]) - a[:, 3]
    return a


# ------------------------------------------------------------------------------------------------ the small solvers
def qr_solve(A, b, x):
    """PnPsolver::qr_solve on a 6 x nc system (A, b are overwritten; x is updated in place and left as it is at a zero column).  eta is the largest
    |A[i][k]| over rows k .. 4: the reference's loop tests an entry before it steps to the next row."""
    nr, nc = A.shape
    A1, A2 = np.zeros(nc), np.zeros(nc)
    for k in range(nc):
        eta = abs(A[k, k])
        for i in range(k + 1, nr):
            elt = abs(A[i - 1, k])
            if eta < elt:
                eta = elt
        if eta == 0.0:
            return x
        inv_eta = f64(1.0) / eta
        s = f64(0.0)
        for i in range(k, nr):
            A[i, k] = A[i, k] * inv_eta
            s = s + A[i, k] * A[i, k]
        sigma = np.sqrt(s)
        if A[k, k] < 0.0:
            sigma = -sigma
        A[k, k] = A[k, k] + sigma
        A1[k] = sigma * A[k, k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s2 = f64(0.0)
            for i in range(k, nr):
                s2 = s2 + A[i, k] * A[i, j]
            tau = s2 / A1[k]
            for i in range(k, nr):
                A[i, j] = A[i, j] - tau * A[i, k]
    for j in range(nc):
        tau = f64(0.0)
        for i in range(j, nr):
            tau = tau + A[i, j] * b[i]
        tau = tau / A1[j]
        for i in range(j, nr):
            b[i] = b[i] - tau * A[i, j]
    x[nc - 1] = b[nc - 1] / A2[nc - 1]
    for i in range(nc - 2, -1, -1):
        s = f64(0.0)
        for j in range(i + 1, nc):
            s = s + A[i, j] * x[j]
        x[i] = (b[i] - s) / A2[i]
    return x


def betas_approx(which, L, rho):
    cols = {1: (0, 1, 3, 6), 2: (0, 1, 2), 3: (0, 1, 2, 3, 4)}[which]
    x = qr_solve(L[:, cols].copy(), rho.copy(), np.zeros(len(cols)))
    b = np.zeros(4)
    if which == 1:
        if x[0] < 0.0:
            b[0] = np.sqrt(-x[0]); b[1] = -x[1] / b[0]; b[2] = -x[2] / b[0]; b[3] = -x[3] / b[0]
        else:
            b[0] = np.sqrt(x[0]); b[1] = x[1] / b[0]; b[2] = x[2] / b[0]; b[3] = x[3] / b[0]
        return b
    if x[0] < 0.0:
        b[0] = np.sqrt(-x[0]); b[1] = np.sqrt(-x[2]) if x[2] < 0.0 else 0.0
    else:
        b[0] = np.sqrt(x[0]); b[1] = np.sqrt(x[2]) if x[2] > 0.0 else 0.0
    if x[1] < 0.0:
        b[0] = -b[0]
    b[2] = x[3] / b[0] if which == 3 else 0.0
    return b


def gauss_newton(L, rho, betas):
    x = np.zeros(4)
    for _ in range(5):
        A, b = np.zeros((6, 4)), np.zeros(6)
        b0, b1, b2, b3 = betas
        for i in range(6):
            r = L[i]
            A[i, 0] = (((2.0 * r[0]) * b0 + r[1] * b1) + r[3] * b2) + r[6] * b3
            A[i, 1] = ((r[1] * b0 + (2.0 * r[2]) * b1) + r[4] * b2) + r[7] * b3
            A[i, 2] = ((r[3] * b0 + r[4] * b1) + (2.0 * r[5]) * b2) + r[8] * b3
            A[i, 3] = ((r[6] * b0 + r[7] * b1) + r[8] * b2) + (2.0 * r[9]) * b3
            b[i] = rho[i] - ((((((((((r[0] * b0) * b0 + (r[1] * b0) * b1) + (r[2] * b1) * b1) + (r[3] * b0) * b2) + (r[4] * b1) * b2) + (r[5] * b2) * b2) +
                                 (r[6] * b0) * b3) + (r[7] * b1) * b3) + (r[8] * b2) * b3) + (r[9] * b3) * b3)
        qr_solve(A, b, x)
        betas = betas + x
    return betas


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def hestenes(abt, trace=None):
    """U, sigma, V of the 3 x 3 ABt = U diag(sigma) V^T by one-sided Jacobi: columns of G = ABt W made orthogonal pair by pair; sorted descending;
    at rank 2 (sigma_3 <= RANK_TOL sigma_1) the third columns are the cross products of the first two"""
    G = [np.array(abt[:, c], f64) for c in range(3)]
    W = [np.array([1.0 if r == c else 0.0 for r in range(3)]) for c in range(3)]
    for _ in range(HEST_SWEEPS):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            alpha, beta, gamma = dot3(G[p], G[p]), dot3(G[q], G[q]), dot3(G[p], G[q])
            if gamma == 0.0:
                continue
            if abs(gamma) <= HEST_EPS * np.sqrt(alpha * beta):
                continue
            rotated = True
            zeta = (beta - alpha) / (2.0 * gamma)
            if abs(zeta) > 1e150:
                t = 1.0 / (2.0 * zeta)
            else:
                t = 1.0 / (abs(zeta) + np.sqrt(zeta * zeta + 1.0))
                if zeta < 0.0:
                    t = -t
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            G[p], G[q] = c * G[p] - s * G[q], s * G[p] + c * G[q]
            W[p], W[q] = c * W[p] - s * W[q], s * W[p] + c * W[q]
        if not rotated:
            break
    sg = [np.sqrt(dot3(G[c], G[c])) for c in range(3)]
    o = sort_desc(sg)
    U = [G[o[c]] / sg[o[c]] for c in range(3)]
    V = [W[o[c]] for c in range(3)]
    if not sg[o[2]] > RANK_TOL * sg[o[0]]:
        note(trace, "rank2_finite" if np.isfinite(sg).all() and sg[o[1]] > 0.0 else "rank2_degenerate")
        U[2], V[2] = cross(U[0], U[1]), cross(V[0], V[1])
    else:
        note(trace, "full_rank")
    return np.array(U).T, np.array([sg[k] for k in o]), np.array(V).T


def rotation(abt, trace=None):
    """estimate_R_and_t's R = U V^T with the det < 0 row flip; 3 x 3"""
    U, _, V = hestenes(abt, trace)
    R = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            R[i, j] = (U[i, 0] * V[j, 0] + U[i, 1] * V[j, 1]) + U[i, 2] * V[j, 2]
    det = ((((((R[0, 0] * R[1, 1]) * R[2, 2] + (R[0, 1] * R[1, 2]) * R[2, 0]) + (R[0, 2] * R[1, 0]) * R[2, 1]) - (R[0, 2] * R[1, 1]) * R[2, 0]) -
            (R[0, 1] * R[1, 0]) * R[2, 2]) - (R[0, 0] * R[1, 2]) * R[2, 1])
    if det < 0.0:
        note(trace, "det_negative")
        R[2] = -R[2]
    return R


# ------------------------------------------------------------------------------------------------ compute_pose
PA, PB = (0, 0, 0, 1, 1, 2), (1, 2, 3, 2, 3, 3)


def control_points(c0, w, V, dm, trace=None):
    """choose_control_points from the eigenvalues w and eigenvectors V (columns) of PW0^T PW0: the centroid, then c0 + sqrt(dc / n) * vector in descending
    order of dc; an eigenvalue below zero (rounding, on coplanar points) is clamped to 0 before the square root"""
    o = sort_desc(w)
    cws = np.zeros((4, 3))
    cws[0] = c0
    for i in range(1, 4):
        dc = w[o[i - 1]]
        if dc < 0.0:
            note(trace, "dc_clamp")
            dc = f64(0.0)
        k = np.sqrt(dc / dm)
        cws[i] = c0 + k * V[:, o[i - 1]]
    return cws


def epnp_front(S, K, trace=None):
    """choose_control_points, compute_barycentric_coordinates and M^T M: the state compute_pose carries to the 12 x 12 eigenproblem"""
    fu, fv, uc, vc = [f64(f32(k)) for k in K]
    dm = f64(S.m)
    c0 = reduce(S.valid, S.P) / dm
    d = S.P - c0
    s6 = reduce(S.valid, np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1))
    w, V = jacobi_batch(np.array([[[s6[0], s6[1], s6[2]], [s6[1], s6[3], s6[4]], [s6[2], s6[4], s6[5]]]]))
    cws = control_points(c0, w[0], V[0], dm, trace)
    cc = np.zeros(9)
    for i in range(3):
        for j in range(1, 4):
            cc[3 * i + j - 1] = cws[j, i] - cws[0, i]
    m00, m01, m02 = cc[4] * cc[8] - cc[5] * cc[7], cc[3] * cc[8] - cc[5] * cc[6], cc[3] * cc[7] - cc[4] * cc[6]
    det = (cc[0] * m00 - cc[1] * m01) + cc[2] * m02
    ci = np.array([m00 / det, (cc[2] * cc[7] - cc[1] * cc[8]) / det, (cc[1] * cc[5] - cc[2] * cc[4]) / det,
                   (cc[5] * cc[6] - cc[3] * cc[8]) / det, (cc[0] * cc[8] - cc[2] * cc[6]) / det, (cc[2] * cc[3] - cc[0] * cc[5]) / det,
                   m02 / det, (cc[1] * cc[6] - cc[0] * cc[7]) / det, (cc[0] * cc[4] - cc[1] * cc[3]) / det])
    a = alphas(S.P, ci, c0)
    du, dv = uc - S.uv[:, 0], vc - S.uv[:, 1]
    M1, M2 = np.zeros((len(a), 12)), np.zeros((len(a), 12))
    for i in range(4):
        M1[:, 3 * i] = a[:, i] * fu; M1[:, 3 * i + 2] = a[:, i] * du
        M2[:, 3 * i + 1] = a[:, i] * fv; M2[:, 3 * i + 2] = a[:, i] * dv
    MtM = np.zeros((12, 12))
    for r in range(12):
        MtM[r] = reduce(S.valid, M1[:, r:r + 1] * M1 + M2[:, r:r + 1] * M2)
    return dict(S=S, K=(fu, fv, uc, vc), dm=dm, c0=c0, cws=cws, ci=ci, a=a, MtM=MtM)


def epnp_back(st, w, V, trace=None):
    """compute_pose from the eigenvectors on: R (3 x 3), t (3,) in double"""
    S, (fu, fv, uc, vc), dm, c0, cws, a = st["S"], st["K"], st["dm"], st["c0"], st["cws"], st["a"]
    o = sort_desc(w)
    v = [V[:, o[11 - i]] for i in range(4)]                                     # ut row 11 - i
    L = np.zeros((6, 10))
    for i in range(6):
        dv = [v[k][3 * PA[i]:3 * PA[i] + 3] - v[k][3 * PB[i]:3 * PB[i] + 3] for k in range(4)]
        L[i] = [dot3(dv[0], dv[0]), 2.0 * dot3(dv[0], dv[1]), dot3(dv[1], dv[1]), 2.0 * dot3(dv[0], dv[2]), 2.0 * dot3(dv[1], dv[2]), dot3(dv[2], dv[2]),
                2.0 * dot3(dv[0], dv[3]), 2.0 * dot3(dv[1], dv[3]), 2.0 * dot3(dv[2], dv[3]), dot3(dv[3], dv[3])]
    rho = np.zeros(6)
    for i in range(6):
        dd = cws[PA[i]] - cws[PB[i]]
        rho[i] = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]
    best = None
    for which in (1, 2, 3):
        betas = gauss_newton(L, rho, betas_approx(which, L, rho))
        ccs = np.zeros((4, 3))
        for j in range(4):
            for k in range(3):
                s = f64(0.0)
                for i in range(4):
                    s = s + betas[i] * v[i][3 * j + k]
                ccs[j, k] = s
        if S.m > 0:
            af = a[S.first]
            if trace is not None:                                               # would another member of the set have decided otherwise?
                neg = (((a[:, 0] * ccs[0, 2] + a[:, 1] * ccs[1, 2]) + a[:, 2] * ccs[2, 2]) + a[:, 3] * ccs[3, 2] < 0.0)[S.valid]
                note(trace, "sign_depends_on_first" if neg.any() and not neg.all() else "sign_unanimous")
            if ((af[0] * ccs[0, 2] + af[1] * ccs[1, 2]) + af[2] * ccs[2, 2]) + af[3] * ccs[3, 2] < 0.0:
                note(trace, "sign_flip")
                ccs = -ccs
        pcs = np.stack([((a[:, 0] * ccs[0, j] + a[:, 1] * ccs[1, j]) + a[:, 2] * ccs[2, j]) + a[:, 3] * ccs[3, j] for j in range(3)], 1)
        pc0 = reduce(S.valid, pcs) / dm
        wd = S.P - c0
        abt = reduce(S.valid, np.stack([(pcs[:, j] - pc0[j]) * wd[:, c] for j in range(3) for c in range(3)], 1)).reshape(3, 3)
        R = rotation(abt, trace)
        t = np.array([pc0[i] - dot3(R[i], c0) for i in range(3)])
        P = S.P
        Xc = ((R[0, 0] * P[:, 0] + R[0, 1] * P[:, 1]) + R[0, 2] * P[:, 2]) + t[0]
        Yc = ((R[1, 0] * P[:, 0] + R[1, 1] * P[:, 1]) + R[1, 2] * P[:, 2]) + t[1]
        inv_Zc = 1.0 / (((R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1]) + R[2, 2] * P[:, 2]) + t[2])
        ue, ve = uc + (fu * Xc) * inv_Zc, vc + (fv * Yc) * inv_Zc
        du, dv = S.uv[:, 0] - ue, S.uv[:, 1] - ve
        err = reduce(S.valid, np.sqrt(du * du + dv * dv))[0] / dm
        if best is None or err < best[0]:
            best = (err, R, t)
    return best[1], best[2]


def epnp_many(sets, K, trace=None):
    """compute_pose for several sets (the 12 x 12 eigenproblems run in lockstep): a list of (R, t)"""
    with np.errstate(all="ignore"):
        fronts = [epnp_front(S, K, trace) for S in sets]
        if not fronts:
            return []
        w, V = jacobi_batch(np.array([st["MtM"] for st in fronts]))
        return [epnp_back(st, w[h], V[h], trace) for h, st in enumerate(fronts)]


def epnp(corr, K, quad=None, mask=None, trace=None):
    return epnp_many([Set(corr, quad, mask)], K, trace)[0]


# ------------------------------------------------------------------------------------------------ CheckInliers
def reprojection_error2(R, t, K, corr):
    """error2 of CheckInliers for every correspondence (float32): the double mRi, mti times float points rounded to float, invZc rounded to float,
    ue and ve in double, distX and distY in float"""
    with np.errstate(all="ignore"):
        corr = np.asarray(corr, f32).reshape(-1, 6)
        fu, fv, uc, vc = [f64(f32(k)) for k in K]
        R, t = np.asarray(R, f64).reshape(3, 3), np.asarray(t, f64).reshape(3)
        x, y, z = corr[:, 0].astype(f64), corr[:, 1].astype(f64), corr[:, 2].astype(f64)
        Xc = ((((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + t[0])).astype(f32)
        Yc = ((((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + t[1])).astype(f32)
        invZc = (1.0 / (((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + t[2])).astype(f32)
        ue = uc + (fu * Xc.astype(f64)) * invZc.astype(f64)
        ve = vc + (fv * Yc.astype(f64)) * invZc.astype(f64)
        distX, distY = (corr[:, 3].astype(f64) - ue).astype(f32), (corr[:, 4].astype(f64) - ve).astype(f32)
        return distX * distX + distY * distY


def check_inliers(R, t, K, corr):
    corr = np.asarray(corr, f32).reshape(-1, 6)
    with np.errstate(all="ignore"):
        mask = reprojection_error2(R, t, K, corr) < corr[:, 5]                  # strict, in float; no test for positive depth
    return mask, int(mask.sum())


def pack_mask(mask):
    words = np.zeros((len(mask) + 63) // 64, np.uint64)
    for i in np.flatnonzero(mask):
        words[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return words


def tcw(R, t):
    T = np.eye(4, dtype=f32)
    with np.errstate(all="ignore"):
        T[:3, :3] = np.asarray(R, f64).reshape(3, 3).astype(f32); T[:3, 3] = np.asarray(t, f64).astype(f32)
    return T


# ------------------------------------------------------------------------------------------------ iterate
def iterate(K, corr, quads, min_inliers, best_in=0, best_mask_in=None, trace=None):
    """what orbhip_pnp_iterate returns, from the model: a dict with the ABI's names (hyp_* for every hypothesis, ref_* for every refine the loop made).
    `trace`, a dict, receives the arms taken: trace["hyp"] counts those of the hypotheses, trace["ref"] those of the refines (see note)"""
    corr = np.asarray(corr, f32).reshape(-1, 6)
    quads = np.asarray(quads, np.int32).reshape(-1, 4)
    n, nh, mi = len(corr), len(quads), int(min_inliers)
    out = dict(n_consumed=0, returned=-1, best=-1, best_inliers_out=None, best_Tcw=None, best_mask=None, refined_Tcw=None, refined_inliers=None, refined_mask=None)
    if n < 4 or n < mi or nh == 0:
        return out
    words = (n + 63) // 64
    hR, ht, hc, hm = np.zeros((nh, 3, 3)), np.zeros((nh, 3)), np.zeros(nh, np.int32), np.zeros((nh, words), np.uint64)
    masks = []
    t_hyp, t_ref = (None, None) if trace is None else (trace.setdefault("hyp", {}), trace.setdefault("ref", {}))
    for h, (R, t) in enumerate(epnp_many([Set(corr, q) for q in quads], K, t_hyp)):
        m, c = check_inliers(R, t, K, corr)
        hR[h], ht[h], hc[h], hm[h] = R, t, c, pack_mask(m)
        masks.append(m)
    run, cur, best, returned, consumed = int(best_in), -1, -1, -1, nh
    carried = np.zeros(n, bool) if best_mask_in is None or best_in <= 0 else np.asarray(best_mask_in, bool)
    refs = {}
    for h in range(nh):
        if hc[h] >= mi:
            if hc[h] > run:
                run, cur, best = int(hc[h]), h, h
            if cur not in refs:                                                 # Refine() is a pure function of the best mask
                src = carried if cur < 0 else masks[cur]
                note(t_ref, "words_%d" % words)
                note(t_ref, "first_ge_64" if src.any() and int(np.flatnonzero(src)[0]) >= 64 else "first_lt_64")
                R, t = epnp(corr, K, mask=src, trace=t_ref)
                refs[cur] = (R, t) + check_inliers(R, t, K, corr)
            if refs[cur][3] > mi:
                returned, consumed = h, h + 1
                break
    keys = list(refs)
    out.update(n_consumed=consumed, returned=returned, best=best, best_inliers_out=run, hyp_R=hR, hyp_t=ht, hyp_count=hc, hyp_mask=hm,
               ref_hyp=np.array(keys, np.int32), ref_R=np.array([refs[k][0] for k in keys]).reshape(-1, 3, 3), ref_t=np.array([refs[k][1] for k in keys]).reshape(-1, 3),
               ref_count=np.array([refs[k][3] for k in keys], np.int32), ref_mask=np.array([pack_mask(refs[k][2]) for k in keys], np.uint64).reshape(-1, words))
    if best >= 0:
        out.update(best_Tcw=tcw(hR[best], ht[best]), best_mask=masks[best])
    if returned >= 0:
        R, t, m, c = refs[cur]
        out.update(refined_Tcw=tcw(R, t), refined_inliers=c, refined_mask=m)
    return out


# ------------------------------------------------------------------------------------------------ the class
INT_MIN = -2 ** 31


def ransac_parameters(N, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991):
    """SetRansacParameters: (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon).  Where the reference's iteration count is not finite, does not fit an
    int, or N == 0, the conversion to int is undefined; x86 gives INT_MIN, so max(1, min(INT_MIN, maxIterations)) = 1 - stated here for every machine."""
    with np.errstate(all="ignore"):
        eps = f32(epsilon)
        n_min = int(f32(N) * eps)                                               # int nMinInliers = N*mRansacEpsilon: a float product, truncated
        n_min = max(n_min, int(min_inliers))
        n_min = max(n_min, int(min_set))
        if N > 0 and eps < f32(n_min) / f32(N):
            eps = f32(n_min) / f32(N)
        if n_min == N:
            n_its = 1
        elif N == 0:
            n_its = INT_MIN
        else:
            x = np.ceil(np.log(f64(1.0 - probability)) / np.log(f64(1.0) - f64(math.pow(float(eps), 3.0))))
            n_its = int(x) if np.isfinite(x) and INT_MIN <= x < 2 ** 31 else INT_MIN
    return n_min, max(1, min(n_its, int(max_iterations))), eps


def max_errors(sigma2, th2=5.991):
    return np.asarray(sigma2, f32) * f32(th2)


class Solver:
    """PnPsolver's RANSAC state with the drop-in's draw queue: `rand(lo, hi)` is DUtils::Random::RandomInt"""

    def __init__(self, K, corr, rand):
        self.K, self.corr, self.rand = np.asarray(K, f32), np.asarray(corr, f32).reshape(-1, 6), rand
        self.N = len(self.corr)
        self.iterations, self.best_inliers, self.best_mask, self.best_Tcw = 0, 0, None, None
        self.queue = []
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
        if min_set != 4:
            raise ValueError("minSet must be 4")
        self.min_inliers, self.max_its, self.epsilon = ransac_parameters(self.N, probability, min_inliers, max_iterations, min_set, epsilon)

    def draw(self):
        avail = list(range(self.N))
        quad = []
        for _ in range(4):
            r = self.rand(0, len(avail) - 1)
            quad.append(avail[r])
            avail[r] = avail[-1]
            avail.pop()
        return quad

    def loop_count(self, n_iterations):
        """while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations): an OR"""
        return max(int(n_iterations), self.max_its - self.iterations, 0)

    def take(self, n_iterations):
        """the quadruples of one iterate(n_iterations): queued ones first, the rest drawn; None where iterate returns before its loop"""
        if self.N < self.min_inliers:
            return None
        need = self.loop_count(n_iterations)
        quads = self.queue[:need]
        self.queue = self.queue[need:]
        while len(quads) < need:
            quads.append(self.draw())
        return quads

    def solve(self, quads):
        """the answer to the quadruples (a device-backed solver overrides this)"""
        return iterate(self.K, self.corr, quads, self.min_inliers, self.best_inliers, self.best_mask)

    def iterate(self, n_iterations):
        """(Tcw or None, bNoMore, inliers, nInliers)"""
        quads = self.take(n_iterations)
        none = np.zeros(self.N, bool)
        if quads is None:
            return None, True, none, 0
        pos = 0
        while pos < len(quads):                                                 # at most MAX_HYP a device call; the best count and mask carry over
            part = quads[pos:pos + MAX_HYP]
            res = self.solve(part)
            self.iterations += res["n_consumed"]
            if res["best"] >= 0:
                self.best_inliers, self.best_mask, self.best_Tcw = res["best_inliers_out"], res["best_mask"], res["best_Tcw"]
            if res["returned"] >= 0:
                self.queue = part[res["n_consumed"]:] + quads[pos + len(part):] + self.queue
                return res["refined_Tcw"], False, res["refined_mask"], res["refined_inliers"]
            pos += len(part)
        if self.iterations >= self.max_its:
            if self.best_inliers >= self.min_inliers:
                return self.best_Tcw, True, self.best_mask, self.best_inliers
            return None, True, none, 0
        return None, False, none, 0

    def find(self):
        return self.iterate(self.max_its)
