"""Scenes for the PnP RANSAC tests (tests/pnp_checks.py): one camera with a known Rcw, tcw, points 2 - 8 m in front of it seen at pyramid levels 0 - 7
with pixel noise that grows with the level, a share of the matches wrong.  Everything is a pure function of the parameters and a seed.

Graded sizes are where a wave, a mask word or a clamp of SetRansacParameters turns over: n = 4 and 5 (N == mRansacMinInliers: one iteration), 20, 63,
64, 65, 129, 300, 1000; 1, 5 and 300 hypotheses; one planar scene (all points on a wall; no hypothesis of it reaches the minimum, so nothing is refined
and ABt of estimate_R_and_t never has rank 2 there: the planar refines are planar_exact and planar_failing_refines of REFINE_CASES)."""
import numpy as np

import pnp_model as M

f32 = np.float32
K = np.array([517.306408, 516.469215, 318.643040, 255.313989], f32)
W, H = 640.0, 480.0
TH2 = 5.991


def level_sigma2(levels=8, scale=1.2):
    s = np.ones(levels, f32)
    for i in range(1, levels):
        s[i] = s[i - 1] * f32(scale)
    return s * s


def pose(rng):
    """a rotation of up to 0.6 rad about a random axis and a translation of up to 1 m: Rcw (3 x 3), tcw (3,) in double"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.1, 0.6)
    X = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(ang) * X + (1.0 - np.cos(ang)) * (X @ X), rng.uniform(-1.0, 1.0, 3)


def scene(n, seed, outliers=0.3, noise=0.5, planar=False):
    """(corr n x 6 float32: Xw, u, v, max_error; Rcw; tcw; which correspondences are true matches)"""
    rng = np.random.default_rng(seed)
    Rcw, tcw = pose(rng)
    fx, fy, cx, cy = [float(k) for k in K]
    u, v = rng.uniform(20.0, W - 20.0, n), rng.uniform(20.0, H - 20.0, n)
    x, y = (u - cx) / fx, (v - cy) / fy
    z = 5.0 / (1.0 - 0.3 * x - 0.2 * y) if planar else rng.uniform(2.0, 8.0, n)     # the wall: z = 5 + 0.3 X + 0.2 Y
    Pc = np.stack([x * z, y * z, z], 1)
    Xw = ((Pc - tcw) @ Rcw).astype(f32)                                         # Rcw^T (Pc - tcw)
    level = rng.integers(0, 8, n)
    s2 = level_sigma2()[level]
    uv = np.stack([u, v], 1) + noise * np.sqrt(s2.astype(np.float64))[:, None] * rng.normal(size=(n, 2))
    good = rng.uniform(size=n) >= outliers
    wrong = np.stack([rng.uniform(0.0, W, n), rng.uniform(0.0, H, n)], 1)
    uv = np.where(good[:, None], uv, wrong)
    corr = np.zeros((n, 6), f32)
    corr[:, 0:3], corr[:, 3:5], corr[:, 5] = Xw, uv.astype(f32), M.max_errors(s2, TH2)
    return corr, Rcw, tcw, good


def draw_quads(n, nh, seed):
    """nh quadruples as PnPsolver draws them: four RandomInt(0, size - 1) with swap-remove from a fresh index list"""
    rng = np.random.default_rng(seed + 7919)
    out = np.zeros((nh, 4), np.int32)
    for h in range(nh):
        avail = list(range(n))
        for k in range(4):
            r = int(rng.integers(0, len(avail)))
            out[h, k] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


#                name           n     seed noise planar: EPnP over all (true) matches, for the model's yardstick (tests/golden/make_golden_pnp_spread.py)
SPREAD_SCENES = [("all_n6", 6, 31, 0.0, False), ("all_n20", 20, 32, 0.0, False), ("all_n65", 65, 33, 0.0, False), ("all_n300", 300, 34, 0.0, False),
                 ("all_n20_noise", 20, 35, 0.5, False), ("all_n129_noise", 129, 36, 0.5, False), ("all_n1000_noise", 1000, 37, 0.5, False),
                 ("all_planar_n100", 100, 38, 0.0, True)]


def independent_epnp(corr, K):
    """EPnP over all correspondences in plain numpy (eigh, lstsq, inv, svd), written apart from tests/pnp_model.py: (R, t)"""
    corr = np.asarray(corr, np.float64).reshape(-1, 6)
    fu, fv, uc, vc = [float(k) for k in np.asarray(K, f32)]
    P, u, v, n = corr[:, 0:3], corr[:, 3], corr[:, 4], len(corr)
    c0 = P.mean(0)
    w, E = np.linalg.eigh((P - c0).T @ (P - c0))
    cws = np.vstack([c0] + [c0 + np.sqrt(max(w[i], 0.0) / n) * E[:, i] for i in (2, 1, 0)])
    a123 = (np.linalg.inv((cws[1:] - c0).T) @ (P - c0).T).T
    a = np.hstack([1.0 - a123.sum(1, keepdims=True), a123])
    Mm = np.zeros((2 * n, 12))
    for i in range(4):
        Mm[0::2, 3 * i], Mm[0::2, 3 * i + 2] = a[:, i] * fu, a[:, i] * (uc - u)
        Mm[1::2, 3 * i + 1], Mm[1::2, 3 * i + 2] = a[:, i] * fv, a[:, i] * (vc - v)
    _, E12 = np.linalg.eigh(Mm.T @ Mm)
    vs = [E12[:, i].reshape(4, 3) for i in range(4)]                            # smallest eigenvalue first
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = [[vs[k][pa] - vs[k][pb] for pa, pb in pairs] for k in range(4)]
    idx = [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3)]
    L = np.array([[(1.0 if p == q else 2.0) * (dv[p][i] @ dv[q][i]) for p, q in idx] for i in range(6)])
    rho = np.array([((cws[pa] - cws[pb]) ** 2).sum() for pa, pb in pairs])

    def pose(betas):
        for _ in range(5):
            bb = np.array([betas[p] * betas[q] for p, q in idx])
            J = np.zeros((6, 4))
            for k, (p, q) in enumerate(idx):
                J[:, p] += L[:, k] * betas[q]
                J[:, q] += L[:, k] * betas[p]
            betas = betas + np.linalg.lstsq(J, rho - L @ bb, rcond=None)[0]
        ccs = sum(betas[k] * vs[k] for k in range(4))
        pcs = a @ ccs
        if pcs[0, 2] < 0:
            pcs = -pcs
        pc0, pw0 = pcs.mean(0), P.mean(0)
        U, _, Vt = np.linalg.svd((pcs - pc0).T @ (P - pw0))
        R = U @ Vt
        if np.linalg.det(R) < 0:
            R[2] = -R[2]
        t = pc0 - R @ pw0
        Pc = P @ R.T + t
        err = np.sqrt((u - (uc + fu * Pc[:, 0] / Pc[:, 2])) ** 2 + (v - (vc + fv * Pc[:, 1] / Pc[:, 2])) ** 2).mean()
        return err, R, t

    cands = []
    x = np.linalg.lstsq(L[:, [0, 1, 3, 6]], rho, rcond=None)[0]
    s = -1.0 if x[0] < 0 else 1.0
    b0 = np.sqrt(s * x[0])
    cands.append(np.array([b0, s * x[1] / b0, s * x[2] / b0, s * x[3] / b0]))
    for cols in ([0, 1, 2], [0, 1, 2, 3, 4]):
        x = np.linalg.lstsq(L[:, cols], rho, rcond=None)[0]
        if x[0] < 0:
            b = [np.sqrt(-x[0]), np.sqrt(-x[2]) if x[2] < 0 else 0.0]
        else:
            b = [np.sqrt(x[0]), np.sqrt(x[2]) if x[2] > 0 else 0.0]
        if x[1] < 0:
            b[0] = -b[0]
        cands.append(np.array([b[0], b[1], x[3] / b[0] if len(cols) == 5 else 0.0, 0.0]))
    best = None
    for b in cands:
        r = pose(b)
        if best is None or r[0] < best[0]:
            best = r
    return best[1], best[2]


_two = {}


def two_poses(mi=12, extra=6, junk=10, seed=5):
    """A scene that holds two poses, for the selection rules: correspondences 0 .. mi-1 are exact under pose B (exactly the minimum), the next mi + extra
    exact under pose A, the rest junk; all at level 0.  Returns a dict: corr, mi, quads_b (two quadruples of B's points whose hypotheses count exactly
    mi inliers - B's points - by the model), quad_a (one of A's points that counts exactly A's), quad_junk (one that stays below the minimum)."""
    key = (mi, extra, junk, seed)
    if key in _two:
        return _two[key]
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = [float(k) for k in K]
    nb, na = mi, mi + extra
    n = nb + na + junk
    corr = np.zeros((n, 6), f32)
    corr[:, 5] = M.max_errors(np.ones(n, f32), TH2)
    for lo, hi in ((0, nb), (nb, nb + na)):
        Rcw, tcw = pose(rng)
        u, v, z = rng.uniform(20.0, W - 20.0, hi - lo), rng.uniform(20.0, H - 20.0, hi - lo), rng.uniform(2.0, 8.0, hi - lo)
        Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
        corr[lo:hi, 0:3] = ((Pc - tcw) @ Rcw).astype(f32)
        corr[lo:hi, 3], corr[lo:hi, 4] = u.astype(f32), v.astype(f32)
    corr[nb + na:, 0:3] = rng.uniform(-3.0, 3.0, (junk, 3)).astype(f32)
    corr[nb + na:, 3], corr[nb + na:, 4] = rng.uniform(0.0, W, junk).astype(f32), rng.uniform(0.0, H, junk).astype(f32)

    def gated(lo, hi, want, count):
        """quadruples drawn among lo .. hi-1 whose hypothesis has exactly the inliers `want`"""
        out = []
        for _ in range(200):
            q = [int(x) for x in lo + rng.permutation(hi - lo)[:4]]
            mask, _ = M.check_inliers(*M.epnp(corr, K, quad=q), K, corr)
            if np.array_equal(mask, want):
                out.append(q)
                if len(out) == count:
                    return out
        raise AssertionError("no quadruple gives the wanted inliers")

    is_b, is_a = np.arange(n) < nb, (np.arange(n) >= nb) & (np.arange(n) < nb + na)
    quads_b, quad_a = gated(0, nb, is_b, 2), gated(nb, nb + na, is_a, 1)[0]
    quad_junk = [nb + na, nb + na + 1, 0, nb]
    assert M.check_inliers(*M.epnp(corr, K, quad=quad_junk), K, corr)[1] < mi
    corr.setflags(write=False)
    _two[key] = dict(corr=corr, mi=mi, quads_b=quads_b, quad_a=quad_a, quad_junk=quad_junk, is_a=is_a, is_b=is_b)
    return _two[key]


#        name             n    n_hyp  seed  outliers noise  minInliers epsilon planar
CASES = [("n4_h1",        4,    1,    11,   0.0,    0.0,   4,         0.5,    False),
         ("n5_h5",        5,    5,    12,   0.0,    0.3,   5,         0.5,    False),
         ("n20_h1",       20,   1,    13,   0.2,    0.3,   10,        0.5,    False),
         ("n20_h5",       20,   5,    14,   0.3,    0.5,   10,        0.5,    False),
         ("n63_h5",       63,   5,    15,   0.3,    0.5,   10,        0.5,    False),
         ("n64_h5",       64,   5,    16,   0.3,    0.5,   10,        0.5,    False),
         ("n65_h300",     65,   300,  17,   0.45,   0.7,   10,        0.5,    False),
         ("n129_h5",      129,  5,    18,   0.3,    0.5,   10,        0.5,    False),
         ("n300_h300",    300,  300,  19,   0.7,    0.7,   10,        0.5,    False),
         ("n1000_h5",     1000, 5,    20,   0.3,    0.5,   10,        0.5,    False),
         ("planar_n100_h5", 100, 5,   21,   0.2,    0.3,   10,        0.5,    True)]
ALL_NAMES = [c[0] for c in CASES]

# Cases whose hypotheses reach the minimum, so that k_pnp_refine runs on masks of 3, 5, 16 and 65 words (none of the eleven above refines past one bit
# of a second word), and planar sets that reach the refine: exact (ABt has rank 2, the pose is finite) and noisy (det < 0 is flipped, every refine
# fails).  With them go first_in_word1 and planar_lattice below.  tests/pnp_checks.py (check_refine_case) asserts from the model what each must provide.
REFINE_CASES = [("refine_n129",  129,  20,   49,   0.2,    0.3,   10,        0.5,    False),      # (seed 41 leaves bit 128, the third word's only one, clear)
                ("refine_n300",  300,  20,   42,   0.2,    0.3,   10,        0.5,    False),
                ("refine_n1000", 1000, 20,   43,   0.2,    0.3,   10,        0.5,    False),
                ("refine_n4160", 4160, 6,    48,   0.2,    0.3,   10,        0.5,    False),
                ("planar_exact", 100,  40,   45,   0.0,    0.0,   10,        0.5,    True),
                ("planar_failing_refines", 200, 40, 46, 0.1, 0.3, 10,        0.5,    True)]
REFINE_NAMES = [c[0] for c in REFINE_CASES] + ["refine_first_in_word1", "planar_lattice"]


def first_in_word1():
    """200 correspondences of which the first 70 are wrong and no hypothesis draws them: every mask a refine takes starts in its second word"""
    corr, Rcw, tcw, _ = scene(200, 47, 0.1, 0.3)
    rng = np.random.default_rng(1)
    corr[:70, 3], corr[:70, 4] = rng.uniform(0.0, W, 70).astype(f32), rng.uniform(0.0, H, 70).astype(f32)
    return corr, (70 + draw_quads(130, 20, 47)).astype(np.int32), 60, Rcw, tcw


def planar_lattice(n=100, nh=10, seed=0):
    """Points that float32 holds exactly on one world plane, z = 5 + x / 4 + y / 2 with x, y multiples of 1 / 256, seen without noise: the smallest
    eigenvalue of PW0^T PW0 is rounding alone, so the stated Jacobi returns it below zero about as often as above.  Below zero it is clamped, the third
    control point falls on the centroid, CC is singular and the pose not finite; scene(planar=True) never gets there in a refine,
    because rounding its world points to float32 lifts them off their wall by more than the eigen-solver's error."""
    rng = np.random.default_rng(seed)
    Rcw, tcw = pose(rng)
    fx, fy, cx, cy = [float(k) for k in K]
    xy = rng.integers(-384, 385, (n, 2)).astype(np.float64) / 256.0
    Xw = np.stack([xy[:, 0], xy[:, 1], 5.0 + xy[:, 0] / 4.0 + xy[:, 1] / 2.0], 1)
    assert np.array_equal(Xw.astype(f32).astype(np.float64), Xw)
    Pc = Xw @ Rcw.T + tcw
    corr = np.zeros((n, 6), f32)
    corr[:, 0:3], corr[:, 3], corr[:, 4] = Xw.astype(f32), (cx + fx * Pc[:, 0] / Pc[:, 2]).astype(f32), (cy + fy * Pc[:, 1] / Pc[:, 2]).astype(f32)
    corr[:, 5] = M.max_errors(np.ones(n, f32), TH2)
    return corr, draw_quads(n, nh, seed), M.ransac_parameters(n, 0.99, 10, 300, 4, 0.5)[0], Rcw, tcw


def case(name):
    """(corr, quads, min_inliers, Rcw, tcw)"""
    _, n, nh, seed, outliers, noise, mi, eps, planar = CASES[ALL_NAMES.index(name)]
    corr, Rcw, tcw, _ = scene(n, seed, outliers, noise, planar)
    return corr, draw_quads(n, nh, seed), M.ransac_parameters(n, 0.99, mi, 300, 4, eps)[0], Rcw, tcw


def refine_case(name):
    """(corr, quads, min_inliers, Rcw, tcw) of one of REFINE_NAMES"""
    if name == "refine_first_in_word1":
        return first_in_word1()
    if name == "planar_lattice":
        return planar_lattice(100, 10, 68)
    _, n, nh, seed, outliers, noise, mi, eps, planar = REFINE_CASES[REFINE_NAMES.index(name)]
    corr, Rcw, tcw, _ = scene(n, seed, outliers, noise, planar)
    return corr, draw_quads(n, nh, seed), M.ransac_parameters(n, 0.99, mi, 300, 4, eps)[0], Rcw, tcw
