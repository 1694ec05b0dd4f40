"""Seeded scenes for Initializer::Initialize (tests/init_model.py, tests/init_checks.py): two views of a 3-D scene or a plane, half a pixel of noise,
some gross outliers, key points of each frame beyond the matched ones (Normalize runs over all of them), sets drawn with the reference's
swap-remove.  Every case is a pure function of its name."""
import numpy as np

import init_model as M

f32 = np.float32
K = np.array([517.306408, 516.469215, 318.643040, 255.313989], f32)              # fx, fy, cx, cy (TUM1.yaml)
W, H = 640.0, 480.0


def rot(axis, deg):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def project(X):
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)


# kind: how the points lie; R, t: the second camera (x2 = R x1 + t); the rest: sizes and disturbances
SCENES = {
    # name: (kind, n, n_sets, seed, dict of options)
    "general_300": ("general", 300, 200, 1, {}),
    "plane_300": ("plane", 300, 200, 2, dict(tilt=1.4)),
    "fronto_300": ("fronto", 300, 64, 3, dict(noise=0.0, outliers=0.0, t=(0.0, 0.0, 0.0), R=("y", 0.0))),
    "rotation_300": ("general", 300, 200, 4, dict(t=(0.0, 0.0, 0.0), R=("y", 3.0))),
    "outliers40_300": ("general", 300, 201, 5, dict(outliers=0.4)),
    "behind_300": ("general", 300, 200, 6, dict(behind=0.2, outliers=0.02)),
    "similar_80": ("far", 80, 64, 110, dict(outliers=0.02, min_tri=10, far=0.6)),
    "farkept_80": ("far", 80, 64, 128, dict(outliers=0.02, min_tri=10, far=0.3)),
    "lowpar_80": ("far", 80, 64, 104, dict(outliers=0.02, min_tri=10, far=0.6)),
    "general_mode1": ("general", 129, 65, 8, dict(mode=1)),
    "plane_mode1": ("plane", 128, 63, 9, dict(mode=1, tilt=1.4)),
    "n8": ("general", 8, 1, 10, dict(outliers=0.0, min_tri=5)),
    "n9": ("general", 9, 63, 11, dict(outliers=0.0, min_tri=5)),
    "n63": ("general", 63, 64, 12, dict(min_tri=30)),
    "n64": ("plane", 64, 65, 13, dict(min_tri=30, tilt=1.4)),
    "n65": ("general", 65, 200, 14, dict(min_tri=30)),
    "n1000": ("general", 1000, 64, 15, {}),
    "good52": ("general", 52, 64, 16, dict(outliers=0.0, noise=0.1, min_tri=10)),
    "good51": ("general", 51, 64, 17, dict(outliers=0.0, noise=0.1, min_tri=10)),
    "good50": ("general", 50, 64, 18, dict(outliers=0.0, noise=0.1, min_tri=10)),
    # little noise and no outliers: these reconstruct whatever sets are drawn (tests/init_cpp draws its own)
    "clean_f": ("general", 120, 64, 31, dict(noise=0.1, outliers=0.0)),
    "clean_h": ("plane", 120, 64, 32, dict(noise=0.1, outliers=0.0, tilt=1.4)),
}
GRADED = ["general_300", "plane_300", "fronto_300", "rotation_300", "outliers40_300", "behind_300", "lowpar_80"]
ALL_NAMES = list(SCENES)
_cache = {}


def rand_from(rng):
    return lambda lo, hi: int(rng.integers(lo, hi + 1))


def case(name):
    """dict: K, matches (n x 4), sets, norm1, norm2, sigma, min_parallax, min_triangulated, gemm_mode, and the truth (R, t, inlier flags)"""
    if name in _cache:
        return _cache[name]
    kind, n, ns, seed, opt = SCENES[name]
    rng = np.random.default_rng(1000 + seed)
    noise, outliers = opt.get("noise", 0.5), opt.get("outliers", 0.1)
    axis, deg = opt.get("R", ("y", -8.0))
    R = rot({"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1)}[axis], deg) @ rot((1, 0.3, 0.2), 1.5 if deg else 0.0)
    t = np.asarray(opt.get("t", (1.2, 0.15, 0.3)), float)
    X = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n), rng.uniform(3.0, 10.0, n)], 1)
    if kind == "plane":
        X[:, 2] = 5.0 + opt.get("tilt", 0.7) * X[:, 0] + 0.3 * X[:, 1]
    elif kind == "fronto":
        X[:, 2] = 5.0
    elif kind == "far":                                                         # most points too far for any parallax: every motion hypothesis keeps them
        far = rng.random(n) < opt.get("far", 0.62)
        X[far] *= (400.0 / X[far, 2])[:, None]
    nb = int(opt.get("behind", 0.0) * n)
    if nb:                                                                      # epipolar-consistent matches of points behind both cameras
        X[:nb] = -X[:nb] - np.array([0.0, 0.0, 2.0])
    x1, x2 = project(X), project(X @ R.T + t)
    x1 += rng.normal(0, noise, x1.shape) if noise else 0.0
    x2 += rng.normal(0, noise, x2.shape) if noise else 0.0
    inlier = np.ones(n, bool)
    no = int(outliers * n)
    if no:
        bad = rng.choice(np.arange(nb, n), no, replace=False)
        x2[bad] = np.stack([rng.uniform(0, W, no), rng.uniform(0, H, no)], 1)
        inlier[bad] = False
    matches = np.ascontiguousarray(np.concatenate([x1, x2], 1), f32)
    extra = 5 + n // 4                                                          # key points without a match, in both frames
    keys1 = np.concatenate([matches[:, 0:2], np.stack([rng.uniform(0, W, extra), rng.uniform(0, H, extra)], 1).astype(f32)])
    keys2 = np.concatenate([np.stack([rng.uniform(0, W, extra), rng.uniform(0, H, extra)], 1).astype(f32), matches[:, 2:4]])
    sets = M.draw_sets(n, ns, rand_from(rng))
    c = dict(K=K, matches=matches, sets=sets, norm1=M.normalize(keys1), norm2=M.normalize(keys2), sigma=1.0, min_parallax=1.0,
             min_triangulated=opt.get("min_tri", 50), gemm_mode=opt.get("mode", 0), truth=dict(R=R, t=t, X=X, inlier=inlier, behind=nb))
    for a in (matches, sets, c["norm1"], c["norm2"]):
        a.setflags(write=False)
    _cache[name] = c
    return c


def arguments(c):
    return {k: c[k] for k in ("K", "matches", "sets", "norm1", "norm2", "sigma", "min_parallax", "min_triangulated", "gemm_mode")}


# ------------------------------------------------------------------------------------------------ an independent restatement, in float64 with numpy.linalg
def independent_null_vectors(matches, sets, norm1, norm2, is_f):
    """per set the unit null vector of the reference's A: A in float as the reference builds it (written here a second time, apart from the model),
    numpy.linalg.svd of the widened A in float64"""
    m = np.asarray(matches, f32)
    out = []
    for st in np.asarray(sets):
        rows = []
        for i in st:
            u1, v1 = f32(f32(m[i, 0] - norm1[0]) * norm1[2]), f32(f32(m[i, 1] - norm1[1]) * norm1[3])
            u2, v2 = f32(f32(m[i, 2] - norm2[0]) * norm2[2]), f32(f32(m[i, 3] - norm2[1]) * norm2[3])
            if is_f:
                rows.append([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, f32(1)])
            else:
                rows.append([0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2])
                rows.append([u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2])
        A = np.array(rows, f32).astype(np.float64)
        sv = np.linalg.svd(A, compute_uv=False)
        full = np.concatenate([sv, np.zeros(9 - len(sv))]) ** 2
        out.append((np.linalg.svd(A)[2][8], full[7] / full[0]))                  # the vector; second-smallest over largest eigenvalue of A^T A
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def _score_h(H, m, sigma):
    Hi = np.linalg.inv(H)
    x1, x2 = np.c_[m[:, 0:2], np.ones(len(m))], np.c_[m[:, 2:4], np.ones(len(m))]
    a, b = x2 @ Hi.T, x1 @ H.T
    c1 = ((m[:, 0:2] - a[:, :2] / a[:, 2:]) ** 2).sum(1) / sigma ** 2
    c2 = ((m[:, 2:4] - b[:, :2] / b[:, 2:]) ** 2).sum(1) / sigma ** 2
    return np.where(c1 > 5.991, 0, 5.991 - c1).sum() + np.where(c2 > 5.991, 0, 5.991 - c2).sum(), ~(c1 > 5.991) & ~(c2 > 5.991)


def _score_f(F, m, sigma):
    x1, x2 = np.c_[m[:, 0:2], np.ones(len(m))], np.c_[m[:, 2:4], np.ones(len(m))]
    l2, l1 = x1 @ F.T, x2 @ F
    c1 = (l2 * x2).sum(1) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2) / sigma ** 2
    c2 = (l1 * x1).sum(1) ** 2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2) / sigma ** 2
    return np.where(c1 > 3.841, 0, 5.991 - c1).sum() + np.where(c2 > 3.841, 0, 5.991 - c2).sum(), ~(c1 > 3.841) & ~(c2 > 3.841)


def _aligned_svd(A, like):
    """numpy's U, s, V with the signs of the model's decomposition (`like`: its U, V, H21, F21): the enumeration of the motion hypotheses follows the signs, which
    no decomposition defines; nothing else is taken from the model"""
    U, s, Vt = np.linalg.svd(A)
    V = Vt.T.copy()
    if like is not None:
        Um, Vm = like[0], like[1]
        for c in range(3):
            if np.dot(U[:, c], Um[:, c].astype(float)) < 0:
                U[:, c] = -U[:, c]
                if c < 2 or s[2] > 1e-6 * s[0]:
                    V[:, c] = -V[:, c]
        if np.dot(V[:, 2], Vm[:, 2].astype(float)) < 0 and not s[2] > 1e-6 * s[0]:
            V[:, 2] = -V[:, 2]
    return U, s, V


def _check_rt(R, t, Km, m, mask, sigma):
    P1, P2 = Km @ np.c_[np.eye(3), np.zeros(3)], Km @ np.c_[R, t]
    O2 = -R.T @ t
    good, cos, pts, tri = 0, [], np.zeros((len(m), 3)), np.zeros(len(m), bool)
    for i in np.flatnonzero(mask):
        A = np.array([m[i, 0] * P1[2] - P1[0], m[i, 1] * P1[2] - P1[1], m[i, 2] * P2[2] - P2[0], m[i, 3] * P2[2] - P2[1]])
        x = np.linalg.svd(A)[2][3]
        X = x[:3] / x[3]
        if not np.isfinite(X).all():
            continue
        n1, n2 = X, X - O2
        c = n1 @ n2 / (np.linalg.norm(n1) * np.linalg.norm(n2))
        X2 = R @ X + t
        if (X[2] <= 0 or X2[2] <= 0) and c < 0.99998:
            continue
        p1, p2 = Km @ X, Km @ X2
        if ((p1[:2] / p1[2] - m[i, 0:2]) ** 2).sum() > 4 * sigma ** 2 or ((p2[:2] / p2[2] - m[i, 2:4]) ** 2).sum() > 4 * sigma ** 2:
            continue
        good += 1; cos.append(c); pts[i] = X; tri[i] = c < 0.99998
    par = np.rad2deg(np.arccos(sorted(cos)[min(50, len(cos) - 1)])) if good else 0.0
    return good, par, pts, tri


def independent(c, like=None):
    """Initialize in float64 with numpy.linalg on the case's matches, sets and normalisation: a dict with returned, model, RH, best_mot, R21, t21,
    triangulated"""
    m, sets, sigma = c["matches"].astype(float), c["sets"], float(c["sigma"])
    n1, n2 = c["norm1"].astype(float), c["norm2"].astype(float)
    T1 = np.array([[n1[2], 0, -n1[0] * n1[2]], [0, n1[3], -n1[1] * n1[3]], [0, 0, 1]])
    T2 = np.array([[n2[2], 0, -n2[0] * n2[2]], [0, n2[3], -n2[1] * n2[3]], [0, 0, 1]])
    vh, vf = independent_null_vectors(c["matches"], sets, c["norm1"], c["norm2"], False)[0], independent_null_vectors(c["matches"], sets, c["norm1"], c["norm2"], True)[0]
    SH = SF = 0.0
    H = F = mh = mf = None
    for h in range(len(sets)):
        Hc = np.linalg.inv(T2) @ vh[h].reshape(3, 3) @ T1
        s, mask = _score_h(Hc, m, sigma)
        if s > SH:
            SH, H, mh = s, Hc, mask
        U, w, Vt = np.linalg.svd(vf[h].reshape(3, 3))
        Fc = T2.T @ (U @ np.diag([w[0], w[1], 0.0]) @ Vt) @ T1
        s, mask = _score_f(Fc, m, sigma)
        if s > SF:
            SF, F, mf = s, Fc, mask
    RH = SH / (SH + SF)
    if like is not None:                                                        # the sign of a null vector is free, and H and F inherit it
        H = -H if H is not None and (H * like[2].astype(float)).sum() < 0 else H
        F = -F if F is not None and (F * like[3].astype(float)).sum() < 0 else F
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], float)
    out = dict(returned=0, model=0 if RH > 0.40 else 1, RH=RH, best_mot=-1, R21=None, t21=None, triangulated=np.zeros(len(m), bool))
    mots = []
    if out["model"] == 0:
        U, w, V = _aligned_svd(np.linalg.inv(Km) @ H @ Km, like)
        s = np.linalg.det(U) * np.linalg.det(V.T)
        d1, d2, d3 = w
        if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
            return out
        a1, a3 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        for sign, (cth, ast, scale) in ((1, ((d2 * d2 + d1 * d3) / ((d1 + d3) * d2), np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2), d1 - d3)),
                                        (-1, ((d1 * d3 - d2 * d2) / ((d1 - d3) * d2), np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2), d1 + d3))):
            for e1, e3, es in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)):
                if sign > 0:
                    Rp = np.array([[cth, 0, -es * ast], [0, 1, 0], [es * ast, 0, cth]])
                    tp = np.array([e1 * a1, 0, -e3 * a3]) * scale
                else:
                    Rp = np.array([[cth, 0, es * ast], [0, -1, 0], [es * ast, 0, -cth]])
                    tp = np.array([e1 * a1, 0, e3 * a3]) * scale
                t = U @ tp
                mots.append((s * U @ Rp @ V.T, t / np.linalg.norm(t)))
        mask = mh
    else:
        U, w, V = _aligned_svd(Km.T @ F @ Km, like)
        W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
        t = U[:, 2] / np.linalg.norm(U[:, 2])
        R1, R2 = U @ W @ V.T, U @ W.T @ V.T
        R1, R2 = (R1 if np.linalg.det(R1) > 0 else -R1), (R2 if np.linalg.det(R2) > 0 else -R2)
        mots = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
        mask = mf
    N = int(mask.sum())
    res = [_check_rt(R, t, Km, m, mask, sigma) for R, t in mots]
    good = [r[0] for r in res]
    ok, best = False, -1
    if out["model"] == 1:
        mx = max(good)
        if not (mx < max(int(0.9 * N), c["min_triangulated"]) or sum(g > 0.7 * mx for g in good) > 1):
            best = good.index(mx)
            ok = res[best][1] > c["min_parallax"]
    else:
        bg = sg = 0
        for k, g in enumerate(good):
            if g > bg:
                sg, bg, best = bg, g, k
            elif g > sg:
                sg = g
        ok = best >= 0 and sg < 0.75 * bg and res[best][1] >= c["min_parallax"] and bg > c["min_triangulated"] and bg > 0.9 * N
    out.update(returned=int(ok), best_mot=best, good=good)
    if ok:
        out.update(R21=mots[best][0], t21=mots[best][1], triangulated=res[best][3])
    return out
