"""Seeded problems for the OptimizeSim3 tests: two cameras with different intrinsics, a true S12 (X1 = s R X2 + t), points in front of both cameras, pixel
noise scaled by the level's sigma, gross outliers in one image or in both, and a perturbed initial S12 whose quaternion is taken from the FLOAT rotation
matrix as LoopClosing.cc:325 does (g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s): Eigen's Quaternion(Matrix3), not normalised afterwards).
case(name, seed) is a pure function of its arguments; tests/golden/sim3_opt_spread.npz records which seed each case uses (the first of 0..15 whose flags and
return value no order of the sums and no last-bit change of exp / sin / cos can move, tests/golden/make_golden_sim3_opt_spread.py)."""
import numpy as np

import sim3_opt_model as M
from pose_opt_cases import axis_angle, inv_level_sigma2, NLEVELS, SCALE

WORKGROUP = 256                                                                # S3O_T of orb_slam2_amd/csrc/orbhip_sim3_opt.hip
STAGE_MAX = 1024                                                               # S3O_STAGE_MAX: pairs staged in LDS up to here
SIZES = (1, 9, 10, 11, 63, 64, 65, 255, 256, 257, STAGE_MAX - 1, STAGE_MAX, STAGE_MAX + 1, 5000)
SHARES = (0.0, 0.3)
SCALES = (0.6, 1.0, 1.7)
CAMS = np.array([520.9, 521.0, 325.1, 249.7, 458.6, 457.3, 367.2, 248.4], np.float32)      # fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2


def _rot(w):
    return M.mul(M.sim3_exp(list(w) + [0.0] * 4), ((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0), 1.0))[0]


def rotation_matrix(q):
    """the matrix of v -> q * v (Eigen's Quaternion * Vector3), for any q"""
    return np.stack(M.rotate(q, *np.eye(3)), 0)


def make(n, share, fix_scale, seed, scale=1.0, noise=1.0, perturb=(0.02, 0.05, 0.03), gross=(15.0, 80.0), which=None, th2=10.0, turn=None, inv_sigma2=None,
         behind=(), qnorm=None):
    """(cams, S12_init float64[8], pairs float32[n, 12], th2, fix_scale, info).  The scene is a cube of side 6 centred 8 in front of camera 1 and 8 / s in
    front of camera 2, whatever the rotation between the two, so every point is in front of both.
      perturb = (rotation, translation, log scale) standard deviations of the initial S12 about the true one (no scale perturbation under fix_scale);
      which   = None: a gross outlier is wrong in image 1, in image 2 or in both (drawn); 1 or 2: in that image alone;
      turn    = (Rtarget, exact): the true rotation is Rtarget and the initial one dR Rtarget - or, if exact, the initial one is Rtarget itself;
      behind  = these pairs' X2 are mirrored so that S12_init.map(X2) lies behind camera 1;  qnorm: the initial quaternion is multiplied by it."""
    rng = np.random.default_rng([n, int(round(share * 100)), int(fix_scale), seed])
    is2 = inv_level_sigma2()
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = CAMS.astype(np.float64)
    Rt = rotation_matrix(_rot(rng.normal(0, 0.3, 3)))
    dR = rotation_matrix(_rot(rng.normal(0, perturb[0], 3))); dt = rng.normal(0, perturb[1], 3); ds = 0.0 if fix_scale else rng.normal(0, perturb[2])
    R0 = dR @ Rt
    if turn is not None:
        Rtarget, exact = turn
        Rt, R0 = (dR.T @ Rtarget, np.asarray(Rtarget, np.float64)) if exact else (np.asarray(Rtarget, np.float64), dR @ Rtarget)
    c1 = np.array([0.0, 0.0, 8.0]) + rng.normal(0, 0.2, 3); c2 = np.array([0.0, 0.0, 8.0 / scale]) + rng.normal(0, 0.2, 3)
    tt = c1 - scale * (Rt @ c2)
    X1 = (c1 + rng.uniform(-3.0, 3.0, (n, 3))).astype(np.float32)
    X2 = (((X1.astype(np.float64) - tt) @ Rt) / scale).astype(np.float32)                 # Rt^T (X1 - t) / s
    y1 = scale * (X2.astype(np.float64) @ Rt.T) + tt
    y2 = ((X1.astype(np.float64) - tt) @ Rt) / scale
    assert (y1[:, 2] > 1.0).all() and (y2[:, 2] > 1.0 / scale).all()
    u1 = y1[:, 0] / y1[:, 2] * fx1 + cx1; v1 = y1[:, 1] / y1[:, 2] * fy1 + cy1
    u2 = y2[:, 0] / y2[:, 2] * fx2 + cx2; v2 = y2[:, 1] / y2[:, 2] * fy2 + cy2
    oct1 = rng.integers(0, NLEVELS, n); oct2 = rng.integers(0, NLEVELS, n)
    s1 = noise * np.float64(np.float32(SCALE)) ** oct1; s2 = noise * np.float64(np.float32(SCALE)) ** oct2
    u1 = u1 + rng.normal(0, 1, n) * s1; v1 = v1 + rng.normal(0, 1, n) * s1; u2 = u2 + rng.normal(0, 1, n) * s2; v2 = v2 + rng.normal(0, 1, n) * s2
    is_gross = np.zeros(n, int)                                                 # 0: none, 1: image 1, 2: image 2, 3: both
    ng = int(round(share * n))
    if ng:
        g = rng.choice(n, ng, replace=False)
        is_gross[g] = rng.integers(1, 4, ng) if which is None else which
        ang = rng.uniform(0, 2 * np.pi, (2, ng)); r = rng.uniform(gross[0], gross[1], (2, ng))
        m1 = (is_gross[g] & 1) != 0; m2 = (is_gross[g] & 2) != 0
        u1[g] += np.where(m1, r[0] * (1.0 + oct1[g]) * np.cos(ang[0]), 0.0); v1[g] += np.where(m1, r[0] * (1.0 + oct1[g]) * np.sin(ang[0]), 0.0)
        u2[g] += np.where(m2, r[1] * (1.0 + oct2[g]) * np.cos(ang[1]), 0.0); v2[g] += np.where(m2, r[1] * (1.0 + oct2[g]) * np.sin(ang[1]), 0.0)
    w1 = is2[oct1].astype(np.float64); w2 = is2[oct2].astype(np.float64)
    if inv_sigma2 is not None:
        w1[:] = inv_sigma2; w2[:] = inv_sigma2
    pairs = np.concatenate([np.stack([u1, v1, w1, u2, v2, w2], 1), X1.astype(np.float64), X2.astype(np.float64)], 1).astype(np.float32)
    # LoopClosing.cc:319-325: R, t float Mats, s a float; gScm(toMatrix3d(R), toVector3d(t), s)
    t0 = (dR @ tt + dt).astype(np.float32).astype(np.float64)
    s0 = float(np.float32(scale * np.exp(ds)))
    S0 = M.sim3_of_matrix(R0.astype(np.float32).astype(np.float64), t0, s0)
    S12 = M.to_array(S0)
    if qnorm is not None:
        S12[:4] *= qnorm
    for i in behind:
        Sq = M.to_sim3(S12)
        p = np.array(M.smap(Sq, *pairs[i, 9:12].astype(np.float64)))
        p[2] = -p[2]
        pairs[i, 9:12] = np.array(M.smap(M.inverse(Sq), *p)).astype(np.float32)
    info = {"S_true": (Rt, tt, scale), "gross": is_gross, "oct": (oct1, oct2)}
    return CAMS.copy(), S12, pairs, np.float32(th2), bool(fix_scale), info


ZERO_CAMS = np.array([512.0, 512.0, 320.0, 240.0, 256.0, 256.0, 300.0, 200.0], np.float32)
ZERO_S12 = np.array([0.0, 0.0, 0.0, 1.0, 1.0, -0.5, 0.0, 2.0])


def zero_residual():
    """40 pairs whose two projections at S12 = (identity rotation, t = (1, -1/2, 0), s = 2) are exact in every format the kernel uses: X2's x and y are
    multiples of 1/4, its z a power of two, X1 = 2 X2 + t, focal lengths powers of two.  Every residual is exactly 0: chi = tempChi = 0, x = 0, the trial
    equals the estimate and both phases end by rho == 0.  There is no seed: the problem is one."""
    i = np.arange(40)
    X2 = np.stack([((2 * i) % 9 - 4) / 4.0, ((5 * i) % 7 - 3) / 4.0, 2.0 ** (1 + i % 3)], 1)
    X1 = 2.0 * X2 + ZERO_S12[4:7]
    fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2 = ZERO_CAMS.astype(np.float64)
    p64 = np.concatenate([np.stack([X1[:, 0] / X1[:, 2] * fx1 + cx1, X1[:, 1] / X1[:, 2] * fy1 + cy1, np.ones(40),
                                    X2[:, 0] / X2[:, 2] * fx2 + cx2, X2[:, 1] / X2[:, 2] * fy2 + cy2, np.ones(40)], 1), X1, X2], 1)
    pairs = p64.astype(np.float32)
    assert np.array_equal(pairs.astype(np.float64), p64) and len(np.unique(pairs[:, 9:12], axis=0)) == 40
    return ZERO_CAMS.copy(), ZERO_S12.copy(), pairs, np.float32(10.0), False, {"S_true": (np.eye(3), ZERO_S12[4:7].copy(), 2.0), "gross": np.zeros(40, int)}


def key(n, share, fix):
    return f"n{n}_o{int(round(share * 100))}_f{int(fix)}"


GRID = [(n, share, fix) for n in SIZES for share in SHARES for fix in (0, 1)]

TURN_PI = {"x": np.diag([1.0, -1.0, -1.0]), "y": np.diag([-1.0, 1.0, -1.0]), "z": np.diag([-1.0, -1.0, 1.0])}
TURN_AXES = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0)}
_B = dict(n=120, share=0.3, fix_scale=False)
BEHIND = (3, 4, 70)
# named cases: what each is there for is checked by tests/golden/make_golden_sim3_opt_spread.py (shows())
EXTRA = {
    "no_removal": dict(n=60, share=0.0, fix_scale=False, noise=0.3),                                  # the second phase is optimize(5)
    "left_9": dict(n=12, share=0.25, fix_scale=False, noise=0.3),                                     # 3 gross of 12: 9 pairs left after the first check, the early return
    "left_10": dict(n=13, share=3.0 / 13.0, fix_scale=False, noise=0.3),                              # 3 gross of 13: 10 left, the second phase runs
    "all_removed": dict(n=40, share=0.0, fix_scale=False, inv_sigma2=1e30),                           # an information of 1e30 per pixel^2 removes every pair
    "forward_only": dict(_B, which=1, scale=1.7),                                                     # pairs whose forward edge alone exceeds th2
    "inverse_only": dict(_B, which=2, scale=0.6),                                                     # ... whose inverse edge alone does
    "far_start": dict(n=90, share=0.1, fix_scale=True, perturb=(0.6, 1.5, 0.4), noise=0.3, scale=1.7),  # rejected trials, a phase ending on a rejected trial
    "far_start_free": dict(_B, perturb=(0.4, 1.2, 0.3)),                                              # ... and a far start with the scale free
    "near_th2": dict(n=200, share=0.4, fix_scale=False, gross=(1.5, 4.0), perturb=(0.05, 0.2, 0.05)),  # outliers close to th2
    "th2_4": dict(_B, th2=4.0),
    "quat_norm_plus": dict(_B, qnorm=1.0 + 1e-7),
    "quat_norm_minus": dict(_B, qnorm=1.0 - 1e-7, fix_scale=True),
    "behind_camera": dict(_B, behind=BEHIND),
    "zero_residual": None,
}
TURNED = []
for _a in "xyz":
    for _s in (1, -1):
        _name = f"turn_{_a}_{'m' if _s < 0 else 'p'}130"
        EXTRA[_name] = dict(_B, turn=(axis_angle(TURN_AXES[_a], _s * 130.0), False), scale=SCALES["xyz".index(_a)])
        TURNED.append(_name)
    EXTRA[f"turn_{_a}_pi_exact"] = dict(_B, turn=(TURN_PI[_a], True), fix_scale=_a == "y")
    TURNED.append(f"turn_{_a}_pi_exact")


def case_args(name):
    if name in EXTRA:
        return dict(EXTRA[name])
    n, share, fix = name.split("_")
    n = int(n[1:])
    return dict(n=n, share=int(share[1:]) / 100.0, fix_scale=bool(int(fix[1:])), scale=SCALES[SIZES.index(n) % 3])


ALL_NAMES = [key(*g) for g in GRID] + list(EXTRA)


def case(name, seed):
    if name == "zero_residual":
        return zero_residual()
    return make(seed=seed, **case_args(name))


def deviation(Sa, Sb):
    """(rotation angle between the two quaternions' rotations, largest |translation entry difference|, |scale difference|) of two S12 arrays"""
    Sa = np.asarray(Sa, np.float64); Sb = np.asarray(Sb, np.float64)
    qa = Sa[:4] / np.sqrt((Sa[:4] ** 2).sum()); qb = Sb[:4] / np.sqrt((Sb[:4] ** 2).sum())
    # the vector part of qa * conj(qb): sin(angle / 2) to first order exact where cos would lose every digit
    ax, ay, az, aw = qa; bx, by, bz, bw = -qb[0], -qb[1], -qb[2], qb[3]
    v = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx])
    w = aw * bw - ax * bx - ay * by - az * bz
    return float(2.0 * np.arctan2(np.sqrt((v * v).sum()), abs(w))), float(np.abs(Sa[4:7] - Sb[4:7]).max()), float(abs(Sa[7] - Sb[7]))
