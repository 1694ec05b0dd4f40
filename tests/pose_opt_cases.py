"""Seeded problems for the pose-optimisation tests: a camera, a true pose, points in front of it, pixel noise scaled by the level's sigma, gross outliers and
a perturbed initial pose; optionally the world frame turned, points mirrored behind the camera, one information for all, a float-product pose.  case(name, seed) is a pure function of its arguments; tests/golden/pose_opt_spread.npz records which seed each
(n, mix, share) uses (the first whose outcome no summation order can change, tests/golden/make_golden_pose_opt_spread.py)."""
import numpy as np

import pose_opt_model as M

WORKGROUP = 256                                                                # PO_T of orb_slam2_amd/csrc/orbhip_pose_opt.hip
STAGE_MAX = 2048                                                               # PO_STAGE_MAX: observations staged in LDS up to here
SIZES = (3, 9, 10, 63, 64, 65, 255, 256, 257, 2000, 5000)                      # (255 and 257 are the workgroup size -+ 1; 5000 is past the staging limit)
MIXES = ("mono", "stereo", "mixed")
SHARES = (0.0, 0.3)
CAM = np.array([520.9, 521.0, 325.1, 249.7, 40.0], np.float32)                 # fx, fy, cx, cy, bf
W, H = 640, 480
NLEVELS, SCALE = 8, 1.2


def inv_level_sigma2():
    """mvInvLevelSigma2 as ORBextractor computes it (ORBextractor.cc:418-434): float tables, the scale factor a double"""
    sf = np.ones(NLEVELS, np.float32); s2 = np.ones(NLEVELS, np.float32)
    for i in range(1, NLEVELS):
        sf[i] = np.float32(np.float64(sf[i - 1]) * np.float64(np.float32(SCALE)))
        s2[i] = sf[i] * sf[i]
    return (np.float32(1.0) / s2).astype(np.float32)


def _rot(w):
    q, _ = M.oplus(np.concatenate([w, np.zeros(3)]), (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)))
    return M.rotation_matrix(q)


def axis_angle(axis, deg):
    """the double rotation matrix of an angle (degrees) about an axis, by Rodrigues' formula: no quaternion, nothing of pose_opt_model"""
    a = np.asarray(axis, np.float64); a = a / np.sqrt((a * a).sum())
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = np.radians(np.float64(deg))
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def float_product(A, B):
    """the 4 x 4 product of two float poses in float arithmetic, one multiplication and one addition after the other (so the bits do not depend on a BLAS)"""
    A = np.asarray(A, np.float32); B = np.asarray(B, np.float32)
    out = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            acc = np.float32(0.0)
            for k in range(4):
                acc = np.float32(acc + np.float32(A[i, k] * B[k, j]))
            out[i, j] = acc
    return out


def make(n, mix, share, seed, noise=1.0, perturb=(0.02, 0.05), gross=(15.0, 80.0), depth=(2.0, 20.0), reframe=None, inv_sigma2=None, behind=(), motion=None):
    """(cam, Tcw_init float32 4x4, obs float32 [n, 7], info): info has the true pose, the octaves and which observations are gross outliers.
    The last four arguments change the finished problem and draw nothing from the generator, so a case without them keeps its bits:
      reframe = (Rtarget, perturbed)  the world frame is turned so that the initial rotation is dR Rtarget (dR the case's own perturbation, or the identity
                                      if not perturbed): with pc = R0 Xw + t0 the camera-frame points at the initial pose (double), the points become
                                      float(R'^T (pc - t0)); observations and t0 stay, so the camera-frame geometry is the same up to that rounding;
      inv_sigma2                      every observation's information is set to this value;
      behind                          these points are mirrored to z < 0 in the initial camera frame (wrong matches; everything stays finite);
      motion                          the initial pose becomes the FLOAT product motion * Tcw_init (mVelocity * mLastFrame.mTcw)."""
    rng = np.random.default_rng([n, MIXES.index(mix), int(round(share * 100)), seed])
    is2 = inv_level_sigma2()
    fx, fy, cx, cy, bf = CAM.astype(np.float64)
    Rt = _rot(rng.normal(0, 0.3, 3)); tt = rng.normal(0, 1.0, 3)
    T_true = np.eye(4); T_true[:3, :3] = Rt; T_true[:3, 3] = tt
    u = rng.uniform(20, W - 20, n); v = rng.uniform(20, H - 20, n); z = rng.uniform(depth[0], depth[1], n)
    pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    pw = ((pc - tt) @ Rt).astype(np.float32)                                   # Rt^T (pc - t); stored as float, as MapPoint::GetWorldPos returns it
    pc = pw.astype(np.float64) @ Rt.T + tt
    u = pc[:, 0] / pc[:, 2] * fx + cx; v = pc[:, 1] / pc[:, 2] * fy + cy; ur = u - bf / pc[:, 2]
    octave = rng.integers(0, NLEVELS, n)
    sigma = noise * np.float64(np.float32(SCALE)) ** octave
    u = u + rng.normal(0, 1, n) * sigma; v = v + rng.normal(0, 1, n) * sigma; ur = ur + rng.normal(0, 1, n) * sigma
    is_gross = np.zeros(n, bool)
    ng = int(round(share * n))
    if ng:
        g = rng.choice(n, ng, replace=False); is_gross[g] = True
        ang = rng.uniform(0, 2 * np.pi, ng); r = rng.uniform(gross[0], gross[1], ng) * (1.0 + octave[g])
        u[g] += r * np.cos(ang); v[g] += r * np.sin(ang); ur[g] += r * np.cos(ang) * rng.choice([-1.0, 0.5], ng)
    stereo = {"mono": np.zeros(n, bool), "stereo": np.ones(n, bool), "mixed": np.arange(n) % 2 == 0}[mix]      # mixed: the type alternates inside a wave
    ur = np.where(stereo, np.maximum(ur, 0.0), -1.0)
    obs = np.stack([u, v, ur, is2[octave].astype(np.float64), pw[:, 0], pw[:, 1], pw[:, 2]], 1).astype(np.float32)
    dR = _rot(rng.normal(0, perturb[0], 3)); dt = rng.normal(0, perturb[1], 3)
    T0 = np.eye(4); T0[:3, :3] = dR @ Rt; T0[:3, 3] = dR @ tt + dt
    if reframe is not None:
        Rtarget, perturbed = reframe
        R0 = T0[:3, :3].copy(); t0 = T0[:3, 3].copy()
        pc0 = pw.astype(np.float64) @ R0.T + t0
        Rn = (dR if perturbed else np.eye(3)) @ np.asarray(Rtarget, np.float64)
        obs[:, 4:7] = ((pc0 - t0) @ Rn).astype(np.float32)
        T0[:3, :3] = Rn
        T_true[:3, :3] = Rt @ R0.T @ Rn
    for i in behind:
        p = T0[:3, :3] @ obs[i, 4:7].astype(np.float64) + T0[:3, 3]
        p[2] = -p[2]
        obs[i, 4:7] = (T0[:3, :3].T @ (p - T0[:3, 3])).astype(np.float32)
    if inv_sigma2 is not None:
        obs[:, 3] = np.float32(inv_sigma2)
    T0 = T0.astype(np.float32)
    if motion is not None:
        T0 = float_product(motion, T0)
    info = {"T_true": T_true, "octave": octave, "gross": is_gross, "stereo": stereo}
    return CAM.copy(), T0, obs, info


ZERO_CAM = np.array([512.0, 512.0, 320.0, 240.0, 32.0], np.float32)


def zero_residual():
    """40 points whose projections at the identity pose are exact in every format the kernel uses: X and Y multiples of 1/4, Z a power of two, f = 512,
    bf = 32, and u, v, u_right computed from them; every second edge monocular.  Every residual is exactly 0: chi = tempChi = 0, x = 0, the trial equals
    the estimate (through theta < 1e-5 of the exponential map) and every round ends by rho == 0.  There is no seed: the problem is one."""
    i = np.arange(40)
    X = ((2 * i) % 9 - 4) / 4.0; Y = ((5 * i) % 7 - 3) / 4.0; Z = 2.0 ** (1 + i % 3)
    fx, fy, cx, cy, bf = ZERO_CAM.astype(np.float64)
    u = X / Z * fx + cx; v = Y / Z * fy + cy; ur = u - bf / Z
    stereo = i % 2 == 0
    ur = np.where(stereo, ur, -1.0)
    obs64 = np.stack([u, v, ur, np.ones(40), X, Y, Z], 1)
    obs = obs64.astype(np.float32)
    assert np.array_equal(obs.astype(np.float64), obs64) and len(np.unique(obs[:, 4:7], axis=0)) == 40
    info = {"T_true": np.eye(4), "octave": np.zeros(40, int), "gross": np.zeros(40, bool), "stereo": stereo}
    return ZERO_CAM.copy(), np.eye(4, dtype=np.float32), obs, info


def key(n, mix, share):
    return f"n{n}_{mix}_{int(round(share * 100))}"


GRID = [(n, mix, share) for n in SIZES for mix in MIXES for share in SHARES]
# further cases, looked for because the grid need not contain what they show (make_golden_pose_opt_spread.py checks that they do show it):
# a large perturbation of the initial pose (rejected LM trials, rounds that end on one), many gross outliers close to the threshold
EXTRA = {
    "far_start": dict(n=120, mix="mixed", share=0.3, perturb=(0.25, 0.8)),
    "far_start_mono": dict(n=90, mix="mono", share=0.3, perturb=(0.3, 1.0)),
    "near_threshold": dict(n=200, mix="mixed", share=0.4, gross=(1.5, 4.0), perturb=(0.05, 0.2)),
    "noisy": dict(n=150, mix="stereo", share=0.3, noise=1.6, gross=(2.0, 6.0), perturb=(0.1, 0.3)),
}
# sizes around the LDS staging limit (here and not in SIZES, so that the grid keeps its order)
for _n in (STAGE_MAX - 1, STAGE_MAX, STAGE_MAX + 1):
    EXTRA[f"n{_n}_mixed_30"] = dict(n=_n, mix="mixed", share=0.3)

# Initial rotations past 120 degrees: trace(R) <= 0, the second half of Eigen's Quaternion(Matrix3) (largest diagonal entry i, the index permutation, w from an
# off-diagonal difference, w < 0 before normalizeRotation's flip).  The grid's initial rotations are _rot(normal(0, 0.3)): trace > 0 in every one.
#   130 degrees about x, y, z and (1, 2, 3), both signs: |w| = cos 65 = 0.42, so a wrong sign or index moves the pose by order 1; i = 0, 1, 2, 2; the negative
#     angles have w < 0 before the flip;
#   175 degrees about x, y, z with the 0.02 rad perturbation: w = 0.04 +- 0.01 ... the perturbation takes part in w;
#   exactly pi about x, y, z: the float block is diag(1, -1, -1) etc., trace exactly -1, w = +-0;
#   exactly 120 degrees about (1, 1, 1): the cyclic permutation matrix, trace exactly 0 (t > 0.0 is false on equality) and the three diagonal entries tie at 0;
#   110 degrees about y: trace = 1 + 2 cos 110 = 0.32, the control just inside the first half.
TURN_PI = {"x": np.diag([1.0, -1.0, -1.0]), "y": np.diag([-1.0, 1.0, -1.0]), "z": np.diag([-1.0, -1.0, 1.0])}
TURN_CYCLIC = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
TURN_AXES = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0), "123": (1.0, 2.0, 3.0), "111": (1.0, 1.0, 1.0)}
TURN_ANGLES = [(a, s * 130.0) for a in ("x", "y", "z", "123") for s in (1, -1)] + [(a, 175.0) for a in "xyz"] + [(a, 180.0) for a in "xyz"] + [("111", 120.0), ("y", 110.0)]
_TURN = dict(n=120, mix="mixed", share=0.3)
TURNED = []
for _a, _deg in TURN_ANGLES:
    if _deg == 180.0:
        _name, _R, _perturbed = f"turn_{_a}_pi_exact", TURN_PI[_a], False
    elif _a == "111":
        _name, _R, _perturbed = "turn_111_120_exact", TURN_CYCLIC, False
    else:
        _name, _R, _perturbed = f"turn_{_a}_{'m' if _deg < 0 else 'p'}{abs(int(_deg))}", axis_angle(TURN_AXES[_a], _deg), True
    EXTRA[_name] = dict(_TURN, reframe=(_R, _perturbed))
    TURNED.append(_name)

# Degenerate and plausible-but-never-generated inputs:
#   all_outliers_*: an information of 1e30 per pixel^2 flags every edge in round 0 (tests/test_pose_opt_model.py says why), so rounds 1-3 have no level-0 edge,
#     optimize() returns at once, and the result is 0 inliers and the initial pose through toSE3Quat / toCvMat;
#   zero_residual: see zero_residual();
#   behind_camera: n120_mixed_30 with two stereo and two monocular points mirrored to z < 0 in the initial camera frame;
#   float_product_pose: the initial pose is a float product of a small float motion and a float pose: orthonormal only to ~1e-7.
EXTRA["all_outliers_12"] = dict(n=12, mix="mixed", share=0.0, inv_sigma2=1e30)
EXTRA["all_outliers_300"] = dict(n=300, mix="mixed", share=0.0, inv_sigma2=1e30)
EXTRA["zero_residual"] = None
BEHIND = (3, 4, 70, 71)
EXTRA["behind_camera"] = dict(_TURN, behind=BEHIND)
MOTION = np.eye(4, dtype=np.float32)
MOTION[:3, :3] = _rot(np.array([0.01, -0.02, 0.015])).astype(np.float32); MOTION[:3, 3] = (0.02, 0.01, -0.03)
EXTRA["float_product_pose"] = dict(_TURN, motion=MOTION)


def case_args(name):
    if name in EXTRA:
        return dict(EXTRA[name])
    n, mix, share = name.split("_")
    return dict(n=int(n[1:]), mix=mix, share=int(share) / 100.0)


ALL_NAMES = [key(*g) for g in GRID] + list(EXTRA)


def case(name, seed):
    if name == "zero_residual":
        return zero_residual()
    return make(seed=seed, **case_args(name))


def rotation_angle(Ta, Tb):
    """angle of Ra Rb^T and the infinity norm of ta - tb, of two float 4x4 poses"""
    Ta = np.asarray(Ta, np.float64).reshape(4, 4); Tb = np.asarray(Tb, np.float64).reshape(4, 4)
    R = Ta[:3, :3] @ Tb[:3, :3].T
    s = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = 0.5 * (np.trace(R) - 1.0)
    return float(np.arctan2(s, c)), float(np.abs(Ta[:3, 3] - Tb[:3, 3]).max())
