"""Seeded problems for the pose-optimisation tests: a camera, a true pose, points in front of it, pixel noise scaled by the level's sigma, gross outliers and
a perturbed initial pose.  case(n, mix, share, seed) is a pure function of its arguments; tests/golden/pose_opt_spread.npz records which seed each
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


def make(n, mix, share, seed, noise=1.0, perturb=(0.02, 0.05), gross=(15.0, 80.0), depth=(2.0, 20.0)):
    """(cam, Tcw_init float32 4x4, obs float32 [n, 7], info): info has the true pose, the octaves and which observations are gross outliers"""
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
    info = {"T_true": T_true, "octave": octave, "gross": is_gross, "stereo": stereo}
    return CAM.copy(), T0.astype(np.float32), obs, info


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


def case_args(name):
    if name in EXTRA:
        return dict(EXTRA[name])
    n, mix, share = name.split("_")
    return dict(n=int(n[1:]), mix=mix, share=int(share) / 100.0)


ALL_NAMES = [key(*g) for g in GRID] + list(EXTRA)


def case(name, seed):
    return make(seed=seed, **case_args(name))


def rotation_angle(Ta, Tb):
    """angle of Ra Rb^T and the infinity norm of ta - tb, of two float 4x4 poses"""
    Ta = np.asarray(Ta, np.float64).reshape(4, 4); Tb = np.asarray(Tb, np.float64).reshape(4, 4)
    R = Ta[:3, :3] @ Tb[:3, :3].T
    s = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = 0.5 * (np.trace(R) - 1.0)
    return float(np.arctan2(s, c)), float(np.abs(Ta[:3, 3] - Tb[:3, 3]).max())
