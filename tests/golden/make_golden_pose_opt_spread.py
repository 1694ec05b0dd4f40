"""Writes tests/golden/pose_opt_spread.npz: for every case of tests/pose_opt_cases.py the seed it uses, the model's pose under the identity order of the
sums over edges, and the largest deviation of the pose over 16 seeded permutations of that order (a rotation angle and a translation infinity norm,
both taken after rounding to float).  The kernel tests allow the device 4 x that spread.

A seed is kept for a case only if
  * the flags and the return value are identical under all 16 permutations, and
  * every edge's final chi2 is farther than 1e-6 (relative) from its threshold - more than 10 float ulps, the granularity of the reference's comparison;
the first such seed is taken.  The kept set must still contain a rejected LM trial, a round that ends on a rejected trial, a Terminate by the
three-strikes criterion and a round-0 outlier that ends as an inlier.

The turned cases (initial rotations past 120 degrees) must, from the model alone, take the largest diagonal entry i = 0, i = 1 and i = 2 of
Quaternion(Matrix3)'s trace <= 0 half, w < 0 before normalizeRotation's flip at least once for each i, and the two exact traces (-1 and 0).  The degenerate
cases must show what they are for (preconditions(): every edge flagged in round 0; four rounds ended by rho == 0 without an accepted step; finite chi2 and
the mirrored edges flagged; an orthonormality defect above 5e-8).  Every key of the committed file must come out byte for byte as it is.
If any condition fails nothing is written.

    python tests/golden/make_golden_pose_opt_spread.py          (CPU only, a few minutes)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pose_opt_cases as Cs          # noqa: E402
import pose_opt_model as M           # noqa: E402

NPERM, MARGIN, MAX_SEED = 16, 1e-6, 40


def margins(chi2, stereo):
    th = np.where(stereo, 7.815, 5.991)
    with np.errstate(all="ignore"):
        return np.abs(chi2 - th) / th


def try_seed(name, seed):
    cam, T0, obs, info = Cs.case(name, seed)
    T, flags, ninl, tr = M.pose_optimization(cam, T0, obs, want_trace=True)
    if len(obs) >= 3 and not (margins(tr["chi2"], info["stereo"]) > MARGIN).all():
        return None
    rot = tr_ = 0.0
    rng = np.random.default_rng([sum(map(ord, name)), seed])
    for _ in range(NPERM):
        Tp, fp, np_ = M.pose_optimization(cam, T0, obs, perm=rng.permutation(len(obs)))
        if not np.array_equal(fp, flags) or np_ != ninl:
            return None
        a, d = Cs.rotation_angle(Tp, T)
        rot, tr_ = max(rot, a), max(tr_, d)
    f = tr["flags"]
    shows = {"rejected": tr["rejected"] > 0, "round_ends_rejected": tr["round_ends_rejected"] > 0, "three_strikes": tr["three_strikes"] > 0,
             "outlier_recovered": bool(len(f) > 1 and (f[0] & ~f[-1]).any())}
    return T, rot, tr_, shows


def quaternion_branch(T0):
    """what Quaternion(Matrix3) does with the float rotation block of T0, read from the model: (trace, i or None, w < 0 before the flip)"""
    m = np.asarray(T0, np.float32)[:3, :3].astype(np.float64)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = M.quat_of_matrix(m)
    if t > 0.0:
        return t, None, bool(q[3] < 0)
    i = int(np.argmax(np.abs(q[:3]) == np.abs(q[:3]).max()))                    # the entry the branch sets to 0.5 sqrt(.) is the largest of x, y, z ...
    d = [m[0, 0], m[1, 1], m[2, 2]]
    assert d[i] == max(d) and q[i] > 0                                          # ... it belongs to the largest diagonal entry, and is positive
    return t, i, bool(q[3] < 0) or bool(np.signbit(q[3]))


def preconditions(name, seed):
    """what a degenerate case must show to be the case it is named for, from the model's trace: None, or what is wrong"""
    cam, T0, obs, info = Cs.case(name, seed)
    T, flags, ninl, tr = M.pose_optimization(cam, T0, obs, want_trace=True)
    init = M.to_cvmat(M.to_se3quat(T0))
    if name.startswith("all_outliers"):
        if not tr["flags"][0].all():
            return "round 0 leaves a level-0 edge"
        if ninl != 0 or not flags.all() or T.tobytes() != init.tobytes() or len(tr["flags"]) != 4:
            return "not 0 inliers at the initial pose"
    if name == "zero_residual":
        if tr["accepted"] != 0 or tr["terminate_trials"] != 4 or tr["rejected"] != 4 or tr["three_strikes"] != 0:
            return f"not four rounds ended by rho == 0 without an accepted step: {tr['accepted']} {tr['rejected']} {tr['terminate_trials']}"
        if flags.any() or ninl != len(obs) or T.tobytes() != T0.tobytes() or (tr["chi2"] != 0.0).any():
            return "not all inliers at the unchanged pose with chi2 = 0"
    if name == "behind_camera":
        P = M.Problem(cam, obs)
        _, chi2, _, _, z = M.errors(P, M.to_se3quat(T0))
        if not ((z[list(Cs.BEHIND)] < -1.0).all() and (np.delete(z, Cs.BEHIND) > 1.0).all() and info["stereo"][list(Cs.BEHIND)].sum() == 2):
            return "not two stereo and two monocular points behind the camera at the initial pose"
        if not (np.isfinite(tr["chi2"]).all() and np.isfinite(chi2).all() and np.isfinite(T).all()):
            return "a non-finite chi2 or pose"
        if not all(f[list(Cs.BEHIND)].all() for f in tr["flags"]):
            return "a mirrored edge is not flagged"
    if name == "float_product_pose":
        R = T0[:3, :3].astype(np.float64)
        defect = np.abs(R @ R.T - np.eye(3)).max()
        print(f"    orthonormality defect of the initial rotation block {defect:.3e}")
        if not defect > 5e-8:
            return "the product is orthonormal to float rounding"
    return None


def main():
    out, seen = {}, {}
    turned = {}
    for name in Cs.ALL_NAMES:
        for seed in range(MAX_SEED):
            r = try_seed(name, seed)
            if r is not None:
                break
        else:
            print(f"{name}: no seed below {MAX_SEED} meets the conditions - nothing written")
            return 1
        T, rot, tr_, shows = r
        why = preconditions(name, seed) if name in ("all_outliers_12", "all_outliers_300", "zero_residual", "behind_camera", "float_product_pose") else None
        if why:
            print(f"{name}: seed {seed}: {why} - nothing written")
            return 1
        if name in Cs.TURNED:
            turned[name] = quaternion_branch(Cs.case(name, seed)[1])
            print(f"    trace {turned[name][0]:+.4f}, i = {turned[name][1]}, w < 0 before the flip: {turned[name][2]}")
        out[name + "/seed"] = np.int32(seed); out[name + "/pose"] = T; out[name + "/spread"] = np.array([rot, tr_])
        for k, v in shows.items():
            seen[k] = seen.get(k, 0) + int(v)
        print(f"{name}: seed {seed}, spread {rot:.3e} rad {tr_:.3e}, {[k for k, v in shows.items() if v]}", flush=True)
    missing = [k for k in ("rejected", "round_ends_rejected", "three_strikes", "outlier_recovered") if not seen.get(k)]
    if missing:
        print(f"the kept set shows no {missing} - nothing written")
        return 1
    got = set(turned.values())
    wrong = [f"no case takes i = {i}" for i in range(3) if not any(b[1] == i for b in got)]
    wrong += [f"no case with i = {i} has w < 0 before the flip" for i in range(3) if not any(b[1] == i and b[2] for b in got)]
    wrong += [f"no case has trace exactly {t}" for t in (-1.0, 0.0) if not any(b[0] == t and b[1] is not None for b in got)]
    if turned["turn_y_p110"][1] is not None:
        wrong.append("the 110 degree control is not in the trace > 0 half")
    if wrong:
        print(f"the turned cases: {wrong} - nothing written")
        return 1
    path = os.path.join(HERE, "pose_opt_spread.npz")
    if os.path.exists(path):                                                    # every key the committed file has comes out as it is, byte for byte
        old = dict(np.load(path))
        changed = [k for k, v in old.items() if k not in out or np.asarray(out[k]).dtype != v.dtype or np.asarray(out[k]).shape != v.shape or np.asarray(out[k]).tobytes() != v.tobytes()]
        if changed:
            print(f"{len(changed)} keys of the committed file would change ({changed[:6]}) - nothing written")
            return 1
        print(f"all {len(old)} keys of the committed file are unchanged; {len(out) - len(old)} new")
    np.savez_compressed(path, **out)
    print("kept", len(Cs.ALL_NAMES), "cases;", seen)
    return 0


if __name__ == "__main__":
    sys.exit(main())
