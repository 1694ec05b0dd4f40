"""Writes tests/golden/pose_opt_spread.npz: for every case of tests/pose_opt_cases.py the seed it uses, the model's pose under the identity order of the
sums over edges, and the largest deviation of the pose over 16 seeded permutations of that order (a rotation angle and a translation infinity norm,
both taken after rounding to float).  The kernel tests allow the device 4 x that spread.

A seed is kept for a case only if
  * the flags and the return value are identical under all 16 permutations, and
  * every edge's final chi2 is farther than 1e-6 (relative) from its threshold - more than 10 float ulps, the granularity of the reference's comparison;
the first such seed is taken.  The kept set must still contain a rejected LM trial, a round that ends on a rejected trial, a Terminate by the
three-strikes criterion and a round-0 outlier that ends as an inlier.  If any condition fails nothing is written.

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


def main():
    out, seen = {}, {}
    for name in Cs.ALL_NAMES:
        for seed in range(MAX_SEED):
            r = try_seed(name, seed)
            if r is not None:
                break
        else:
            print(f"{name}: no seed below {MAX_SEED} meets the conditions - nothing written")
            return 1
        T, rot, tr_, shows = r
        out[name + "/seed"] = np.int32(seed); out[name + "/pose"] = T; out[name + "/spread"] = np.array([rot, tr_])
        for k, v in shows.items():
            seen[k] = seen.get(k, 0) + int(v)
        print(f"{name}: seed {seed}, spread {rot:.3e} rad {tr_:.3e}, {[k for k, v in shows.items() if v]}", flush=True)
    missing = [k for k in ("rejected", "round_ends_rejected", "three_strikes", "outlier_recovered") if not seen.get(k)]
    if missing:
        print(f"the kept set shows no {missing} - nothing written")
        return 1
    np.savez_compressed(os.path.join(HERE, "pose_opt_spread.npz"), **out)
    print("kept", len(Cs.ALL_NAMES), "cases;", seen)
    return 0


if __name__ == "__main__":
    sys.exit(main())
