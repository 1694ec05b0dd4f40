"""Writes tests/golden/sim3_spread.npz: for every graded case of tests/sim3_cases.py the seed it uses, the model's per-hypothesis R, t, s under the stated
arithmetic, and the largest deviation from them among the model's variants - the eigenvector from numpy.linalg.eigh instead of the
stated Jacobi, and atan2, sin and cos each moved one double ulp up and down: spread[0] the largest |dR_ij|, spread[1] the largest |dt_i| / max|t|,
spread[2] the largest |ds| / |s|, each over all hypotheses of the case and taken after rounding to float.  The kernel tests allow the device 4 x that
spread plus one float ulp per entry (tests/sim3_checks.py).

Triples are gated by the eigenvalue gap (tests/sim3_cases.py); the script asserts that fewer than 5 % of all draws were rejected and that every graded
hypothesis is finite.  If a condition fails nothing is written.

    python tests/golden/make_golden_sim3_spread.py          (CPU only, under a minute)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sim3_cases as Cs          # noqa: E402
import sim3_model as M           # noqa: E402

VARIANTS = [dict(eig="eigh")] + [dict(nudge=tuple(d if k == i else 0 for k in range(3))) for i in range(3) for d in (1, -1)]


def main():
    out = {}
    for name in Cs.ALL_NAMES:
        seed = 0
        corr, tri, fix, mode, _ = Cs.case(name, seed)
        base = [M.horn(corr[t, 0:3].T, corr[t, 3:6].T, fix, mode) for t in tri]
        if not all(np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s) for R, t, s in base):
            print(f"{name}: a graded hypothesis is not finite - nothing written")
            return 1
        spread = np.zeros(3)
        for v in VARIANTS:
            for (R, t, s), tr in zip(base, tri):
                Rv, tv, sv = M.horn(corr[tr, 0:3].T, corr[tr, 3:6].T, fix, mode, **v)
                spread[0] = max(spread[0], np.abs(Rv.astype(float) - R).max())
                spread[1] = max(spread[1], np.abs(tv.astype(float) - t).max() / np.abs(t).max())
                spread[2] = max(spread[2], abs(float(sv) - float(s)) / abs(float(s)))
        out[name + "/seed"] = np.int32(seed); out[name + "/spread"] = spread
        out[name + "/R"] = np.array([b[0] for b in base], np.float32); out[name + "/t"] = np.array([b[1] for b in base], np.float32)
        out[name + "/s"] = np.array([b[2] for b in base], np.float32)
        print(f"{name}: {len(tri)} hypotheses, spread R {spread[0]:.3e}  t {spread[1]:.3e}  s {spread[2]:.3e}", flush=True)
    if not Cs.rejected_share() < 0.05:
        print(f"{Cs.TALLY[1]} of {Cs.TALLY[0]} draws rejected by the eigenvalue gap - nothing written")
        return 1
    np.savez_compressed(os.path.join(HERE, "sim3_spread.npz"), **out)
    print("kept", len(Cs.ALL_NAMES), "cases;", Cs.TALLY[1], "of", Cs.TALLY[0], "draws rejected")
    return 0


if __name__ == "__main__":
    sys.exit(main())
