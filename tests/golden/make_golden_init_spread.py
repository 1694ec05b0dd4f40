#!/usr/bin/env python3
"""Records, per graded scene of tests/init_cases.py, how far the choices tests/init_model.py could have made for a null vector lie apart: the unit null
vector of the 16 x 9 (H) and 8 x 9 (F) systems of every set and of the 4 x 4 triangulation systems of the winning motion hypothesis, taken from
numpy.linalg.eigh(A^T A), from numpy.linalg.svd(A) and from the stated cyclic Jacobi on A^T A (all in float64, signs aligned), over the systems whose
second-smallest eigenvalue of A^T A exceeds 1e-10 of the largest.  tests/test_init_model.py allows the model 4 x the recorded value plus one float
ulp per entry against an independent restatement, the margin of the project's earlier spreads (H16, H18).

    python tests/golden/make_golden_init_spread.py          -> tests/golden/init_spread.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import init_cases as Cs                                                         # noqa: E402
import init_model as M                                                          # noqa: E402
from pnp_model import jacobi_batch                                              # noqa: E402

GATE = 1e-10


def spread(A, AtA):
    """the largest distance between the three choices of the unit null vector over the gated systems, and the share of systems the gate leaves out"""
    worst, out = 0.0, 0
    w, V = jacobi_batch(AtA)
    for k in range(len(A)):
        ew, ev = np.linalg.eigh(AtA[k])
        if not ew[1] > GATE * ew[-1]:
            out += 1
            continue
        cand = [ev[:, 0], np.linalg.svd(A[k].astype(np.float64))[2][-1], V[k][:, int(M.smallest(w[k:k + 1])[0])]]
        cand = [v if v @ cand[0] >= 0 else -v for v in cand]
        worst = max(worst, max(np.abs(a - b).max() for a in cand for b in cand))
    return worst, out / max(len(A), 1)


def systems(name):
    """(A, A^T A) of every H set, every F set and the winning motion hypothesis' triangulations of a case"""
    c = Cs.case(name)
    args = Cs.arguments(c)
    _, Ah, AtAh = M.null_vectors(args["matches"], args["sets"], args["norm1"], args["norm2"], False, with_system=True)
    _, Af, AtAf = M.null_vectors(args["matches"], args["sets"], args["norm1"], args["norm2"], True, with_system=True)
    m = M.reconstruct(**args)
    tri = None
    if m["best_mot"] >= 0:
        R, t = m["mot_R"][m["best_mot"]], m["mot_t"][m["best_mot"]]
        mask = m["mask_h"] if m["model"] == 0 else m["mask_f"]
        fx, fy, cx, cy = Cs.K
        P1 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], np.float32)
        with np.errstate(all="ignore"):
            x, A4, AtA4 = M.triangulate(args["matches"][mask], P1, M.projection(Cs.K, R, t, args["gemm_mode"])[0], with_system=True)
        tri = (x, A4, AtA4)
    return (Ah, AtAh), (Af, AtAf), tri


def main():
    out = {}
    for name in Cs.GRADED:
        (Ah, AtAh), (Af, AtAf), tri = systems(name)
        with np.errstate(all="ignore"):
            out[name + "/H"] = np.array(spread(Ah, AtAh))
            out[name + "/F"] = np.array(spread(Af, AtAf))
            out[name + "/T"] = np.array(spread(tri[1], tri[2]) if tri is not None else (0.0, 0.0))
        print(name, "H", out[name + "/H"], "F", out[name + "/F"], "triangulation", out[name + "/T"])
    np.savez_compressed(os.path.join(HERE, "init_spread.npz"), **out)


if __name__ == "__main__":
    main()
