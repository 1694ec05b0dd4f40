#!/usr/bin/env python3
"""Records, per scene of tests/pnp_cases.py's SPREAD_SCENES (EPnP over all inliers, n >= 6: the null space of M^T M is one-dimensional and the answer is
well defined), the largest deviation of tests/pnp_model.py's R and t from an independent plain-numpy EPnP (pnp_cases.independent_epnp: eigh, lstsq,
inv, svd), and on the noise-free scenes the independent EPnP's own error against the true pose.  tests/test_pnp_model.py allows the model 4 x the
recorded value plus one float ulp, the margin of tests/sim3_checks.py: the two differ by rounding and by which of several equivalent decompositions
they take, which the recorded spread samples; 4 x keeps false alarms rare.

    python tests/golden/make_golden_pnp_spread.py          -> tests/golden/pnp_spread.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pnp_cases as Cs                                                          # noqa: E402
import pnp_model as M                                                           # noqa: E402


def main():
    out = {}
    for name, n, seed, noise, planar in Cs.SPREAD_SCENES:
        corr, Rcw, tcw, _ = Cs.scene(n, seed, 0.0, noise, planar)
        R, t = M.epnp(corr, Cs.K, mask=np.ones(n, bool))
        Ri, ti = Cs.independent_epnp(corr, Cs.K)
        out[name + "/model_R"], out[name + "/model_t"] = R, t
        out[name + "/spread"] = np.array([np.abs(R - Ri).max(), np.abs(t - ti).max() / np.abs(ti).max()])
        out[name + "/truth"] = np.array([np.abs(Ri - Rcw).max(), np.abs(ti - tcw).max() / np.abs(tcw).max()])
        print(name, "spread", out[name + "/spread"], "independent against the true pose", out[name + "/truth"])
    np.savez_compressed(os.path.join(HERE, "pnp_spread.npz"), **out)


if __name__ == "__main__":
    main()
