"""tests/sim3_opt_model.py pinned without a device and without g2o (the model is a restatement by reading, NOT pinned against the reference, which cannot
be built where this project is developed: g2o needs Eigen): its numerical Jacobians against the closed-form derivative of its own error, recovery of a
known Sim3, a small gradient at the result, the fixed scale, the early return, the unnormalised quaternion, and that the named cases of
tests/sim3_opt_cases.py show what they are there for."""
import math
import os
import sys

import numpy as np
import pytest

import sim3_opt_cases as Cs
import sim3_opt_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("fix", [False, True])
def test_numerical_jacobians_equal_the_closed_form(fix):
    """Central differences with a step of 1e-9 of an error whose values are pixels up to ~1000.  The truncation error (step^2 times a third derivative)
    is below 1e-14 and plays no part.  What limits the agreement is rounding: an error value is the end of about ten roundings of quantities up to
    P = max(|u|, |v|, f |x / z| + c) pixels, so it is off by up to 10 ulp(P) / 2; a difference of two by twice that; times scalar = 5e8.
    With P < 1024 that is 10 * 1.14e-13 * 5e8 = 5.7e-4 pixels per unit of the update, against entries of tens to hundreds.
    (Measured: 1.1e-4 with the scale free, 1.3e-4 with it fixed.)"""
    cams, S12, pairs, th2, _, info = Cs.make(300, 0.0, fix, 3, scale=1.7)
    P = M.Problem(cams, pairs, th2, fix)
    S = M.to_sim3(S12)
    assert max(np.abs(pairs[:, [0, 1, 3, 4]]).max(), 1.0) < 1024
    N12, N21 = M.numeric_jacobians(P, S)
    A12, A21 = M.analytic_jacobians(P, S)
    worst = max(np.abs(N12 - A12).max(), np.abs(N21 - A21).max())
    bound = 10 * np.spacing(1023.0) * M.SCALAR
    print(f"largest |numerical - closed form| {worst:.3e}, bound {bound:.3e}, largest entry {max(np.abs(A12).max(), np.abs(A21).max()):.1f}")
    assert worst <= bound
    assert np.abs(A12).max() > 500 and np.abs(A21).max() > 500 and min(np.abs(A12[:, :, :6]).max((0, 1)).min(), np.abs(A21[:, :, :6]).max((0, 1)).min()) > 30
    if fix:
        assert (N12[:, :, 6] == 0.0).all() and (N21[:, :, 6] == 0.0).all()      # exactly 0: both perturbations are the estimate itself
    else:
        # (a scaling about camera 1's centre does not move a projection into camera 1: the forward edge's column 6 is rounding noise; the scale is seen by the inverse edges alone)
        assert np.abs(N12[:, :, 6]).max() <= bound and np.abs(A12[:, :, 6]).max() < 1e-9 and np.abs(N21[:, :, 6]).max() > 50
    # a forward difference would be off by the second derivative times the step, far below the rounding floor too - but a ONE-SIDED quotient with scalar
    # 1 / (2 delta) is half the derivative, and a wrong sign of inverse() flips J21: both are orders of magnitude outside the bound
    assert np.abs(0.5 * A12 - A12).max() > 100 * bound and np.abs(-A21 - A21).max() > 100 * bound


@pytest.mark.parametrize("scale", Cs.SCALES)
def test_exact_observations_recover_the_sim3(scale):
    """no pixel noise, no outliers: what is left is the float rounding of the points and of the key points (2^-15 pixels at 300), so the true S12 is
    recovered to about 1e-7; every pair stays and the second phase is optimize(5)"""
    cams, S12, pairs, th2, fix, info = Cs.make(80, 0.0, False, 2, scale=scale, noise=0.0)
    S, removed, nin, tr = M.optimize_sim3(cams, S12, pairs, th2, fix, want_trace=True)
    Rt, tt, sc = info["S_true"]
    true = np.array(list(M.quat_of_matrix([[float(Rt[i, j]) for j in range(3)] for i in range(3)])) + list(tt) + [sc])
    d0, d = Cs.deviation(S12, true), Cs.deviation(S, true)
    print(f"start {d0}, result {d}")
    assert d0[0] > 1e-2 and d0[1] > 1e-2 and d[0] < 2e-6 and d[1] < 2e-5 and d[2] < 5e-6 * scale
    assert nin == 80 and not removed.any() and tr["second_iterations"] == 5 and not tr["early"]


def test_gradient_vanishes_at_the_result():
    """Both phases minimise sum rho(chi2) over the live pairs' edges; b is minus half the gradient of that cost (the Huber weights are part of it).  The
    stop criteria leave a Gauss-Newton step whose predicted decrease b^T H^-1 b is below what they test for, a thousandth of chi; at the start it is
    most of what can be gained.  (Measured: 1.7e-12 of chi = 604 at the result; 6.8e3 of 1.1e4 at the start.)"""
    cams, S12, pairs, th2, fix, info = Cs.make(200, 0.3, False, 4, scale=0.6)
    S, removed, nin, tr = M.optimize_sim3(cams, S12, pairs, th2, fix, want_trace=True)
    P = M.Problem(cams, pairs, th2, fix)
    live = tr["chi2"][1][2]

    def left(est):
        H, b, chi = M.evaluate(P, est, live)
        ok, x = M.solve(H, b, 0.0, [0.0] * 7)
        assert ok
        return float(np.dot(b, x)), chi, np.abs(x).max()
    dec, chi, x = left(M.to_sim3(S))
    dec0, chi0, x0 = left(M.to_sim3(S12))
    print(f"predicted decrease at the result {dec:.3e} of chi {chi:.3e} (step {x:.3e}); at the start {dec0:.3e} of {chi0:.3e} (step {x0:.3e})")
    assert not tr["early"] and tr["second_iterations"] == 10
    assert 0 <= dec <= 1e-3 * chi and dec0 > 1e3 * dec and dec0 > 0.5 * (chi0 - chi)
    assert x < 1e-5 < x0


def test_fixed_scale_keeps_the_bits_of_the_scale():
    cams, S12, pairs, th2, fix, info = Cs.make(100, 0.3, True, 1, scale=1.7)
    S12 = S12.copy(); S12[7] = 1.7000000000000002                                   # (not a float: every bit of the double must survive)
    S, removed, nin, tr = M.optimize_sim3(cams, S12, pairs, th2, True, want_trace=True)
    assert not tr["early"] and tr["accepted"] >= 5 and S[7].tobytes() == S12[7].tobytes() and S[:7].tobytes() != S12[:7].tobytes()
    H, b, chi = M.evaluate(M.Problem(cams, pairs, th2, True), M.to_sim3(S12), np.ones(100, bool))
    assert all(H[M._IDX.index((j, 6))] == 0.0 for j in range(7)) and b[6] == 0.0     # column 6 is exactly 0: H66 is lambda alone
    # ... under the jitter too: exp(0) is 1 in every library
    Sj = M.optimize_sim3(cams, S12, pairs, th2, True, jitter=7)[0]
    assert Sj[7].tobytes() == S12[7].tobytes()
    # with the scale free the same problem moves it
    assert M.optimize_sim3(cams, S12, pairs, th2, False)[0][7] != S12[7]


@pytest.mark.parametrize("n", [0, 1, 9, 10])
def test_early_return(n):
    """fewer than 10 pairs left after the first check: 0, g2oS12 untouched, the first check's flags; 1 <= n < 10 still runs optimize(5) and the check"""
    cams, S12, pairs, th2, fix, info = Cs.make(40, 0.0, False, 6)
    pairs = pairs[:n].copy()
    if n:
        pairs[0, 0] += 200.0                                                        # one gross outlier: removed by the first check
    S, removed, nin, tr = M.optimize_sim3(cams, S12, pairs, th2, fix, want_trace=True)
    assert nin == 0 and S.tobytes() == S12.tobytes() and len(removed) == n
    if n == 0:
        assert tr["iterations"] == []
        return
    assert tr["early"] and tr["iterations"][0] >= 1 and len(tr["iterations"]) == 1 and removed.sum() == tr["n_bad"]
    assert removed[0] == (n > 1)                                                   # (one pair alone is fitted exactly by seven parameters, outlier or not)
    assert tr["estimate"] is not None and M.to_array(tr["estimate"]).tobytes() != S12.tobytes()        # the estimate moved; the member does not hand it back
    # with 11 pairs and the same outlier 10 are left: the second phase runs and S12 is written
    cams, S12, pairs, th2, fix, info = Cs.make(40, 0.0, False, 6)
    pairs = pairs[:11].copy(); pairs[0, 0] += 200.0
    S, removed, nin, tr = M.optimize_sim3(cams, S12, pairs, th2, fix, want_trace=True)
    assert not tr["early"] and tr["second_iterations"] == 10 and nin == 10 and removed.tolist() == [1] + [0] * 10 and S.tobytes() != S12.tobytes()


@pytest.mark.parametrize("defect", [1e-7, -1e-7, 1e-3])
def test_unnormalised_quaternion_is_carried_through(defect):
    """Sim3's constructors and operator* never normalise: |q| of the result is |q| of the input times the |q| of the updates' quaternions (1 to rounding).
    Eigen's q * v (v + 2 w (u x v) + 2 u x (u x v)) is a rotation only for a unit q, and inverse() uses the conjugate, not the inverse quaternion: a defect
    of the norm changes what both edges compute, and the result differs from the one a normalised input gives."""
    cams, S12, pairs, th2, fix, info = Cs.make(100, 0.0, False, 8, noise=0.2)
    S_unit = M.optimize_sim3(cams, S12, pairs, th2, fix)[0]
    Sq = S12.copy(); Sq[:4] *= 1.0 + defect
    S = M.optimize_sim3(cams, Sq, pairs, th2, fix)[0]
    norm = math.sqrt(float((S[:4] ** 2).sum())); norm_unit = math.sqrt(float((S_unit[:4] ** 2).sum()))
    print(f"|q| - 1: {norm - 1.0:+.3e} (input {defect:+.1e}), from a unit input {norm_unit - 1.0:+.3e}; s {S[7]:.9f} against {S_unit[7]:.9f}")
    # (the case's own quaternion comes from a FLOAT matrix: its norm is 1 to about 1e-8, and that defect is carried through just the same)
    assert abs(norm_unit - 1.0) < 1e-7 and abs((norm / norm_unit - 1.0) - defect) < 1e-3 * abs(defect) + 1e-12
    assert abs(S[7] - S_unit[7]) > 1e-9 and abs(S[7] - S_unit[7]) < 10 * abs(defect)


def test_inverse_and_product():
    """inverse() is built from the conjugate: for a unit quaternion S * S^-1 maps every point to itself; for |q| != 1 it does not (conj(q) is not q^-1),
    and the model keeps that"""
    S12 = Cs.make(10, 0.0, False, 0, scale=1.7)[1]
    S12[:4] /= np.sqrt((S12[:4] ** 2).sum())
    S = M.to_sim3(S12)
    X = np.array([0.3, -1.2, 4.0])
    back = M.smap(M.mul(S, M.inverse(S)), *X)
    assert np.abs(np.array(back) - X).max() < 1e-14
    y = np.array(M.smap(M.inverse(S), *M.smap(S, *X)))
    assert np.abs(y - X).max() < 1e-14
    Sq = (tuple(1.001 * v for v in S[0]), S[1], S[2])
    y = np.array(M.smap(M.inverse(Sq), *M.smap(Sq, *X)))
    assert 1e-3 < np.abs(y - X).max() < 1e-1


def test_named_cases_show_what_they_are_for():
    """the committed seeds still make every named case the case it is named for (the generator's own check, on the committed file)"""
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden_sim3_opt_spread as G
    finally:
        sys.path.remove(GOLDEN)
    g = dict(np.load(os.path.join(GOLDEN, "sim3_opt_spread.npz")))
    assert sorted({k.split("/")[0] for k in g}) == sorted(Cs.ALL_NAMES)
    for name in Cs.EXTRA:
        seed = int(g[name + "/seed"])
        cams, S12, pairs, th2, fix, info = Cs.case(name, seed)
        S, removed, nin, tr = M.optimize_sim3(cams, S12, pairs, th2, fix, want_trace=True)
        assert S.tobytes() == g[name + "/S12"].tobytes(), name
        assert G.shows(name, seed, S, removed, nin, tr) is None, name
    spreads = np.array([g[n + "/spread"] for n in Cs.ALL_NAMES])
    print("largest recorded spread", spreads.max(0))
    assert spreads.max(0)[0] > 1e-8                                                  # orders of magnitude above pose optimisation's 1e-9 rad: the 5e8 amplification
