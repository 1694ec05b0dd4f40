"""tests/pose_opt_model.py, the numpy restatement of Optimizer::PoseOptimization, pinned by what can be checked without g2o (the reference cannot be built
where this project is developed: g2o needs Eigen): its Jacobians against central differences of its own error, recovery of a known pose, a small gradient
at the result, the short-case rules, and the rule that a level-0 edge is classified by the error the round's last evaluation left."""
import numpy as np
import pytest

import pose_opt_cases as Cs
import pose_opt_model as M


def _camera_points(P, pose):
    _, _, x, y, z = M.errors(P, pose)
    return x, y, z


@pytest.mark.parametrize("mix", ["mono", "stereo"])
def test_analytic_jacobians_equal_central_differences(mix):
    """d e / d delta of e(exp(delta) T) at delta = 0, delta = (omega, upsilon), by central differences with step h = 1e-5 on the smooth error (the
    stereo edge's float 1/z kept in double: the analytic Jacobian is that function's).  Bound on an entry: truncation h^2 / 6 * M3 plus rounding
    8 eps F / h, with M3 <= 1e5 px the third derivatives of a projection with f = 521, |x/z|, |y/z| <= 0.7, z >= 2 m, bf = 40 (each derivative in
    delta costs at most a factor (1 + r^2) <= 2 or 1/z <= 0.5 on f (x/z): 6 * 521 * 2^3 ~ 2.5e4, four times that allowed), and F <= 2e3 px the
    largest intermediate: 1e-10 / 6 * 1e5 + 8 * 2.2e-16 * 2e3 / 1e-5 = 2.1e-6 px per unit of delta, on entries of up to ~1e3."""
    cam, T0, obs, info = Cs.make(200, mix, 0.0, 3)
    P = M.Problem(cam, obs)
    pose = M.to_se3quat(T0)
    x, y, z = _camera_points(P, pose)
    assert z.min() > 1.5 and np.abs(x / z).max() < 0.8 and np.abs(y / z).max() < 0.8
    A = M.jacobians(P, x, y, z)
    h, bound = 1e-5, 1e-10 / 6 * 1e5 + 8 * 2.2e-16 * 2e3 / 1e-5
    rows = 3 if mix == "stereo" else 2
    worst = 0.0
    for j in range(6):
        d = np.zeros(6); d[j] = h
        ep, *_ = M.errors(P, M.oplus(d, pose), float_invz=False)
        em, *_ = M.errors(P, M.oplus(-d, pose), float_invz=False)
        num = (ep - em) / (2 * h)
        worst = max(worst, np.abs(num[:, :rows] - A[:, :rows, j]).max())
    print(f"{mix}: largest |analytic - central difference| {worst:.3e}, bound {bound:.3e}, largest entry {np.abs(A[:, :rows]).max():.3e}")
    assert worst <= bound
    assert np.abs(A[:, :rows]).max() > 100                                      # (the bound is far below the entries it checks)
    if mix == "stereo":                                                        # ... and the reference's float 1/z moves the error by no more than its rounding
        e32, *_ = M.errors(P, pose); e64, *_ = M.errors(P, pose, float_invz=False)
        fx, fy, cx, cy, bf = P.cam
        q = 2.0 ** -24 / z
        assert (np.abs(e32[:, 0] - e64[:, 0]) <= q * np.abs(x) * fx * 1.0001).all() and (np.abs(e32[:, 2] - e64[:, 2]) <= q * (np.abs(x) * fx + bf) * 1.0001).all()
        assert (e32 != e64).any()


@pytest.mark.parametrize("mix", Cs.MIXES)
def test_noise_free_data_recovers_the_pose_and_flags_every_gross_outlier(mix):
    cam, T0, obs, info = Cs.make(300, mix, 0.3, 4, noise=0.0)
    T, flags, ninl = M.pose_optimization(cam, T0, obs)
    ang, dt = Cs.rotation_angle(T, info["T_true"])
    a0, d0 = Cs.rotation_angle(T0, info["T_true"])
    print(f"{mix}: start {a0:.3e} rad {d0:.3e} m, result {ang:.3e} rad {dt:.3e} m")
    # what is left is the float rounding of the points (2^-24 of up to 20 m: ~1e-6 m, ~1e-4 px at 2 m or 2e-7 rad for ONE point; 210 inliers average it
    # down by ~sqrt(210)) and of the returned pose's entries (6e-8).  Asserted: 2e-7 rad and 1e-6 m; measured 0.8-1.4e-8 rad and 0.3-1e-7 m
    assert a0 > 1e-3 and ang < 2e-7 and dt < 1e-6
    assert np.array_equal(flags, info["gross"]) and ninl == 300 - info["gross"].sum()


def test_gradient_of_the_last_round_vanishes_at_the_result():
    """The last round minimises sum chi2 over its level-0 edges without a kernel.  Its stop criteria leave a step whose predicted decrease b^T H^-1 b
    is below what they test for: three iterations running with a decrease under chi / 1000.  So at the result b^T H^-1 b <= chi / 1000, against a
    predicted decrease of most of chi at the start; and the Gauss-Newton step left is far inside the pose's float rounding."""
    cam, T0, obs, info = Cs.make(300, "mixed", 0.3, 5)
    T, flags, ninl, tr = M.pose_optimization(cam, T0, obs, want_trace=True)
    P = M.Problem(cam, obs)
    active = ~tr["flags"][2]

    def left(pose):
        H, b, chi = M.evaluate(P, pose, active, False)
        ok, x = M.solve(H, b, 0.0, np.zeros(6))
        return float(b @ x), float(chi), x
    dec, chi, x = left(tr["pose"])
    dec0, chi0, x0 = left(M.to_se3quat(T0))
    print(f"predicted decrease at the result {dec:.3e} of chi {chi:.3e} (step {np.abs(x).max():.3e}); at the start {dec0:.3e} of {chi0:.3e} (step {np.abs(x0).max():.3e})")
    assert 0 <= dec <= 1e-3 * chi and dec0 > 0.5 * chi0                        # the bound the stop criterion gives (measured: 2.3e-13 of chi = 430)
    # ... and since LM converges quadratically near the minimum the step left is in fact at rounding level: below the float rounding of the returned
    # translation (6e-8 of ~1 m) and rotation entries (measured 1e-9)
    assert np.abs(x).max() < 6e-8


@pytest.mark.parametrize("n", [0, 2, 3, 9, 10])
def test_short_cases(n):
    cam, T0, obs, info = Cs.make(max(n, 1), "mixed", 0.3, 2)
    obs = obs[:n]
    T, flags, ninl, tr = M.pose_optimization(cam, T0, obs, want_trace=True)
    if n < 3:                                                                  # fewer than 3 correspondences: 0, the pose untouched, no flag set
        assert ninl == 0 and T.tobytes() == T0.tobytes() and len(flags) == n and not flags.any() and tr["flags"] == []
        return
    assert len(tr["flags"]) == (1 if n < 10 else 4)                            # fewer than 10 edges: the first round only
    assert ninl == n - flags.sum() and T.tobytes() != T0.tobytes()
    assert np.array_equal(flags, tr["flags"][-1])


def test_round_without_a_level_0_edge_returns_at_once():
    cam, T0, obs, info = Cs.make(12, "mixed", 0.0, 2)
    P = M.Problem(cam, obs)
    init = M.to_se3quat(T0)
    trace = {"accepted": 0, "rejected": 0, "terminate_trials": 0, "three_strikes": 0}
    cur, last = M.optimize(P, init, np.zeros(12, bool), True, None, trace)
    assert cur is init and last is init and trace["accepted"] == trace["rejected"] == 0
    # an information of 1e30 per pixel^2: an inlier would need its residual below sqrt(5.991e-30) = 2.4e-15 px, under the rounding of a projection of
    # hundreds of pixels (1e-13 px) - and the noise is a pixel.  Every edge is an outlier after round 0 whatever pose the round reaches (Huber fits pass
    # through some observations to many digits, so a merely large information would not do); rounds 1-3 have nothing to optimise and classify afresh
    # at the initial pose
    obs = np.array(obs); obs[:, 3] = 1e30
    T, flags, ninl, tr = M.pose_optimization(cam, T0, obs, want_trace=True)
    assert tr["flags"][0].all()                                                # (the precondition: round 0 leaves no level-0 edge)
    assert T.tobytes() == M.to_cvmat(init).tobytes() and len(tr["flags"]) == 4 and ninl == 12 - flags.sum()


def _turns():
    """(label, unit axis, angle in rad, double rotation matrix): the turned cases' axes and angles, the two exact float blocks among them as they are, and
    100 seeded random axes with angles in (120, 180] degrees.  The matrices come from Rodrigues' formula (Cs.axis_angle), which shares nothing with the model."""
    out = []
    for a, deg in Cs.TURN_ANGLES:
        axis = np.asarray(Cs.TURN_AXES[a]) / np.linalg.norm(Cs.TURN_AXES[a])
        out.append((f"{a} {deg:+.0f}", axis, np.radians(deg), Cs.axis_angle(axis, deg)))
        if deg == 180.0:
            out.append((f"{a} pi exact", axis, np.pi, Cs.TURN_PI[a]))
    out.append(("111 120 exact", np.ones(3) / np.sqrt(3.0), 2.0 * np.pi / 3.0, Cs.TURN_CYCLIC))
    # an axis almost along one coordinate with 1e-5 of another: two diagonal entries differ by 1e-10, and taking any but the largest makes the radicand
    # 4 q_i^2 = 4e-10 sin^2(a/2) out of numbers of size 1 - the choice of i is what keeps the precision, and only such a rotation shows a wrong choice
    for d in range(3):
        for s in range(3):
            if s != d:
                axis = np.zeros(3); axis[d] = 1.0; axis[s] = 1e-5; axis /= np.linalg.norm(axis)
                out += [(f"axis {d} + 1e-5 axis {s}, {deg:+.0f}", axis, np.radians(deg), Cs.axis_angle(axis, deg)) for deg in (130.0, -130.0, 175.0, -175.0)]
    rng = np.random.default_rng(120)
    for k in range(100):
        axis = rng.normal(0, 1, 3); axis /= np.linalg.norm(axis)
        deg = 180.0 - rng.uniform(0.0, 60.0) * (k > 0)                          # (120, 180], the first one 180 itself
        out.append((f"random {k}", axis, np.radians(deg), Cs.axis_angle(axis, deg)))
    return out


def test_quaternion_of_a_rotation_past_120_degrees():
    """quat_of_matrix's trace <= 0 half and normalize_rotation's flip - what every turned case of the kernel tests is compared with - against the closed
    form: a rotation by a about the unit axis n has q = (n sin(a/2), cos(a/2)), up to the sign that makes w >= 0; and rotation_matrix gives R back.

    Bound 1e-14 per entry, for both.  R's entries are sums of three products of numbers below 1, each rounded: a few 1e-16 absolute.  In the trace <= 0
    half the radicand is 1 + m_ii - m_jj - m_kk = 4 q_i^2 with q_i the largest of x, y, z; trace <= 0 means w^2 <= 1/4, so x^2 + y^2 + z^2 >= 3/4 and
    q_i >= 0.5: the radicand is >= 1 and the few 1e-16 it carries stay a few 1e-16 through the square root and the division by 2 q_i >= 1 that gives the
    other three entries (sums and differences of two entries of R: 4e-16 at most each).  The normalisation divides by 1 + O(1e-16).  rotation_matrix
    multiplies pairs of entries and doubles: about ten roundings of numbers below 2.  Forty times 2.2e-16 covers it; a wrong sign or index changes an
    entry by the size of 2 w q_i >= 0.4 at 130 degrees, thirteen orders above the bound.  At |w| below the bound itself (the half turns) q and -q are the
    same statement, so the overall sign is left open there, and only there; w >= 0 is asserted always."""
    bound = 1e-14
    worst_q = worst_r = 0.0
    took = set()
    for label, axis, a, R in _turns():
        want = np.concatenate([axis * np.sin(a / 2.0), [np.cos(a / 2.0)]])
        if want[3] < 0:
            want = -want
        raw = M.quat_of_matrix(R)
        q = M.normalize_rotation(raw)
        assert q[3] >= 0, label
        dq = np.abs(q - want).max()
        if abs(want[3]) < bound:
            dq = min(dq, np.abs(q + want).max())
        dr = np.abs(M.rotation_matrix(q) - R).max()
        worst_q, worst_r = max(worst_q, dq), max(worst_r, dr)
        assert dq <= bound and dr <= bound, (label, dq, dr, q, want)
        if R[0, 0] + R[1, 1] + R[2, 2] <= 0.0:
            took.add((int(np.argmax(np.diag(R))), bool(raw[3] < 0)))
    print(f"{len(_turns())} rotations: largest |q - closed form| {worst_q:.3e}, largest |rotation_matrix(q) - R| {worst_r:.3e}, bound {bound:.1e}; (i, w < 0) taken {sorted(took)}")
    assert took == {(i, s) for i in range(3) for s in (False, True)}            # every largest diagonal entry, with w of either sign before the flip


def test_turned_and_degenerate_cases_show_what_they_are_for():
    """the preconditions tests/golden/make_golden_pose_opt_spread.py asserted when it kept the seeds, once more on the kept seeds: the turned cases take
    every i of the trace <= 0 half with w of either sign and the two exact traces, the control does not; the degenerate cases are degenerate"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_pose_opt_spread.py")
    spec = importlib.util.spec_from_file_location("make_golden_pose_opt_spread", path)
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    g = np.load(os.path.join(os.path.dirname(path), "pose_opt_spread.npz"))
    b = {n: G.quaternion_branch(Cs.case(n, int(g[n + "/seed"]))[1]) for n in Cs.TURNED}
    assert b.pop("turn_y_p110")[1] is None
    assert {(v[1], v[2]) for v in b.values()} >= {(i, s) for i in range(3) for s in (False, True)}
    assert b["turn_111_120_exact"][0] == 0.0 and all(b[f"turn_{a}_pi_exact"][0] == -1.0 for a in "xyz") and all(v[0] <= 0.0 for v in b.values())
    for n in ("all_outliers_12", "all_outliers_300", "zero_residual", "behind_camera", "float_product_pose"):
        assert G.preconditions(n, int(g[n + "/seed"])) is None, n


def camera_centre_problem():
    """n65_mixed_30 of the case set with R = I in the initial pose and point 5 exactly at the initial camera centre (with R = I the centre -t is a float
    vector, so R X + t is exactly 0): that edge's chi2 is non-finite from the first evaluation on"""
    cam, T0, obs, info = Cs.make(65, "mixed", 0.3, 0)
    T0 = np.array(T0); T0[:3, :3] = np.eye(3, dtype=np.float32)
    obs = np.array(obs); obs[5, 4:7] = -T0[:3, 3]
    return cam, T0, obs


def test_stale_errors_change_the_flags_of_a_whole_problem():
    """A level-0 edge is classified by the error the round's last computeActiveErrors left: after a rejected last trial that is the rejected pose's error
    (pop() restores the estimate, not the errors).  A whole problem where this decides the returned flags: one point at the initial camera centre.  Its
    chi2 is non-finite, so the system is, so every trial pose is NaN and is rejected; every round ends on such a trial, and every level-0 edge is
    classified from a NaN chi2, which is not > its threshold: no edge is flagged.  Fresh errors at the estimate (the initial pose, 0.02 rad and 5 cm off,
    with 30 % gross outliers) would flag most of them."""
    cam, T0, obs = camera_centre_problem()
    T, flags, ninl, tr = M.pose_optimization(cam, T0, obs, want_trace=True)
    assert tr["stale_matters"] and tr["round_ends_rejected"] == 4 and tr["accepted"] == 0
    assert flags.sum() == 0 and ninl == 65
    P = M.Problem(cam, obs)
    init = M.to_se3quat(T0)
    fresh, chi2 = M.classify(P, np.zeros(65, bool), init, init, fresh=True)
    print(f"stale rule flags {int(flags.sum())} of 65, fresh errors at the estimate would flag {int(fresh.sum())}")
    assert fresh.sum() >= 20 and not fresh[5] and not np.isfinite(chi2[5])      # (the edge at the centre itself is NaN under both rules)
    assert T.tobytes() == M.to_cvmat(init).tobytes()                           # the estimate never moved


def test_stale_errors_are_what_the_classification_reads():
    """The same rule on finite data, where a round ends on a rejected trial after ten trials in a row failed.  (1) There the chi2 a level-0 edge is
    classified by differs from a fresh one by more than 10 float ulps (1.2e-6 relative: the comparison is made in float).  (2) Given such a round's two
    poses, an observation whose chi2 lies between the two values gets a different flag from the two rules.  Step (2) rescales one observation's inv_sigma2
    AFTER the round was run: with finite data the tenth rejected step is ~1e-9 of a Gauss-Newton step, edges near their threshold move by less than a float
    step, and no complete finite problem with different returned flags is in this file (the whole-problem case is the test above)."""
    cam, T0, obs, info = Cs.make(5000, "mono", 0.3, 0)
    P = M.Problem(cam, obs)
    init = M.to_se3quat(T0)
    trace = {"accepted": 0, "rejected": 0, "terminate_trials": 0, "three_strikes": 0}
    flags = np.zeros(P.n, bool)
    found = None
    for rnd in range(4):
        cur, last = M.optimize(P, init, ~flags, rnd < 3, None, trace)
        _, c_cur, *_ = M.errors(P, cur); _, c_last, *_ = M.errors(P, last)
        if last is not cur:
            with np.errstate(all="ignore"):
                rel = np.where(~flags & (c_cur > 0), np.abs(c_last - c_cur) / c_cur, 0.0)
            if rel.max() > 1.2e-6:
                found = (rnd, int(rel.argmax()), cur, last, flags.copy())
                break
        flags, _ = M.classify(P, flags, cur, last)
    assert found is not None, "no round of this case ends on a rejected trial with stale errors more than 10 float ulps from fresh ones"
    rnd, i, cur, last, flags = found
    o = np.array(obs)
    _, c_cur, *_ = M.errors(P, cur); _, c_last, *_ = M.errors(P, last)
    o[i, 3] = np.float32(obs[i, 3] * 5.991 / (0.5 * (c_cur[i] + c_last[i])))     # chi2 is linear in inv_sigma2: the threshold now lies between the two values
    P2 = M.Problem(cam, o)
    stale, _ = M.classify(P2, flags, cur, last)
    fresh, _ = M.classify(P2, flags, cur, last, fresh=True)
    assert stale[i] != fresh[i] and stale[i] == (c_last[i] > c_cur[i])
    assert np.array_equal(np.delete(stale, i), np.delete(fresh, i))
