"""tests/pnp_model.py alone (no library): its stated replacements of OpenCV's primitives against numpy.linalg, EPnP over all inliers against an
independent plain-numpy EPnP with the recorded spread (tests/golden/pnp_spread.npz), SetRansacParameters at its edges, the draw queue and the loop's
OR.  The minimal-set hypotheses are NOT compared with numpy.linalg: with four points the null space of M^T M has four dimensions and the result depends
on the basis the eigen-solver returns; there the stated Jacobi is the definition."""
import os

import numpy as np
import pytest

import pnp_cases as Cs
import pnp_model as M
import sim3_model as S3

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_spread.npz")
f32 = np.float32


def test_jacobi_batch_is_the_one_matrix_statement():
    rng = np.random.default_rng(1)
    mats = []
    for n in (3, 12):
        for _ in range(3):
            B = rng.normal(size=(n + 2, n))
            mats.append(B.T @ B)
        B = rng.normal(size=(n - 1, n))
        mats.append(B.T @ B)                                                    # rank-deficient
        mats.append(np.diag(np.arange(float(n))))                               # already diagonal: no sweep
    for n in (3, 12):
        group = [A for A in mats if len(A) == n]
        w, V = M.jacobi_batch(np.array(group))
        for k, A in enumerate(group):
            ws, Vs = S3.jacobi(A)
            assert np.array(ws).tobytes() == w[k].tobytes() and np.array(Vs).tobytes() == V[k].tobytes()
            assert np.allclose(np.sort(w[k]), np.linalg.eigvalsh(A), atol=1e-12 * max(1.0, np.abs(A).max()))


def test_sort_is_descending_with_ties_by_index_and_the_clamp():
    assert M.sort_desc([1.0, 3.0, 3.0, -2.0, 5.0]) == [4, 1, 2, 0, 3]
    assert M.sort_desc([2.0, 2.0, 2.0]) == [0, 1, 2]
    # an eigenvalue of PW0^T PW0 below zero is clamped before sqrt(dc / n): the control point coincides with the centroid, no NaN; without the clamp
    # the square root of a negative number would make it NaN
    c0, V = np.array([1.0, 2.0, 3.0]), np.eye(3)
    with np.errstate(all="ignore"):
        cws = M.control_points(c0, np.array([4.0, -1e-17, 1.0]), V, np.float64(4.0))
        assert np.isnan(np.sqrt(np.float64(-1e-17) / 4.0))
    assert cws.tolist() == [[1.0, 2.0, 3.0], [2.0, 2.0, 3.0], [1.0, 2.0, 3.5], [1.0, 2.0, 3.0]]


@pytest.mark.parametrize("nc", [3, 4, 5])
def test_qr_solve_against_lstsq(nc):
    rng = np.random.default_rng(nc)
    for _ in range(5):
        A, b = rng.normal(size=(6, nc)), rng.normal(size=6)
        x = M.qr_solve(A.copy(), b.copy(), np.zeros(nc))
        want = np.linalg.lstsq(A, b, rcond=None)[0]
        assert np.abs(x - want).max() <= 1e-12 * np.linalg.cond(A) * max(1.0, np.abs(want).max())
    A = rng.normal(size=(6, nc))
    A[:, 0] = 0.0                                                               # a zero column: x stays as it was
    assert M.qr_solve(A, rng.normal(size=6), np.full(nc, 7.0)).tolist() == [7.0] * nc


def test_hestenes_against_svd():
    rng = np.random.default_rng(5)
    for rank in (3, 3, 3, 2, 2):
        A = rng.normal(size=(3, 3))
        if rank == 2:
            U, s, Vt = np.linalg.svd(A)
            A = U @ np.diag([s[0], s[1], 0.0]) @ Vt
        U, s, V = M.hestenes(A)
        Un, sn, Vtn = np.linalg.svd(A)
        assert np.abs(s - sn).max() <= 1e-13 * sn[0]
        got, want = U @ V.T, Un @ Vtn
        if rank == 2:                                                           # the third pair is a free sign in numpy; the model takes the cross products
            want2 = Un @ np.diag([1.0, 1.0, -1.0]) @ Vtn
            assert min(np.abs(got - want).max(), np.abs(got - want2).max()) <= 1e-9
            assert abs(np.linalg.det(U) * np.linalg.det(V) - 1.0) <= 1e-9
        else:
            assert np.abs(got - want).max() <= 1e-12 * sn[0] / sn[2]


@pytest.mark.parametrize("scene", Cs.SPREAD_SCENES, ids=[s[0] for s in Cs.SPREAD_SCENES])
def test_epnp_over_all_inliers_against_an_independent_epnp(scene):
    name, n, seed, noise, planar = scene
    g = np.load(GOLDEN)
    corr, Rcw, tcw, _ = Cs.scene(n, seed, 0.0, noise, planar)
    R, t = M.epnp(corr, Cs.K, mask=np.ones(n, bool))
    assert R.tobytes() == g[name + "/model_R"].tobytes() and t.tobytes() == g[name + "/model_t"].tobytes(), "the model no longer gives the recorded pose - rerun tests/golden/make_golden_pnp_spread.py"
    Ri, ti = Cs.independent_epnp(corr, Cs.K)
    # The recorded spread is this scene's own figure and the model's pose is pinned to the golden's bits, so the first bound can only fail when
    # numpy's decompositions change; it is the form the model's yardstick takes in tests/sim3_checks.py.  The check with teeth is the second, against
    # the true pose on the noise-free scenes.  Why the noisy scenes spread up to 9e-4 in R is not established: the suspicion is that near-equal small
    # eigenvalues of M^T M give the two sides different bases for find_betas_approx_2 / _3, so that another of the three candidates wins.
    sp, truth = g[name + "/spread"], g[name + "/truth"]
    ulp = float(np.spacing(f32(1.0)))
    dR, dt = np.abs(R - Ri).max(), np.abs(t - ti).max() / np.abs(ti).max()
    print(f"{name}: model against the independent EPnP: R {dR:.3e} (recorded {sp[0]:.3e}), t {dt:.3e} (recorded {sp[1]:.3e})")
    assert dR <= 4.0 * sp[0] + ulp and dt <= 4.0 * sp[1] + ulp
    if noise == 0.0:
        eR, et = np.abs(R - Rcw).max(), np.abs(t - tcw).max() / np.abs(tcw).max()
        print(f"{name}: model against the true pose: R {eR:.3e}, t {et:.3e} (the independent EPnP: {truth[0]:.3e}, {truth[1]:.3e})")
        assert eR <= 4.0 * truth[0] + ulp and et <= 4.0 * truth[1] + ulp


def test_set_ransac_parameters_edges():
    P = M.ransac_parameters
    assert P(100, 0.99, 10, 300, 4, 0.5)[:2] == (50, 35)                         # Tracking's call: ceil(log(0.01) / log(1 - 0.125))
    assert P(19, 0.99, 10, 300, 4, 0.5)[0] == 10 and P(21, 0.99, 10, 300, 4, 0.5)[0] == 10 and P(22, 0.99, 10, 300, 4, 0.5)[0] == 11     # int(N * 0.5f) truncates
    assert P(10, 0.99, 8, 300, 4, f32(0.4))[0] == 8                              # 10 * 0.4f = 4.0000000596 -> 4: the minInliers clamp
    assert P(4, 0.99, 2, 300, 4, 0.4)[:2] == (4, 1)                              # the minSet clamp; N == mRansacMinInliers: one iteration
    assert P(5, 0.99, 5, 300, 4, 0.5)[:2] == (5, 1)
    n_min, its, eps = P(20, 0.99, 10, 300, 4, 0.4)
    assert (n_min, eps) == (10, f32(10) / f32(20)) and its == int(np.ceil(np.log(1 - 0.99) / np.log(1 - 0.5 ** 3)))      # epsilon raised to minInliers / N
    assert P(0, 0.99, 8, 300, 4, 0.4)[:2] == (8, 1)                              # N == 0: undefined in the reference, 1 here on every machine
    assert P(3, 0.99, 8, 300, 4, 0.4)[:2] == (8, 1)                              # epsilon = 8 / 3 > 1: log of a negative number, not finite -> 1
    assert P(1000, 0.99, 10, 300, 4, 0.01)[1] == 300                             # clipped by maxIterations
    assert P(100, 1.0, 10, 300, 4, 0.5)[1] == 1                                  # log(0) = -inf over a negative: +inf does not fit an int -> 1
    assert P(100, 0.99, 10, 0, 4, 0.5)[1] == 1                                   # max(1, ...)


def test_draw_queue_and_the_or_of_the_loop():
    calls = []

    class Canned(M.Solver):
        def solve(self, quads):
            calls.append([list(q) for q in quads])
            return self.answer(quads)

    rng = np.random.default_rng(2)
    corr = Cs.scene(30, 9, 0.3, 0.5)[0]
    s = Canned(Cs.K, corr, lambda lo, hi: int(rng.integers(lo, hi + 1)))
    s.set_ransac_parameters(0.99, 10, 12, 4, 0.5)
    assert s.max_its == 12 and s.min_inliers == 15
    # the first iterate(5) on a fresh solver runs max(5, 12 - 0) = 12 hypotheses; the device returns at the third, nine stay queued
    s.answer = lambda q: dict(n_consumed=3, returned=2, best=2, best_inliers_out=20, best_mask=np.ones(30, bool), best_Tcw=np.eye(4, dtype=f32),
                              refined_Tcw=np.eye(4, dtype=f32), refined_mask=np.ones(30, bool), refined_inliers=22)
    T, no_more, _, k = s.iterate(5)
    assert len(calls[0]) == 12 and all(len(set(q)) == 4 and min(q) >= 0 and max(q) < 30 for q in calls[0])
    assert T is not None and not no_more and k == 22 and s.iterations == 3 and s.queue == calls[0][3:]
    # the next iterate(5): max(5, 12 - 3) = 9, all from the queue, nothing drawn; none returns: the loop ends at mRansacMaxIts with the unrefined best
    s.answer = lambda q: dict(n_consumed=len(q), returned=-1, best=-1, best_inliers_out=20)
    T, no_more, mask, k = s.iterate(5)
    assert calls[1] == calls[0][3:] and s.queue == [] and s.iterations == 12 and no_more and k == 20 and T is not None and mask.all()
    # past mRansacMaxIts the OR still runs nIterations hypotheses a call
    assert s.loop_count(5) == 5 and s.loop_count(0) == 0
    T, no_more, _, _ = s.iterate(5)
    assert len(calls[2]) == 5 and s.iterations == 17 and no_more
    # N < mRansacMinInliers: bNoMore at once, nothing drawn
    few = Canned(Cs.K, corr[:7], lambda lo, hi: lo)                             # the default minInliers is 8
    assert few.iterate(5)[:2] == (None, True) and len(calls) == 3


def test_more_than_4096_hypotheses_are_split_with_the_best_carried():
    seen = []

    class Canned(M.Solver):
        def solve(self, quads):
            seen.append((len(quads), self.best_inliers))
            return dict(n_consumed=len(quads), returned=-1, best=0, best_inliers_out=self.best_inliers + 1, best_mask=np.ones(self.N, bool), best_Tcw=np.eye(4, dtype=f32))

    s = Canned(Cs.K, Cs.scene(30, 9, 0.3, 0.5)[0], lambda lo, hi: lo)
    s.set_ransac_parameters(0.99, 10, 300, 4, 0.5)
    s.iterate(5000)
    assert seen == [(4096, 0), (904, 1)] and s.iterations == 5000
