"""tests/sim3_model.py on its own (no library): the Jacobi eigen-solver against numpy, Horn's closed form on exact similarities, the integer
thresholds, the selection rules, SetRansacParameters, the draw queue, the non-finite case and the variants the recorded spread is made of."""
import numpy as np
import pytest

import sim3_cases as Cs
import sim3_model as M

f32 = np.float32


@pytest.mark.parametrize("n", [2, 4, 7, 12])
def test_jacobi_equals_eigh(n):
    rng = np.random.default_rng(n)
    for _ in range(20):
        B = rng.normal(size=(n, n)) * 10.0 ** rng.integers(-3, 4)
        A = B + B.T
        w, V = M.jacobi(A)
        w, V = np.array(w), np.array(V)
        order = np.argsort(w)
        assert np.allclose(w[order], np.linalg.eigvalsh(A), rtol=1e-12, atol=1e-12 * np.abs(A).max())
        assert np.allclose(V.T @ V, np.eye(n), atol=1e-13) and np.allclose(A @ V, V * w, atol=1e-11 * np.abs(A).max())


def test_jacobi_survives_a_tiny_off_diagonal_and_non_finite_input():
    w, V = M.jacobi([[1.0, 1e-200], [1e-200, 3.0]])                              # theta ~ 1e200: theta * theta overflows
    assert w == [1.0, 3.0] and np.isfinite(V).all()
    w, V = M.jacobi([[1e300, 1e-10, 0, 0], [1e-10, -1e300, 0, 0], [0, 0, 1, 0.5], [0, 0, 0.5, 2]])
    assert np.isfinite(w).all() and np.isfinite(V).all()
    w, V = M.jacobi([[1.0, np.nan], [np.nan, 2.0]])                             # returns: the sweep bound is a constant
    assert not np.isfinite(w).all()


def test_largest_eigenvector_has_a_non_negative_first_entry_and_takes_the_first_of_a_tie():
    v = M.largest_eigenvector([[0.0, -1.0, 0, 0], [-1.0, 0.0, 0, 0], [0, 0, -5.0, 0], [0, 0, 0, -6.0]])
    assert v[0] > 0 and abs(v[0] + v[1]) < 1e-15
    assert M.largest_eigenvector(np.diag([2.0, 2.0, 1.0, 0.0])) == [1.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 1.3])
def test_horn_recovers_an_exact_similarity(mode, scale):
    rng = np.random.default_rng(int(scale * 10) + mode)
    for _ in range(20):
        R = Cs.rotation(rng.normal(size=3), rng.uniform(0.01, 3.0))
        t = rng.uniform(-2, 2, 3)
        X2 = rng.uniform(-3, 3, (3, 3)) + [0, 0, 6]
        X1 = scale * X2 @ R.T + t
        Rm, tm, sm = M.horn(X1.T.astype(f32), X2.T.astype(f32), False, mode)
        assert np.abs(Rm.reshape(3, 3) - R).max() < 2e-5 and np.abs(tm - t).max() < 2e-4 and abs(sm - scale) < 2e-5
        if scale == 1.0:
            Rf, tf, sf = M.horn(X1.T.astype(f32), X2.T.astype(f32), True, mode)
            assert sf == f32(1.0) and np.abs(Rf - Rm).max() == 0 and np.abs(tf - t).max() < 2e-4
        T12, T21 = M.transforms(Rm, tm, sm, mode)
        assert np.abs(T12.astype(float) @ T21.astype(float) - np.eye(4)).max() < 1e-5
        assert T12[3].tolist() == [0, 0, 0, 1] and T21[3].tolist() == [0, 0, 0, 1]


def test_the_two_gemm_modes_differ_somewhere():
    corr, tri, *_ = Cs.case("n300_h300_fix_m0")
    a = M.iterate(Cs.K1, Cs.K2, corr, tri[:40], False, 0)
    b = M.iterate(Cs.K1, Cs.K2, corr, tri[:40], False, 1)
    assert a["hyp_t"].tobytes() != b["hyp_t"].tobytes() and np.abs(a["hyp_t"] - b["hyp_t"]).max() < 1e-4


def test_thresholds_are_truncated_integers():
    thr = M.max_error(Cs.level_sigma2())
    assert thr.tolist() == [9.0, 13.0, 19.0, 27.0, 39.0, 57.0, 82.0, 118.0]     # 9.21 * 1.2^(2 l), truncated
    assert thr.dtype == f32


def test_select_rules():
    assert M.select([3, 5, 5, 2], 0, 6, 4) == (4, -1, 2, 5)                     # a later tie replaces the best
    assert M.select([3, 7, 9], 0, 6, 3) == (2, 1, 1, 7)                         # the first new best above min_inliers returns
    assert M.select([3, 6, 2], 0, 6, 3) == (3, -1, 1, 6)                        # strictly above
    assert M.select([3, 6, 2], 7, 1, 3) == (3, -1, -1, 7)                       # nothing reaches the incoming best
    assert M.select([3, 7, 2], 7, 1, 3) == (2, 1, 1, 7)                         # ... equal to it is a new best
    assert M.select([9, 9, 9], 0, 1, 0) == (0, -1, -1, 0)
    assert M.select([1, 2, 9], 0, 6, 2) == (2, -1, 1, 2)                        # its_left cuts the loop


def test_ransac_max_its():
    assert M.ransac_max_its(150, 0.99, 6, 300) == 300
    assert M.ransac_max_its(150, 0.99, 75, 300) == 35                           # ceil(log(0.01) / log(1 - 0.125))
    assert M.ransac_max_its(10, 0.99, 10, 300) == 1                             # mRansacMinInliers == N
    assert M.ransac_max_its(10, 0.99, 11, 300) == 1                             # epsilon > 1: the log of a negative number
    assert M.ransac_max_its(0, 0.99, 6, 300) == 1
    assert M.ransac_max_its(100, 0.99, 0, 50) == 1                              # log(1) = 0: -inf
    assert M.ransac_max_its(64, 0.99, 40, 13) == 13


def test_identical_point_sets_give_a_nan_rotation_and_no_inliers():
    corr, tri, *_ = Cs.case("n20_h5_fix13_m0")
    corr = corr.copy(); corr[:3, 3:6] = corr[:3, 0:3]
    r = M.iterate(Cs.K1, Cs.K2, corr, [[0, 1, 2]], True, 0)
    assert np.isnan(r["hyp_R"]).all() and r["hyp_count"][0] == 0 and r["best"] == 0 and not r["inliers"].any()


def test_solver_queue_and_draw_order():
    corr, *_ = Cs.case("n64_h5_free_m0")
    calls = []

    def rand(lo, hi):
        calls.append((lo, hi))
        return (7 * len(calls)) % (hi + 1)

    s = M.Solver(Cs.K1, Cs.K2, corr, False, rand, 0)
    s.set_ransac_parameters(0.99, 30, 300)
    tri = s.take(5)
    assert len(tri) == 5 and calls == [(0, 63), (0, 62), (0, 61)] * 5 and all(len(set(t)) == 3 for t in tri)
    out = s.absorb(tri, dict(n_consumed=2, returned=1, best=1, best_inliers_out=40, T12=np.eye(4, dtype=f32), R12=None, t12=None, s12=None, inliers=np.ones(64, bool)))
    assert out[0] is not None and out[3] == 64 and s.iterations == 2 and s.queue == tri[2:]
    again = s.take(5)
    assert again[:3] == tri[2:] and len(calls) == 15 + 6                        # the queued triples first, two more drawn
    assert M.Solver(Cs.K1, Cs.K2, corr[:2], False, rand, 0).iterate(5)[1] is True and len(calls) == 21      # N < 3: no draw, bNoMore


def test_variants_stay_within_a_few_float_ulps_on_gated_triples():
    corr, tri, fix, mode, _ = Cs.case("n64_h300_free13_m1")
    worst = 0.0
    for t in tri[:60]:
        P1, P2 = corr[t, 0:3].T, corr[t, 3:6].T
        R, tt, s = M.horn(P1, P2, fix, mode)
        for v in (dict(eig="eigh"), dict(nudge=(1, 0, 0)), dict(nudge=(0, -1, 0)), dict(nudge=(0, 0, 1))):
            Rv, tv, sv = M.horn(P1, P2, fix, mode, **v)
            worst = max(worst, float((np.abs(Rv.astype(float) - R) / np.spacing(np.maximum(np.abs(R), f32(1e-3)))).max()))
    assert worst <= 4.0, worst
