"""The checks tests/test_sim3_emu.py (CPU emulation of the kernels) and tests/test_sim3_gpu.py (the device) share: orbhip_sim3_iterate and its batch form
against tests/sim3_model.py on the scenes of tests/sim3_cases.py, with the seeds and per-case tolerance of tests/golden/sim3_spread.npz.

How kernel and model are compared, so that no margin around a threshold is needed:
  1. Horn, per hypothesis, with tolerance: the kernel's hyp_R, hyp_t, hyp_s against the model's.  The kernel may deviate by 4 x the case's recorded
     spread (the largest deviation among the model's variants: eigenvector from numpy.linalg.eigh, atan2 / sin / cos one double ulp up and down) plus one
     float ulp per entry: the device's atan2, sin and cos may differ from libm's in a last bit, which is what the variants sample, and 4 x the largest of
     seven keeps false alarms rare; the ulp is the rounding to float.  |dR_ij| <= 4 spread_R + ulp(R_ij), |dt_i| <= 4 spread_t max|t| + ulp(t_i),
     |ds| <= 4 spread_s |s| + ulp(s).  (The recorded spreads are 0 on every case: the bound is one float ulp.)
  2. Everything after Horn is exact, FROM THE KERNEL'S OWN R, t, s: transforms and check_inliers of the model applied to hyp_R, hyp_t, hyp_s must give
     the kernel's masks and counts bit for bit, select on those counts its n_consumed, returned, best, best_inliers_out, and T12 and inliers follow.
  3. Where the kernel's R, t, s bits equal the model's on every hypothesis, the whole record equals the model's; under emulation that is asserted."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

import orb_slam2_amd
from orb_slam2_amd import orbhip as OH
import sim3_cases as Cs
import sim3_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sim3_spread.npz")
_golden = None
_cache = {}
f32 = np.float32


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def case(name):
    """(corr, triples, fix_scale, mode, min_inliers, the model's answer, the recorded spread): computed once, shared, never changed"""
    if name not in _cache:
        g = golden()
        corr, tri, fix, mode, mi = Cs.case(name, int(g[name + "/seed"]))
        m = M.iterate(Cs.K1, Cs.K2, corr, tri, fix, mode, mi, 0)
        assert m["hyp_R"].tobytes() == g[name + "/R"].reshape(-1, 3, 3).tobytes() and m["hyp_t"].tobytes() == g[name + "/t"].tobytes() and \
            m["hyp_s"].tobytes() == g[name + "/s"].tobytes(), f"{name}: the model no longer gives the recorded hypotheses - rerun tests/golden/make_golden_sim3_spread.py"
        for a in [corr, tri] + [v for v in m.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _cache[name] = (corr, tri, fix, mode, mi, m, g[name + "/spread"])
    return _cache[name]


def device(corr, tri, fix, mode, mi, best_in=0, library=None, K1=Cs.K1, K2=Cs.K2):
    return orb_slam2_amd.sim3_iterate(K1, K2, corr, tri, fix, mode, mi, best_in, per_hypothesis=True, library=library)


def same_record(a, b):
    """two answers (dicts of the ABI's names) are equal bit for bit"""
    for k in ("n_consumed", "returned", "best", "best_inliers_out"):
        if a[k] != b[k]:
            return False
    for k in ("T12", "R12", "t12", "s12", "inliers", "hyp_R", "hyp_t", "hyp_s", "hyp_count", "hyp_mask"):
        x, y = a.get(k), b.get(k)
        if (x is None) != (y is None) or (x is not None and np.asarray(x).tobytes() != np.asarray(y).tobytes()):
            return False
    return True


def horn_close(d, m, spread):
    """step 1; returns (ok, the largest excess over the tolerance)"""
    worst = -np.inf
    for k, sp, scale in (("hyp_R", spread[0], None), ("hyp_t", spread[1], "max"), ("hyp_s", spread[2], "self")):
        got, want = np.asarray(d[k], np.float64), np.asarray(m[k], np.float64)
        size = 1.0 if scale is None else np.abs(want).max(axis=-1, keepdims=True) if scale == "max" else np.abs(want)
        tol = 4.0 * sp * size + np.spacing(np.abs(np.asarray(m[k], f32))).astype(np.float64)
        if not np.isfinite(got).all():
            return False, np.inf
        worst = max(worst, float((np.abs(got - want) - tol).max()))
    return worst <= 0.0, worst


def after_horn_exact(d, corr, tri, mode, mi, best_in, K1=Cs.K1, K2=Cs.K2):
    """step 2: from the kernel's own R, t, s the model must reproduce everything else the kernel reports"""
    nh = len(tri)
    counts = np.zeros(nh, np.int32)
    masks = []
    for h in range(nh):
        T12, T21 = M.transforms(d["hyp_R"][h], d["hyp_t"][h], d["hyp_s"][h], mode)
        mask, counts[h] = M.check_inliers(T12, T21, K1, K2, corr, mode)
        assert np.array_equal(M.pack_mask(mask), d["hyp_mask"][h]), (h, np.flatnonzero(M.pack_mask(mask) != d["hyp_mask"][h])[:4])
        masks.append(mask)
    assert np.array_equal(counts, d["hyp_count"]), np.flatnonzero(counts != d["hyp_count"])[:8]
    cons, ret, best, run = M.select(counts, best_in, mi, nh)
    assert (d["n_consumed"], d["returned"], d["best"], d["best_inliers_out"]) == (cons, ret, best, run), (d["n_consumed"], d["returned"], d["best"], d["best_inliers_out"], cons, ret, best, run)
    if best >= 0:
        assert d["T12"].tobytes() == M.transforms(d["hyp_R"][best], d["hyp_t"][best], d["hyp_s"][best], mode)[0].tobytes()
        assert d["R12"].tobytes() == d["hyp_R"][best].tobytes() and d["t12"].tobytes() == d["hyp_t"][best].tobytes() and d["s12"] == d["hyp_s"][best]
        assert np.array_equal(d["inliers"], masks[best])
    else:
        assert d["T12"] is None and d["inliers"] is None
    return counts


def horn_bits_equal(d, m):
    return all(np.asarray(d[k]).tobytes() == np.asarray(m[k]).tobytes() for k in ("hyp_R", "hyp_t", "hyp_s"))


def check_case(name, library, exact):
    corr, tri, fix, mode, mi, m, spread = case(name)
    d = device(corr, tri, fix, mode, mi, library=library)
    ok, over = horn_close(d, m, spread)
    print(f"{name}: n {len(corr)}, {len(tri)} hypotheses, consumed {d['n_consumed']}, returned {d['returned']}, best {d['best']} with {d['best_inliers_out']} inliers, "
          f"largest |difference| - tolerance {over:.3e}, Horn bits equal: {horn_bits_equal(d, m)}")
    assert ok, (name, over)
    after_horn_exact(d, corr, tri, mode, mi, 0)
    if exact:
        assert horn_bits_equal(d, m), name
    if horn_bits_equal(d, m):
        assert same_record(d, m), name


def check_rejected_share():
    for name in Cs.ALL_NAMES:
        case(name)
    assert Cs.rejected_share() < 0.05, Cs.TALLY


# ------------------------------------------------------------------------------------------------ dedicated cases
def check_threshold_is_truncated(library):
    """Level 0: the threshold is (float)(size_t)(9.21 * 1) = 9, not 9.21.  Three exact correspondences of a quarter turn about z give the transform; two more
    are placed, from the model's own T12, so that one's error in image 1 is about 9.1 and the other's about 8.9.  Only the second may be an inlier."""
    X2 = np.array([[1.0, 0.5, 4.0], [-1.0, 1.0, 5.0], [0.5, -1.0, 6.0]])
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([0.25, -0.5, 0.125])
    X1 = X2 @ Rz.T + t
    big = Cs.level_sigma2()[7]
    corr = [np.concatenate([X1[i], X2[i], [1.0, 1.0]]) for i in range(3)]
    R, tt, s = M.horn(np.array(X1, f32).T, np.array(X2, f32).T, True, 0)
    T12, T21 = M.transforms(R, tt, s, 0)
    P = np.array([0.3, 0.2, 5.0])
    p1 = T12[:3, :3].astype(float) @ P + T12[:3, 3]
    for target in (9.1, 8.9):
        q = p1.copy(); q[0] += np.sqrt(target) * q[2] / float(Cs.K1[0])             # sqrt(target) pixels along u in image 1
        corr.append(np.concatenate([q, P, [1.0, big]]))
    corr = np.array(corr, f32)
    e1, e2 = M.reprojection_errors(T12, T21, Cs.K1, Cs.K1, corr, 0)
    assert 9.0 < e1[3] < 9.21 and 8.5 < e1[4] < 9.0 and e2[3] < 60 and e2[4] < 60, (e1, e2)     # the first would pass an untruncated threshold
    assert M.max_error(corr[:, 6])[3] == 9.0 and M.max_error(corr[:, 7])[3] == 118.0 and 118.0 < 9.21 * float(big) < 119.0
    tri = np.array([[0, 1, 2]], np.int32)
    d = device(corr, tri, True, 0, 100, library=library, K2=Cs.K1)
    after_horn_exact(d, corr, tri, 0, 100, 0, K2=Cs.K1)
    assert d["inliers"].tolist() == [True, True, True, False, True], d["inliers"]
    assert d["hyp_count"][0] == 4 and d["returned"] == -1 and d["best"] == 0


def _counts_case():
    corr, tri, fix, mode, mi, m, _ = case("n64_h300_free13_m1")
    return corr, tri, fix, mode, m["hyp_count"]


def check_select_rules(library):
    """strict `>` against min_inliers, a later tie replaces the best, best_inliers_in above every count, the return at the first, a middle and the last
    hypothesis - each against select() on the kernel's own counts, and against what the rule says"""
    corr, tri, fix, mode, counts = _counts_case()
    order = np.argsort(counts, kind="stable")
    good, bad = int(order[-1]), [int(k) for k in order[:4]]
    cg = int(counts[good])
    assert all(counts[b] < cg for b in bad)
    # min_inliers equal to the best count: no return; one less: the return
    t5 = tri[[bad[0], good, bad[1], bad[2], bad[3]]]
    d = device(corr, t5, fix, mode, cg, library=library)
    c = after_horn_exact(d, corr, t5, mode, cg, 0)
    assert c[1] == cg and d["returned"] == -1 and d["n_consumed"] == 5 and d["best"] == 1 and d["best_inliers_out"] == cg
    d = device(corr, t5, fix, mode, cg - 1, library=library)
    after_horn_exact(d, corr, t5, mode, cg - 1, 0)
    assert d["returned"] == 1 and d["n_consumed"] == 2 and d["best"] == 1
    # a later tie replaces the best (the same triple twice gives the same count)
    tt = tri[[good, bad[0], good, bad[1]]]
    d = device(corr, tt, fix, mode, cg, library=library)
    after_horn_exact(d, corr, tt, mode, cg, 0)
    assert d["best"] == 2 and d["returned"] == -1 and d["hyp_count"][0] == d["hyp_count"][2] == cg
    # best_inliers_in above every count: nothing becomes a best
    d = device(corr, t5, fix, mode, 6, best_in=cg + 1, library=library)
    after_horn_exact(d, corr, t5, mode, 6, cg + 1)
    assert d["best"] == -1 and d["returned"] == -1 and d["n_consumed"] == 5 and d["best_inliers_out"] == cg + 1 and d["inliers"] is None
    # ... and equal to the best count: that hypothesis is a new best and returns
    d = device(corr, t5, fix, mode, 6, best_in=cg, library=library)
    after_horn_exact(d, corr, t5, mode, 6, cg)
    assert d["best"] == 1 and d["returned"] == 1
    # the return at hypothesis 0, in the middle and at the last one
    for pos in (0, 2, 4):
        idx = [bad[0], bad[1], bad[2], bad[3]]
        idx.insert(pos, good)
        tp = tri[idx]
        d = device(corr, tp, fix, mode, cg - 1, library=library)
        after_horn_exact(d, corr, tp, mode, cg - 1, 0)
        assert d["returned"] == pos and d["n_consumed"] == pos + 1 and d["best"] == pos, (pos, d["returned"])
    # more than one pass of the selection wave (64 counts a pass): the return in the second pass, the running best carried over
    idx = [bad[k % 4] for k in range(70)]
    idx[66] = good
    tp = tri[idx]
    d = device(corr, tp, fix, mode, cg - 1, library=library)
    after_horn_exact(d, corr, tp, mode, cg - 1, 0)
    assert d["returned"] == 66 and d["n_consumed"] == 67


def check_untouched_without_best(library):
    """best = -1: T12, R12, t12, s12 and the inliers buffer keep what the caller put there"""
    corr, tri, fix, mode, counts = _counts_case()
    rec = OH._Sim3Problem()
    keep = OH._sim3_fill(rec, dict(K1=Cs.K1, K2=Cs.K2, corr=corr, triples=tri[:5], fix_scale=fix, gemm_mode=mode, min_inliers=6, best_inliers_in=int(counts[:5].max()) + 1), False)
    keep["inliers"][:] = 7
    rec.T12[:] = [-5.0] * 16; rec.R12[:] = [-5.0] * 9; rec.t12[:] = [-5.0] * 3; rec.s12 = -5.0
    L = orb_slam2_amd.lib(library)
    assert L.orbhip_sim3_iterate(0, C.byref(rec)) == 0, L.orbhip_last_error()
    assert rec.best == -1 and rec.returned == -1 and rec.n_consumed == 5
    assert (keep["inliers"] == 7).all() and all(v == -5.0 for v in list(rec.T12) + list(rec.R12) + list(rec.t12)) and rec.s12 == -5.0


def check_non_finite(library):
    """identical point sets (an exactly symmetric M: vec == 0, 0/0, a NaN R, 0 inliers) and a collinear triple (a double largest eigenvalue): the call
    returns, the finite pattern equals the model's and everything after Horn follows exactly from the kernel's own R, t, s"""
    corr, tri, fix, mode, mi, m, _ = case("n65_h5_fix_m0")
    corr = corr.copy()
    corr[0:3, 3:6] = corr[0:3, 0:3]                                             # identical sets
    line = np.array([0.5, -0.25, 1.0], f32)
    for k, a in enumerate((4.0, 5.0, 7.0)):                                     # both sets on one line through the origin, the second at twice the distance
        corr[10 + k, 0:3] = line * f32(a); corr[10 + k, 3:6] = line * f32(2.0 * a)
    tri = np.array([[0, 1, 2], [10, 11, 12], [2, 1, 0], tri[0], [12, 10, 11]], np.int32)
    for md in (0, 1):
        for fx in (True, False):
            mm = M.iterate(Cs.K1, Cs.K2, corr, tri, fx, md, mi, 0)
            d = device(corr, tri, fx, md, mi, library=library)
            for k in ("hyp_R", "hyp_t", "hyp_s"):
                assert np.array_equal(np.isfinite(d[k]), np.isfinite(mm[k])), (k, md, fx, d[k], mm[k])
            assert not np.isfinite(d["hyp_R"][0]).any() and d["hyp_count"][0] == 0 and d["hyp_count"][2] == 0
            after_horn_exact(d, corr, tri, md, mi, 0)
            assert np.isfinite(d["hyp_R"][3]).all() and d["hyp_count"][3] > 0


def _raw(corr, tri, **kw):
    rec = OH._Sim3Problem()
    q = dict(K1=Cs.K1, K2=Cs.K2, corr=corr, triples=tri, fix_scale=True, gemm_mode=0, min_inliers=6, best_inliers_in=0)
    q.update(kw)
    return rec, OH._sim3_fill(rec, q, False)


def check_refused_inputs(library):
    L = orb_slam2_amd.lib(library)
    corr, tri, *_ = case("n20_h5_fix13_m0")

    def refused(rec, status, word):
        st = L.orbhip_sim3_iterate(0, C.byref(rec))
        msg = L.orbhip_last_error()
        assert st == status and msg != b"" and word in msg.decode(), (st, msg)

    rec, keep = _raw(corr, tri, gemm_mode=2)
    refused(rec, OH.ERR_UNSUPPORTED, "gemm_mode 2")
    rec, keep = _raw(corr, tri, gemm_mode=3)
    refused(rec, OH.ERR_INVALID, "gemm_mode")
    bad = tri.copy(); bad[3, 1] = len(corr)
    rec, keep = _raw(corr, bad)
    refused(rec, OH.ERR_INVALID, "outside 0..19")
    bad = tri.copy(); bad[2, 0] = -1
    rec, keep = _raw(corr, bad)
    refused(rec, OH.ERR_INVALID, "outside")
    bad = tri.copy(); bad[4, 2] = bad[4, 0]
    rec, keep = _raw(corr, bad)
    refused(rec, OH.ERR_INVALID, "twice")
    for field in ("corr", "triples", "inliers"):
        rec, keep = _raw(corr, tri)
        setattr(rec, field, None)
        refused(rec, OH.ERR_INVALID, "null")
    rec, keep = _raw(corr, np.tile(tri, (1000, 1))[:4097])
    refused(rec, OH.ERR_INVALID, "4097")
    assert L.orbhip_sim3_iterate(0, None) == OH.ERR_INVALID and L.orbhip_last_error() != b""
    assert L.orbhip_sim3_iterate_batch(0, 2, None) == OH.ERR_INVALID and L.orbhip_last_error() != b""
    assert L.orbhip_sim3_iterate_batch(0, -1, C.byref(rec)) == OH.ERR_INVALID
    rec, keep = _raw(corr, np.tile(tri, (1000, 1))[:4096], min_inliers=1000)     # ... and 4096 are served
    assert L.orbhip_sim3_iterate(0, C.byref(rec)) == 0 and rec.n_consumed == 4096


def check_short_untouched(library):
    """n < 3 or no hypothesis: n_consumed = 0, returned = best = -1, nothing else written"""
    L = orb_slam2_amd.lib(library)
    corr, tri, *_ = case("n20_h5_fix13_m0")
    for n, nh in ((0, 5), (1, 5), (2, 5), (20, 0)):
        rec, keep = _raw(corr[:n], np.zeros((nh, 3), np.int32) if n < 3 else tri[:nh])
        full = np.full(24, 7, np.uint8)
        rec.inliers = full.ctypes.data
        rec.n_consumed, rec.returned, rec.best, rec.best_inliers_out = 9, 9, 9, -3
        rec.T12[:] = [-5.0] * 16; rec.R12[:] = [-5.0] * 9; rec.t12[:] = [-5.0] * 3; rec.s12 = -5.0
        assert L.orbhip_sim3_iterate(0, C.byref(rec)) == 0, L.orbhip_last_error()
        assert (rec.n_consumed, rec.returned, rec.best, rec.best_inliers_out) == (0, -1, -1, -3), (n, nh)
        assert (full == 7).all() and all(v == -5.0 for v in list(rec.T12) + list(rec.R12) + list(rec.t12)) and rec.s12 == -5.0
    rec, keep = _raw(corr, tri, min_inliers=1000)                                # ... and n bytes, no more, are written otherwise
    full = np.full(24, 7, np.uint8)
    rec.inliers = full.ctypes.data
    assert L.orbhip_sim3_iterate(0, C.byref(rec)) == 0 and rec.best >= 0
    assert (full[20:] == 7).all() and (full[:20] <= 1).all()


# ------------------------------------------------------------------------------------------------ batch, repeat, threads
BATCH = ["n64_h5_free_m0", "n3_h5_fix_m0", "n1000_h5_free13_m0", None, "n300_h300_fix_m0", "n4_h5_free13_m1", "n129_h1_free_m1", "n64_h5_free_m0",
         "n20_h300_free13_m0", "n65_h5_fix_m0", "n63_h5_fix_m1", "n300_h5_fix13_m0", "n1000_h300_fix_m1", "n129_h5_fix_m0", "n65_h1_free13_m1", "n64_h5_free_m0"]


def _problem(name):
    corr, tri, fix, mode, mi, *_ = case(name)
    return dict(K1=Cs.K1, K2=Cs.K2, corr=corr, triples=tri, fix_scale=fix, gemm_mode=mode, min_inliers=mi, best_inliers_in=0)


def check_batch_slots(library):
    """a problem alone, and the same problem at slots 0, 7 and 15 of a mixed-size batch of 16: the same bits; every other slot equals its own single call"""
    short = _problem("n20_h5_fix13_m0")
    short["corr"] = short["corr"][:2]; short["triples"] = np.zeros((5, 3), np.int32)
    probs = [_problem(n) if n else short for n in BATCH]
    out = orb_slam2_amd.sim3_iterate_batch(probs, per_hypothesis=True, library=library)
    assert len(out) == 16
    alone = device(*case("n64_h5_free_m0")[:5], library=library)
    for k in (0, 7, 15):
        assert same_record(out[k], alone), k
    assert (out[3]["n_consumed"], out[3]["returned"], out[3]["best"]) == (0, -1, -1)
    for k, n in enumerate(BATCH):
        if n is not None:
            assert same_record(out[k], device(*case(n)[:5], library=library)), (k, n)
    assert orb_slam2_amd.sim3_iterate_batch([], library=library) == []


def check_repeat(library):
    a = device(*case("n300_h300_free13_m1")[:5], library=library)
    b = device(*case("n300_h300_free13_m1")[:5], library=library)
    assert same_record(a, b)


def check_three_threads(library):
    names = ["n64_h300_free13_m1", "n300_h300_fix_m0", "n1000_h5_free13_m0"]
    want = {n: device(*case(n)[:5], library=library) for n in names}
    out, errs = {}, []

    def work(name):
        try:
            for _ in range(3):
                out[name] = device(*case(name)[:5], library=library)
            orb_slam2_amd.lib(library).orbhip_thread_release()
        except Exception as e:                                                # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for n in names:
        assert same_record(out[n], want[n]), n


# ------------------------------------------------------------------------------------------------ the class's loop on the device
class DeviceSolver(M.Solver):
    """the model's solver state and draw queue around the device's answers"""

    def __init__(self, *a, library=None, **kw):
        self.library = library
        super().__init__(*a, **kw)

    def solve(self, tri):
        return orb_slam2_amd.sim3_iterate(self.K1, self.K2, self.corr, tri, self.fix_scale, self.mode, self.min_inliers, self.best_inliers, library=self.library)


class ScriptedRandom:
    """DUtils::Random::RandomInt from a seeded generator, counting its calls"""

    def __init__(self, seed):
        self.rng, self.calls = np.random.default_rng(seed), []

    def __call__(self, lo, hi):
        self.calls.append((lo, hi))
        return int(self.rng.integers(lo, hi + 1))


def check_solver_rounds(library, exact):
    """The class's loop around the device's answers (the model's Solver with solve() on the device), draw for draw:
      * N < mRansacMinInliers: no draw, bNoMore;
      * iterate(5) rounds that never return, mRansacMaxIts = 13: 5 + 5 + 3 hypotheses - the last round has its_left < n_hyp - then bNoMore;
      * an early return leaves the triples not consumed queued, and the next call takes them before it draws.
    With `exact` (emulation) every round also equals the model's solver on the same draws."""
    corr, _ = Cs.scene(64, 1.0, 3, wrong=0.7)
    corr2, _, fix2, mode2, *_ = case("n64_h5_free_m0")

    def pair(c, fix, mode, seed):
        ra, rb = ScriptedRandom(seed), ScriptedRandom(seed)
        return DeviceSolver(Cs.K1, Cs.K2, c, fix, ra, mode, library=library), M.Solver(Cs.K1, Cs.K2, c, fix, rb, mode), ra, rb

    def both(a, b, n):
        x, y = a.iterate(n), b.iterate(n)
        if exact:
            assert (x[0] is None) == (y[0] is None) and x[1] == y[1] and x[3] == y[3] and np.array_equal(x[2], y[2]) and (x[0] is None or x[0].tobytes() == y[0].tobytes())
            assert a.iterations == b.iterations and a.queue == b.queue and a.best_inliers == b.best_inliers
        return x

    a, b, ra, rb = pair(corr, False, 1, 5)
    for s in (a, b):
        s.set_ransac_parameters(0.99, 1000, 13)
    T, no_more, inl, ninl = both(a, b, 5)
    assert T is None and no_more and ra.calls == [] and not inl.any() and ninl == 0

    for s in (a, b):
        s.set_ransac_parameters(0.99, 40, 13)
    assert a.max_its == 13
    for k, total in enumerate((5, 10, 13)):
        T, no_more, inl, ninl = both(a, b, 5)
        assert T is None and a.iterations == total and len(ra.calls) == 3 * total and no_more == (total == 13), (k, a.iterations, no_more)
        assert ra.calls[-3:] == [(0, 63), (0, 62), (0, 61)]
    assert a.queue == [] and a.best is not None and a.best_inliers <= 40
    T, no_more, inl, ninl = both(a, b, 5)
    assert T is None and no_more and len(ra.calls) == 39                        # exhausted: nothing is drawn any more
    assert not exact or ra.calls == rb.calls

    a, b, ra, rb = pair(corr2, fix2, mode2, 2)                                  # (this seed returns at the third hypothesis)
    for s in (a, b):
        s.set_ransac_parameters(0.99, 30, 300)
    rounds = 0
    while True:
        T, no_more, inl, ninl = both(a, b, 5)
        rounds += 1
        assert len(ra.calls) == 15 * rounds and rounds < 9
        if T is not None:
            break
    assert ninl > 30 and inl.sum() == ninl and not no_more
    left = len(a.queue)
    assert left == 5 * rounds - a.iterations and left > 0, (left, rounds, a.iterations)          # the early return left drawn triples queued
    first = list(a.queue)
    taken = a.take(5)
    assert taken[:left] == first and len(ra.calls) == 15 * rounds + 3 * (5 - left)               # ... which the next call takes before it draws
    a.absorb(taken, a.solve(taken))
    assert not exact or ra.calls[:15 * rounds] == rb.calls


# ------------------------------------------------------------------------------------------------ the C++ drop-in
def build_cpp(tmp, library, sanitize=False):
    """tests/sim3_cpp/main.cc + orb_slam2_amd/cpp/Sim3Solver.cc as a stand-alone program linked to `library`, in the directory tmp"""
    d, f = os.path.split(os.path.abspath(library))
    exe = os.path.join(str(tmp), "sim3_cpp_asan" if sanitize else "sim3_cpp")
    cmd = ["g++", "-std=c++14", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-DCVLITE_ALGEBRA", "-DORBHIP_USE_OPENCV"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    cmd += ["-I" + os.path.join(ROOT, "tests", "sim3_cpp"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "cvlite"),
            os.path.join(ROOT, "tests", "sim3_cpp", "main.cc"), os.path.join(ROOT, "orb_slam2_amd", "cpp", "Sim3Solver.cc"),
            "-o", exe, "-L" + d, "-l" + f[3:-3], "-Wl,-rpath," + d]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpp(exe, env=None):
    """the program under gemm modes 0 and 1 (equal to the C ABI; its SetRansacParameters equal to the model's) and 2 (refused at construction)"""
    for mode in ("0", "1", "2"):
        e = dict(os.environ if env is None else env)
        e["ORBHIP_GEMM_MODE"] = mode
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=e)
        assert r.returncode == 0 and "sim3_cpp ok" in r.stdout, (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        if mode == "2":
            assert "refused at construction" in r.stdout
            continue
        rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("maxits ")]
        assert len(rows) == 9, r.stdout
        for _, n, m, its, _, v in rows:
            assert M.ransac_max_its(int(n), 0.99, int(m), int(its)) == int(v), (n, m, its, v)
