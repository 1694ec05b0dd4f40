"""The checks tests/test_pnp_emu.py (CPU emulation of the kernels) and tests/test_pnp_gpu.py (the device) share: orbhip_pnp_iterate and its batch form
against tests/pnp_model.py on the scenes of tests/pnp_cases.py.

There is no tolerance between kernel and model: EPnP as stated in DESIGN.md H18 needs +, -, *, / and sqrt only, every one correctly rounded on both
sides, so every per-hypothesis record, every refine record and the whole answer must be equal bit for bit.  One allowance, which is not a tolerance:
two NaNs are equal whatever their sign and payload (IEEE 754 leaves both open; x86 and the device differ), a NaN and a number are not."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import orb_slam2_amd
from orb_slam2_amd import orbhip as OH
import pnp_cases as Cs
import pnp_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_cache = {}
HEAD = ("n_consumed", "returned", "best", "best_inliers_out")
ARRAYS = ("best_Tcw", "best_mask", "refined_Tcw", "refined_inliers", "refined_mask", "hyp_R", "hyp_t", "hyp_count", "hyp_mask", "ref_hyp", "ref_R", "ref_t", "ref_count", "ref_mask")


def same_bits(a, b):
    if (a is None) != (b is None):
        return False
    if a is None:
        return True
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        u = np.uint64 if a.itemsize == 8 else np.uint32
        return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def differences(d, m):
    """the names in which a device answer differs from the model's"""
    bad = [k for k in HEAD if d[k] != m[k] and not (m[k] is None)]
    return bad + [k for k in ARRAYS if k in m and not same_bits(np.asarray(d[k]) if d[k] is not None else None, np.asarray(m[k]) if m[k] is not None else None)]


def model(corr, quads, mi, best_in=0, best_mask_in=None):
    return M.iterate(Cs.K, corr, quads, mi, best_in, best_mask_in)


def device(corr, quads, mi, best_in=0, best_mask_in=None, library=None):
    return orb_slam2_amd.pnp_iterate(Cs.K, corr, quads, mi, best_in, best_mask_in, per_hypothesis=True, library=library)


def case(name):
    """(corr, quads, min_inliers, the model's answer): computed once, shared, never changed"""
    if name not in _cache:
        corr, quads, mi, _, _ = Cs.case(name)
        m = model(corr, quads, mi)
        for a in [corr, quads] + [v for v in m.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _cache[name] = (corr, quads, mi, m)
    return _cache[name]


def check_case(name, library):
    corr, quads, mi, m = case(name)
    d = device(corr, quads, mi, library=library)
    hyp_equal = sum(same_bits(d["hyp_R"][h], m["hyp_R"][h]) and same_bits(d["hyp_t"][h], m["hyp_t"][h]) for h in range(len(quads)))
    print(f"{name}: n {len(corr)}, {len(quads)} hypotheses, min {mi}, consumed {d['n_consumed']}, returned {d['returned']}, best {d['best']} with {d['best_inliers_out']} inliers, "
          f"{len(d['ref_hyp'])} refines {list(d['ref_count'])}, hypotheses with the model's bits: {hyp_equal} of {len(quads)}")
    assert differences(d, m) == [], name


def rules_sequence():
    """the two-pose scene's hypotheses for the selection rules and the model's answer"""
    if "rules" not in _cache:
        T = Cs.two_poses()
        quads = [T["quad_junk"], T["quads_b"][0], T["quads_b"][1], T["quad_a"]]
        _cache["rules"] = (T, quads, model(T["corr"], quads, T["mi"]))
    return _cache["rules"]


def check_conditions():
    """what the generator must provide, so that no test passes by emptiness"""
    refined = exhausted = never = several = 0
    bad = total = 0
    answers = [case(name)[3] for name in Cs.ALL_NAMES] + [rules_sequence()[2]]
    mins = [case(name)[2] for name in Cs.ALL_NAMES] + [rules_sequence()[0]["mi"]]
    for m, mi in zip(answers, mins):
        refined += m["returned"] >= 0
        exhausted += m["returned"] < 0 and m["best"] >= 0
        never += int((m["hyp_count"] >= mi).sum()) == 0
        several += len(m["ref_hyp"]) > 1
        bad += int((~(np.isfinite(m["hyp_R"]).all(axis=(1, 2)) & np.isfinite(m["hyp_t"]).all(axis=1))).sum())
        total += len(m["hyp_count"])
    for name in Cs.REFINE_NAMES:                                                # the cases of check_refine_case count too, under the same cap
        m = refine_case(name)[3]
        bad += int((~(np.isfinite(m["hyp_R"]).all(axis=(1, 2)) & np.isfinite(m["hyp_t"]).all(axis=1))).sum())
        total += len(m["hyp_count"])
    print(f"{bad} non-finite hypotheses of {total}")
    assert refined >= 1 and exhausted >= 1 and never >= 1 and several >= 1, (refined, exhausted, never, several)
    assert bad < 0.05 * total, (bad, total)


# ------------------------------------------------------------------------------------------------ dedicated cases
def check_strict_threshold(library):
    """error2 < mvMaxError[i] is strict and in float: a point whose max_error equals its error2 exactly is an outlier, one ulp more makes it an inlier"""
    corr, quads, mi, m = case("n20_h5")
    corr = corr.copy()
    R, t = m["hyp_R"][0], m["hyp_t"][0]
    e2 = M.reprojection_error2(R, t, Cs.K, corr)
    i, j = [int(k) for k in np.flatnonzero(np.isfinite(e2) & (e2 > 0))[:2]]
    corr[i, 5], corr[j, 5] = e2[i], np.nextafter(e2[j], f32(np.inf))
    mm = model(corr, quads[:1], mi)
    assert not (mm["hyp_mask"][0, i >> 6] >> np.uint64(i & 63)) & np.uint64(1) and (mm["hyp_mask"][0, j >> 6] >> np.uint64(j & 63)) & np.uint64(1)
    d = device(corr, quads[:1], mi, library=library)
    assert differences(d, mm) == []


def check_select_rules(library):
    """count == min refines; a refined count == min fails; a count tied with the best does not replace it but refines the standing mask again (the same
    refine: it fails again); a refine fails and a later one succeeds"""
    T, quads, m = rules_sequence()
    mi = T["mi"]
    assert list(m["hyp_count"][:3]) == [m["hyp_count"][0], mi, mi] and m["hyp_count"][0] < mi < m["hyp_count"][3]
    assert list(m["ref_hyp"]) == [1, 3] and m["ref_count"][0] == mi and m["ref_count"][1] > mi, (m["ref_hyp"], m["ref_count"])
    assert (m["n_consumed"], m["returned"], m["best"]) == (4, 3, 3)
    d = device(T["corr"], quads, mi, library=library)
    assert differences(d, m) == []
    # without the last hypothesis the loop ends on the unrefined best: the first of the two equals
    m2 = model(T["corr"], quads[:3], mi)
    assert (m2["n_consumed"], m2["returned"], m2["best"], m2["best_inliers_out"]) == (3, -1, 1, mi) and list(m2["ref_hyp"]) == [1]
    d2 = device(T["corr"], quads[:3], mi, library=library)
    assert differences(d2, m2) == [] and d2["refined_Tcw"] is None
    assert np.array_equal(d2["best_mask"], T["is_b"])


def check_carried_in(library):
    """mnBestInliers and mvbBestInliers carried in from an earlier call: a hypothesis that reaches the minimum without exceeding them refines the
    carried-in mask, before any new maximum"""
    T, quads, _ = rules_sequence()
    mi = T["mi"]
    first = model(T["corr"], quads[1:2], mi)
    assert first["best"] == 0 and first["returned"] == -1
    later = [quads[0], quads[2], quads[3]]
    m = model(T["corr"], later, mi, first["best_inliers_out"], first["best_mask"])
    assert list(m["ref_hyp"]) == [-1, 2] and (m["returned"], m["best"]) == (2, 2)
    d = device(T["corr"], later, mi, first["best_inliers_out"], first["best_mask"], library=library)
    assert differences(d, m) == []
    m = model(T["corr"], later[:2], mi, first["best_inliers_out"], first["best_mask"])
    assert list(m["ref_hyp"]) == [-1] and (m["returned"], m["best"], m["best_inliers_out"]) == (-1, -1, mi)
    d = device(T["corr"], later[:2], mi, first["best_inliers_out"], first["best_mask"], library=library)
    assert differences(d, m) == [] and d["best_Tcw"] is None and d["best_mask"] is None


def check_behind_camera(library):
    """CheckInliers has no test for positive depth: the mirror image of a point through the camera centre projects to the same pixel and counts"""
    T, quads, m = rules_sequence()
    corr = T["corr"].copy()
    R, t = m["hyp_R"][3], m["hyp_t"][3]                                         # pose A, from the model
    i = int(np.flatnonzero(T["is_a"])[-1])
    Pc = R @ corr[i, 0:3].astype(np.float64) + t
    corr[i, 0:3] = (R.T @ (-Pc - t)).astype(f32)
    mm = model(corr, quads[3:4], T["mi"])
    assert (R[2] @ corr[i, 0:3].astype(np.float64) + t[2]) < 0 and (mm["hyp_mask"][0, i >> 6] >> np.uint64(i & 63)) & np.uint64(1)
    d = device(corr, quads[3:4], T["mi"], library=library)
    assert differences(d, mm) == []


def check_degenerate(library):
    """coincident and collinear minimal sets: a non-finite pose, no inliers, and every loop still ends"""
    corr, _, mi, _ = case("n20_h5")
    corr = corr.copy()
    corr[0:4, 0:3] = corr[0, 0:3]
    for k in range(4):
        corr[4 + k, 0:3] = np.array([0.5 * k, 1.0 * k, 4.0 + 0.25 * k], f32)
    quads = [[0, 1, 2, 3], [4, 5, 6, 7], [3, 2, 1, 0]]
    m = model(corr, quads, mi)
    assert (~np.isfinite(m["hyp_R"]).all(axis=(1, 2))).all() and list(m["hyp_count"]) == [0, 0, 0] and m["best"] == -1
    d = device(corr, quads, mi, library=library)
    assert differences(d, m) == []


def check_refused_inputs(library):
    corr, quads, mi, _ = case("n20_h5")
    for bad in ([[0, 1, 2, 20]], [[0, 1, 2, -1]], [[0, 1, 2, 1]], np.zeros((4097, 4), np.int32) + np.arange(4, dtype=np.int32)):
        with pytest.raises(OH.OrbHipError):
            device(corr, bad, mi, library=library)
    with pytest.raises(OH.OrbHipError):
        device(corr, quads, mi, best_in=12, best_mask_in=None, library=library)
    # nothing is computed: the record of a refused call keeps what it held
    rec = (OH._PnpProblem * 1)()
    keep = OH._pnp_fill(rec[0], dict(K=Cs.K, corr=corr, quads=[[0, 1, 2, 2]], min_inliers=mi), True)
    rec[0].n_consumed, rec[0].returned, rec[0].best = 77, 78, 79
    L = OH.lib(library)
    assert L.orbhip_pnp_iterate(0, C.cast(rec, C.c_void_p)) != 0
    assert (rec[0].n_consumed, rec[0].returned, rec[0].best) == (77, 78, 79) and not keep["hyp_count"].any()


def check_short_untouched(library):
    """n < 4 and n < min_inliers: answered at once, nothing else written"""
    corr, quads, mi, _ = case("n20_h5")
    for c, q, m_in in ((corr[:3], [[0, 1, 2, 0]], 2), (corr[:8], [[0, 1, 2, 3]], 9), (corr, np.zeros((0, 4), np.int32), mi)):
        rec = (OH._PnpProblem * 1)()
        keep = OH._pnp_fill(rec[0], dict(K=Cs.K, corr=c, quads=q, min_inliers=m_in), True)
        rec[0].n_consumed, rec[0].best_inliers_out, rec[0].refined_inliers, rec[0].n_ref = 7, 7, 7, 7
        rec[0].best_Tcw[0] = 5.0
        keep["best_mask"][:] = 3
        assert OH.lib(library).orbhip_pnp_iterate(0, C.cast(rec, C.c_void_p)) == 0
        assert (rec[0].n_consumed, rec[0].returned, rec[0].best) == (0, -1, -1)
        assert (rec[0].best_inliers_out, rec[0].refined_inliers, rec[0].n_ref, rec[0].best_Tcw[0]) == (7, 7, 7, 5.0) and (keep["best_mask"] == 3).all()


def _batch_problems():
    T, quads, _ = rules_sequence()
    first = model(T["corr"], quads[1:2], T["mi"])
    out = []
    for name in ("n63_h5", "n129_h5"):
        corr, q, mi, m = case(name)
        out.append((dict(K=Cs.K, corr=corr, quads=q, min_inliers=mi), m))
    corr = case("n20_h5")[0]
    out.insert(1, (dict(K=Cs.K, corr=corr[:3], quads=[[0, 1, 2, 0]], min_inliers=2), M.iterate(Cs.K, corr[:3], [[0, 1, 2, 0]], 2)))
    later = [quads[0], quads[2], quads[3]]
    out.append((dict(K=Cs.K, corr=T["corr"], quads=later, min_inliers=T["mi"], best_in=first["best_inliers_out"], best_mask_in=first["best_mask"]),
                model(T["corr"], later, T["mi"], first["best_inliers_out"], first["best_mask"])))
    corr, q, mi, m = case("n5_h5")
    out.append((dict(K=Cs.K, corr=corr, quads=q, min_inliers=mi), m))
    return out


def check_batch_slots(library):
    """mixed sizes, one slot answered at once, one with carried-in state: every slot gives the single call's bits, in either order"""
    probs = _batch_problems()
    for order in (list(range(len(probs))), list(range(len(probs)))[::-1]):
        res = orb_slam2_amd.pnp_iterate_batch([probs[k][0] for k in order], per_hypothesis=True, library=library)
        for k, d in zip(order, res):
            m = probs[k][1]
            if m["n_consumed"] == 0 and m["best_inliers_out"] is None:
                assert (d["n_consumed"], d["returned"], d["best"]) == (0, -1, -1)
            else:
                assert differences(d, m) == [], (order, k)


def check_repeat(library):
    corr, quads, mi, m = case("n64_h5")
    for _ in range(2):
        assert differences(device(corr, quads, mi, library=library), m) == []


def check_three_threads(library):
    names = ("n63_h5", "n64_h5", "n129_h5")
    for n in names:
        case(n)
    bad = []

    def work(name):
        try:
            corr, quads, mi, m = case(name)
            for _ in range(3):
                if differences(device(corr, quads, mi, library=library), m):
                    bad.append(name)
            OH.lib(library).orbhip_thread_release()
        except Exception as e:                                                  # noqa: BLE001 - reported below
            bad.append((name, repr(e)))

    threads = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert bad == []


class _Rand:
    """a stand-in for DUtils::Random::RandomInt: a fixed stream"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def __call__(self, lo, hi):
        return int(self.rng.integers(lo, hi + 1))


class DeviceSolver(M.Solver):
    library = None

    def solve(self, quads):
        return orb_slam2_amd.pnp_iterate(self.K, self.corr, quads, self.min_inliers, self.best_inliers, self.best_mask, library=self.library)


def check_solver_rounds(library):
    """the class's rounds over several iterate(5) with the draw queue: the device-backed solver and the model's walk through the same states"""
    for name, rounds in (("n63_h5", 3), ("n129_h5", 2)):
        corr = case(name)[0]
        a, b = M.Solver(Cs.K, corr, _Rand(3)), DeviceSolver(Cs.K, corr, _Rand(3))
        b.library = library
        for s in (a, b):
            s.set_ransac_parameters(0.99, 10, 12, 4, 0.5)
        for r in range(rounds):
            ra, rb = a.iterate(5), b.iterate(5)
            assert same_bits(ra[0], rb[0]) and ra[1] == rb[1] and np.array_equal(ra[2], rb[2]) and ra[3] == rb[3], (name, r)
            assert (a.iterations, a.queue, a.best_inliers) == (b.iterations, b.queue, b.best_inliers), (name, r)


def check_jacobi_forms(library):
    """emulation only: the cooperative form of the Jacobi routine, the serial template and the model give equal bits on the graded cases' M^T M"""
    L = OH.lib(library)
    L.orbhip_test_jacobi12.argtypes = [C.c_void_p, C.c_void_p]
    L.orbhip_test_jacobi12.restype = None
    mats = []
    for name in ("n20_h5", "n64_h5"):
        corr, quads, _, _ = case(name)
        with np.errstate(all="ignore"):
            mats += [M.epnp_front(M.Set(corr, q), Cs.K)["MtM"] for q in quads[:3]]
            mats.append(M.epnp_front(M.Set(corr, mask=np.ones(len(corr), bool)), Cs.K)["MtM"])
    mats.append(np.diag(np.arange(12.0)))
    w, V = M.jacobi_batch(np.array(mats))
    for k, A in enumerate(mats):
        A = np.ascontiguousarray(A, np.float64)
        out = np.zeros((4, 12, 12))
        L.orbhip_test_jacobi12(A.ctypes.data, out.ctypes.data)
        assert same_bits(np.diag(out[0]).copy(), np.diag(out[2]).copy()) and same_bits(out[1], out[3]), k
        assert same_bits(np.diag(out[0]).copy(), w[k]) and same_bits(out[1], V[k]), k


# ------------------------------------------------------------------------------------------------ refines past one mask word, planar refines
def refine_case(name):
    """(corr, quads, min_inliers, the model's answer, the arms the model took: trace["hyp"] and trace["ref"]) of one of Cs.REFINE_NAMES"""
    key = ("refine", name)
    if key not in _cache:
        corr, quads, mi, _, _ = Cs.refine_case(name)
        trace = {}
        m = M.iterate(Cs.K, corr, quads, mi, trace=trace)
        for a in [corr, quads] + [v for v in m.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _cache[key] = (corr, quads, mi, m, trace)
    return _cache[key]


def _lowest_bit(words):
    nz = np.flatnonzero(words)
    return 64 * int(nz[0]) + (int(words[nz[0]]) & -int(words[nz[0]])).bit_length() - 1 if len(nz) else -1


def check_refine_case(name, library):
    """k_pnp_refine where the graded cases never take it: masks of 3, 5, 16 and 65 words with set bits in every word (the masked sum's stride past two
    passes, the popcount loop's second pass), a mask whose first set bit is in its second word, and planar sets in a refine: rank 2 with a finite pose,
    det < 0, the clamped eigenvalue.  What each case must provide is asserted from the model first."""
    corr, quads, mi, m, trace = refine_case(name)
    words, ref = (len(corr) + 63) // 64, trace["ref"]
    src = [m["hyp_mask"][h] for h in m["ref_hyp"] if h >= 0]                    # the masks the refines ran over
    assert len(m["ref_hyp"]) >= 1 and len(src) == len(m["ref_hyp"]) and ref.get("words_%d" % words, 0) == len(src), (name, m["ref_hyp"], ref)
    if name.startswith("refine_n"):
        assert m["returned"] >= 0 and all((s != 0).all() for s in src), (name, m["returned"], src)
        assert words == {"refine_n129": 3, "refine_n300": 5, "refine_n1000": 16, "refine_n4160": 65}[name]
    elif name == "refine_first_in_word1":
        assert all(s[0] == 0 and _lowest_bit(s) >= 64 for s in src) and ref.get("first_ge_64", 0) == len(src) and m["returned"] >= 0, (name, src)
    elif name == "planar_exact":
        # ABt of a refine has rank 2 and the pose is finite; the clamp is met by minimal sets only (their poses are the non-finite ones)
        assert m["returned"] >= 0 and ref.get("rank2_finite", 0) >= 1 and np.isfinite(m["ref_R"]).all() and np.isfinite(m["ref_t"]).all(), (name, ref)
        assert trace["hyp"].get("dc_clamp", 0) >= 1 and trace["hyp"].get("rank2_finite", 0) >= 1, (name, trace["hyp"])
    elif name == "planar_failing_refines":
        assert len(src) >= 2 and (m["ref_count"] <= mi).all() and m["returned"] == -1 and m["best"] >= 0 and ref.get("det_negative", 0) >= 1, (name, m["ref_count"], ref)
    elif name == "planar_lattice":
        # the clamp inside a refine: CC is singular, the refined pose not finite, the refine fails with no inlier
        assert ref.get("dc_clamp", 0) >= 1 and np.isnan(m["ref_R"]).all() and np.isnan(m["ref_t"]).all() and (m["ref_count"] == 0).all() and m["returned"] == -1 and m["best"] >= 0, (name, ref)
    d = device(corr, quads, mi, library=library)
    print(f"{name}: n {len(corr)}, {words} words, {len(quads)} hypotheses, min {mi}, returned {d['returned']}, best {d['best']}, refines of {[int(h) for h in d['ref_hyp']]}: "
          f"{[int(np.unpackbits(s.view(np.uint8)).sum()) for s in src]} -> {[int(c) for c in d['ref_count']]} inliers; arms in the refines {ref}")
    assert differences(d, m) == [], name


def sign_first():
    """the two-pose scene with pose A's lowest point mirrored through the camera centre of the hypothesis, and the same with that point and the next
    swapped: (i, corr, quad, model answer, corr swapped, quad swapped, model answer)"""
    if "sign_first" not in _cache:
        T = Cs.two_poses()
        quad, mi = list(T["quad_a"]), T["mi"]
        i = int(np.flatnonzero(T["is_a"])[0])
        assert i not in quad and i + 1 < len(T["corr"]) and T["is_a"][i + 1]
        m0 = model(T["corr"], [quad], mi)
        R, t = m0["hyp_R"][0], m0["hyp_t"][0]
        corr = T["corr"].copy()
        Pc = R @ corr[i, 0:3].astype(np.float64) + t
        corr[i, 0:3] = (R.T @ (-Pc - t)).astype(f32)
        swapped = corr.copy()
        swapped[[i, i + 1]] = corr[[i + 1, i]]
        quad_s = [i if q == i + 1 else q for q in quad]
        tr, tr_s = {}, {}
        m, ms = M.iterate(Cs.K, corr, [quad], mi, trace=tr), M.iterate(Cs.K, swapped, [quad_s], mi, trace=tr_s)
        _cache["sign_first"] = (i, corr, quad, m, tr, swapped, quad_s, ms, tr_s)
    return _cache["sign_first"]


def check_sign_first(library):
    """solve_for_sign reads the FIRST point of the set only.  The first set bit of the refined mask is a point behind the camera: the refine flips the
    sign and finds no inlier; with that point second, the same set refines well.  A kernel that took any other set bit as `first` fails one of the two."""
    i, corr, quad, m, tr, swapped, quad_s, ms, tr_s = sign_first()
    mi = Cs.two_poses()["mi"]
    assert _lowest_bit(m["hyp_mask"][0]) == i and _lowest_bit(ms["hyp_mask"][0]) == i and (int(ms["hyp_mask"][0][0]) >> (i + 1)) & 1
    assert list(m["ref_hyp"]) == [0] and list(ms["ref_hyp"]) == [0] and m["ref_count"][0] != ms["ref_count"][0], (m["ref_count"], ms["ref_count"])
    assert tr["ref"].get("sign_depends_on_first", 0) >= 1 and tr_s["ref"].get("sign_depends_on_first", 0) >= 1, (tr["ref"], tr_s["ref"])
    assert (m["returned"] >= 0) != (ms["returned"] >= 0), (m["returned"], ms["returned"])
    print(f"first set bit {i}: mirrored point first: refined {m['ref_count'][0]}, returned {m['returned']}; second: refined {ms['ref_count'][0]}, returned {ms['returned']} (min {mi})")
    assert differences(device(corr, [quad], mi, library=library), m) == []
    assert differences(device(swapped, [quad_s], mi, library=library), ms) == []


PASS_SEQUENCES = ("lane63_then_lane0", "tie_in_pass1", "carried_in_pass1_then_new", "new_before_carried", "carried_never_reached", "returns_on_carried_in_pass1")


def pass_sequence(name):
    """a hypothesis sequence of the two-pose scene longer than one 64-lane pass of k_pnp_select: (quads, best_in, best_mask_in, the model's answer, the
    bookkeeping the model must show)"""
    key = ("pass", name)
    if key not in _cache:
        T = Cs.two_poses()
        J, B0, B1, A, mi = T["quad_junk"], T["quads_b"][0], T["quads_b"][1], T["quad_a"], T["mi"]
        if "first" not in _cache:
            _cache["first"] = model(T["corr"], [B0], mi)                        # a call that ended on B's unrefined mask: count mi
            _cache["after"] = model(T["corr"], [A], mi)                         # a call that returned on A: A's count and mask stay in the solver
        first, after = _cache["first"], _cache["after"]
        assert first["best"] == 0 and first["returned"] == -1 and first["best_inliers_out"] == mi
        assert after["returned"] == 0 and after["best"] == 0 and after["best_inliers_out"] > mi
        quads, carried, want = {
            # a new maximum at lane 63 whose refine fails (count == min), the next at lane 0 of pass 1
            "lane63_then_lane0": ([J] * 63 + [B0, A], None, dict(ref_hyp=[63, 64], returned=64, n_consumed=65, best=64)),
            # a tie in pass 1 refines the standing mask again and adds no candidate
            "tie_in_pass1": ([J] * 10 + [B0] + [J] * 60 + [B1] + [J] * 5, None, dict(ref_hyp=[10], returned=-1, n_consumed=77, best=10)),
            # the carried-in mask first met in pass 1, a new maximum in pass 2
            "carried_in_pass1_then_new": ([J] * 70 + [B1] + [J] * 59 + [A] + [J] * 3, first, dict(ref_hyp=[-1, 130], returned=130, n_consumed=131, best=130)),
            # a new maximum comes first: the carried-in mask is never refined
            "new_before_carried": ([J] * 130 + [A, B1], first, dict(ref_hyp=[130], returned=130, n_consumed=131, best=130)),
            "carried_never_reached": ([J] * 65, first, dict(ref_hyp=[], returned=-1, n_consumed=65, best=-1, best_inliers_out=mi)),
            # the carried-in mask first met in pass 1 and its refine succeeds: the call returns at cand_at[0], which none of the others reads
            "returns_on_carried_in_pass1": ([J] * 70 + [A] + [J] * 3, after, dict(ref_hyp=[-1], returned=70, n_consumed=71, best=-1)),
        }[name]
        best_in, mask_in = (0, None) if carried is None else (carried["best_inliers_out"], carried["best_mask"])
        _cache[key] = (quads, best_in, mask_in, model(T["corr"], quads, mi, best_in, mask_in), want)
    return _cache[key]


def check_select_passes(name, library):
    """k_pnp_select past its first 64 hypotheses (PASS_SEQUENCES): the model's bookkeeping is asserted first, then the device must give the model's bits"""
    T = Cs.two_poses()
    quads, best_in, mask_in, m, want = pass_sequence(name)
    assert len(quads) > 64 and all(list(m[k]) == want[k] if k == "ref_hyp" else m[k] == want[k] for k in want), ({k: m[k] for k in want}, want)
    if name == "tie_in_pass1":
        assert (m["hyp_count"][[10, 71]] == T["mi"]).all()
    d = device(T["corr"], quads, T["mi"], best_in, mask_in, library=library)
    assert differences(d, m) == [], name
    if name == "carried_never_reached":
        assert d["best_Tcw"] is None and d["best_mask"] is None and len(d["ref_hyp"]) == 0


def _raw_call(library, problem, change):
    """orbhip_pnp_iterate on a record filled by OH._pnp_fill and then changed by change(rec, keep): (rec, keep)"""
    rec = (OH._PnpProblem * 1)()
    keep = OH._pnp_fill(rec[0], problem, True)
    change(rec[0], keep)
    assert OH.lib(library).orbhip_pnp_iterate(0, C.cast(rec, C.c_void_p)) == 0
    return rec[0], keep


REF_KEYS = ("ref_hyp", "ref_R", "ref_t", "ref_count", "ref_mask")


def check_ref_cap(library):
    """a caller with room for fewer refine records than the loop made: n_ref says how many there were, only ref_cap rows are written"""
    T, quads, m = rules_sequence()
    assert len(m["ref_hyp"]) == 2
    fill = dict(ref_hyp=-7, ref_R=7.5, ref_t=7.5, ref_count=-7, ref_mask=0x7777777777777777)

    def change(rec, keep):
        rec.ref_cap = 1
        for k in REF_KEYS:
            keep[k][...] = fill[k]

    rec, keep = _raw_call(library, dict(K=Cs.K, corr=T["corr"], quads=quads, min_inliers=T["mi"]), change)
    assert rec.n_ref == 2
    for k in REF_KEYS:
        assert same_bits(keep[k][0], np.asarray(m[k][0])), k
        assert (keep[k][1:] == fill[k]).all(), k
    d = OH._pnp_result(rec, keep)
    assert differences(d, {k: v for k, v in m.items() if k not in REF_KEYS}) == []


def check_hyp_count_alone(library):
    """a caller that asks for the counts of the hypotheses and not for their poses or masks"""
    T, quads, m = rules_sequence()

    def change(rec, keep):
        rec.hyp_R, rec.hyp_t, rec.hyp_mask = None, None, None
        keep["hyp_R"][...], keep["hyp_t"][...], keep["hyp_mask"][...] = 7.5, 7.5, 0x7777777777777777

    rec, keep = _raw_call(library, dict(K=Cs.K, corr=T["corr"], quads=quads, min_inliers=T["mi"]), change)
    assert (keep["hyp_R"] == 7.5).all() and (keep["hyp_t"] == 7.5).all() and (keep["hyp_mask"] == 0x7777777777777777).all()
    assert np.array_equal(keep["hyp_count"], m["hyp_count"])
    d = OH._pnp_result(rec, keep)
    assert differences(d, {k: v for k, v in m.items() if k not in ("hyp_R", "hyp_t", "hyp_mask")}) == []


def check_batch_refines(library):
    """the new problems in one call, in both orders: different hypothesis counts, candidate counts and mask words, so that surplus blocks of k_pnp_hyp and
    k_pnp_refine return early; every slot gives its single call's bits"""
    T = Cs.two_poses()
    probs = []
    for name in ("refine_n129", "planar_exact", "refine_first_in_word1", "planar_lattice"):
        corr, q, mi, m, _ = refine_case(name)
        probs.append((dict(K=Cs.K, corr=corr, quads=q, min_inliers=mi), m))
    quads, best_in, mask_in, m, _ = pass_sequence("carried_in_pass1_then_new")
    probs.insert(3, (dict(K=Cs.K, corr=T["corr"], quads=quads, min_inliers=T["mi"], best_in=best_in, best_mask_in=mask_in), m))
    _, corr, quad, m = sign_first()[:4]
    probs.append((dict(K=Cs.K, corr=corr, quads=[quad], min_inliers=T["mi"]), m))
    assert len({len(p[0]["quads"]) for p in probs}) >= 4 and len({len(p[1]["ref_hyp"]) for p in probs}) >= 2 and len({p[1]["hyp_mask"].shape[1] for p in probs}) >= 3
    for order in (list(range(len(probs))), list(range(len(probs)))[::-1]):
        res = orb_slam2_amd.pnp_iterate_batch([probs[k][0] for k in order], per_hypothesis=True, library=library)
        for k, d in zip(order, res):
            assert differences(d, probs[k][1]) == [], (order, k)


# ------------------------------------------------------------------------------------------------ the C++ drop-in
def build_cpp(tmp, library, sanitize=False):
    """tests/pnp_cpp/main.cc + orb_slam2_amd/cpp/PnPsolver.cc as a stand-alone program linked to `library`, in the directory tmp"""
    d, f = os.path.split(os.path.abspath(library))
    exe = os.path.join(str(tmp), "pnp_cpp_asan" if sanitize else "pnp_cpp")
    cmd = ["g++", "-std=c++14", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-DCVLITE_ALGEBRA", "-DORBHIP_USE_OPENCV"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    cmd += ["-I" + os.path.join(ROOT, "tests", "pnp_cpp"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "cvlite"),
            os.path.join(ROOT, "tests", "pnp_cpp", "main.cc"), os.path.join(ROOT, "orb_slam2_amd", "cpp", "PnPsolver.cc"),
            "-o", exe, "-L" + d, "-l" + f[3:-3], "-Wl,-rpath," + d]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpp(exe, env=None, split=False):
    """the program: the class equal to the C ABI (iterate rounds, find, the unrefined end, IterateBatch; with `split` a call above 4096 hypotheses),
    its SetRansacParameters equal to the model's"""
    r = subprocess.run([exe] + (["split"] if split else []), capture_output=True, text=True, timeout=300, env=dict(os.environ if env is None else env))
    assert r.returncode == 0 and "pnp_cpp ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout.splitlines()[-1])
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("params ")]
    assert len(rows) == 13, r.stdout
    for _, n, m, its, eps, _, got_min, got_its in rows:
        want = M.ransac_parameters(int(n), 0.99, int(m), int(its), 4, f32(float(eps)))
        assert want[:2] == (int(got_min), int(got_its)), (n, m, its, eps, got_min, got_its, want)
    if split:
        assert "2 device calls in the split run" in r.stdout
