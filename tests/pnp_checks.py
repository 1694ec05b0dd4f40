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
