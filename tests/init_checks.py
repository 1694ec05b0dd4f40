"""The checks tests/test_init_emu.py (CPU emulation of the kernels) and tests/test_init_gpu.py (the device) share: orbhip_init_reconstruct and its batch
form against tests/init_model.py on the scenes of tests/init_cases.py.

There is no tolerance between kernel and model: DESIGN.md H19 needs +, -, *, / and sqrt only, every one correctly rounded on both sides, and the one
acos is the host's on both sides, so every hypothesis record, every motion-hypothesis record and the whole answer must be equal bit for bit.  One
allowance, which is not a tolerance: two NaNs are equal whatever their sign and payload, a NaN and a number are not."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import orb_slam2_amd
from orb_slam2_amd import orbhip as OH
import init_cases as Cs
import init_model as M
from pnp_checks import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_cache = {}
HEAD = ("returned", "model", "best_h", "best_f", "n_mot", "best_mot")
ARRAYS = ("SH", "SF", "H21", "F21", "R21", "t21", "mot_cos", "mot_good", "mask_h", "mask_f", "p3d", "triangulated", "hyp_score", "hyp_M", "mot_R", "mot_t")


def differences(dv, m):
    """the names in which a device answer differs from the model's"""
    bad = [k for k in HEAD if dv[k] != m[k]]
    return bad + [k for k in ARRAYS if not same_bits(np.asarray(dv[k]) if dv[k] is not None else None, np.asarray(m[k]) if m[k] is not None else None)]


def model(args, trace=None):
    return M.reconstruct(trace=trace, **args)


def device(args, library=None):
    return orb_slam2_amd.init_reconstruct(per_hypothesis=True, library=library, **args)


def case(name):
    """(arguments, the model's answer, the arms the model took): computed once, shared, never changed"""
    if name not in _cache:
        args, trace = Cs.arguments(Cs.case(name)), {}
        m = model(args, trace)
        for a in [v for v in m.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _cache[name] = (args, m, trace)
    return _cache[name]


# the arms each named case must take, asserted from the model before the library is called (no test passes by emptiness)
ARMS = {
    "general_300": ("model_F", "F_arm_1_returns"), "plane_300": ("model_H", "H_returns"), "fronto_300": ("model_H", "H_early"),
    "rotation_300": ("model_H", "H_reject_parallax", "H_fails"), "outliers40_300": ("model_F",), "behind_300": ("model_F", "F_reject_mingood", "det_flip"),
    "similar_80": ("model_F", "F_reject_nsimilar"), "lowpar_80": ("model_F", "F_arm_2_fails_parallax"),
    "general_mode1": ("model_F", "F_arm_3_returns", "det_flip", "stat_index_0"), "plane_mode1": ("model_H", "H_returns"),
    "good52": ("stat_index_50",), "good51": ("stat_index_50",), "good50": ("stat_index_49",),
}


def check_case(name, library):
    args, m, trace = case(name)
    for arm in ARMS.get(name, ()):
        assert trace.get(arm, 0) >= 1, (name, arm, trace)
    dv = device(args, library=library)
    n, ns = len(args["matches"]), len(args["sets"])
    hyp_equal = sum(same_bits(dv["hyp_M"][k, h], m["hyp_M"][k, h]) and same_bits(dv["hyp_score"][k, h], m["hyp_score"][k, h]) for k in range(2) for h in range(ns))
    print(f"{name}: n {n}, {ns} sets, returned {dv['returned']}, model {dv['model']}, SH {dv['SH']:.1f}, SF {dv['SF']:.1f}, nGood {list(dv['mot_good'][:max(dv['n_mot'], 0)])}, "
          f"ends on {dv['best_mot']}, {int(dv['triangulated'].sum())} triangulated, hypotheses with the model's bits: {hyp_equal} of {2 * ns}")
    assert differences(dv, m) == [], name


def check_conditions():
    """what the generator must provide"""
    from_h = from_f = parallax = similar = early = bad = total = 0
    for name in Cs.ALL_NAMES:
        _, m, tr = case(name)
        from_h += m["returned"] == 1 and m["model"] == 0
        from_f += m["returned"] == 1 and m["model"] == 1
        parallax += tr.get("H_reject_parallax", 0) + sum(v for k, v in tr.items() if k.endswith("fails_parallax"))
        similar += tr.get("F_reject_nsimilar", 0) >= 1 and tr.get("F_reject_mingood", 0) == 0
        early += tr.get("H_early", 0)
        bad += int((~(np.isfinite(m["hyp_M"]).all(axis=(2, 3)) & np.isfinite(m["hyp_score"]))).sum())
        total += m["hyp_score"].size
    print(f"{bad} non-finite hypotheses of {total}; from H {from_h}, from F {from_f}, parallax {parallax}, nsimilar {similar}, early {early}")
    assert from_h >= 1 and from_f >= 1 and parallax >= 1 and similar >= 1 and early >= 1, (from_h, from_f, parallax, similar, early)
    assert bad < 0.05 * total, (bad, total)


# ------------------------------------------------------------------------------------------------ dedicated cases
def with_matches(args, matches, **kw):
    a = dict(args)
    a["matches"] = np.ascontiguousarray(matches, f32)
    a.update(kw)
    return a


def check_strict_thresholds(library):
    """`chiSquare > th` is strict and in float: a match whose larger chi-square equals 5.991f (H) or 3.841f (F) exactly is an inlier, one float step
    above an outlier.  One set only, so the hypothesis is fixed whatever sigma is; chi = squareDist * invSigmaSquare, so sigma is walked float by float
    around sqrt(squareDist / th) of the match nearest the threshold until the model's own product lands on th, and on the float above it.  (Moving the
    match instead cannot reach a given float: its squareDist comes out of a cancellation and steps far wider than chi's spacing.)"""
    args, m, _ = case("general_300")
    one = f32(1.0)
    for k, th, best in ((1, f32(3.841), m["best_f"]), (0, f32(5.991), m["best_h"])):
        a = dict(args, sets=args["sets"][best:best + 1])
        Mx = m["hyp_M"][k, best]
        with np.errstate(all="ignore"):
            chi = (lambda G, invS: np.maximum(*M.chi_f(Mx, G, invS))) if k else (lambda G, invS: np.maximum(*M.chi_h(Mx, M.inv3(Mx), G, invS)))
            sq = chi(args["matches"], one)
            sq[args["sets"][best]] = np.inf
            found = {}
            for i in np.argsort(np.abs(sq - th))[:40]:                          # the matches nearest the threshold at sigma = 1, outside the set
                s = f32(np.sqrt(np.float64(sq[i]) / np.float64(th)))
                for _ in range(100):
                    s = np.nextafter(s, f32(0))
                for _ in range(200):
                    c = chi(args["matches"][i:i + 1], M.inv_sigma_square(s))[0]
                    if c == th:
                        found.setdefault(True, (int(i), s))
                    elif c == np.nextafter(th, f32(np.inf)):
                        found.setdefault(False, (int(i), s))
                    s = np.nextafter(s, f32(np.inf))
                if len(found) == 2:
                    break
        assert set(found) == {True, False}, (k, found)
        for inlier, (i, s) in found.items():
            a2 = dict(a, sigma=float(s))
            mm = model(a2)
            assert same_bits(mm["hyp_M"][k, 0], Mx) and mm["hyp_score"][k, 0] > 0 and bool((mm["mask_f"] if k else mm["mask_h"])[i]) == inlier, (k, inlier)
            assert differences(device(a2, library=library), mm) == [], (k, inlier)


def check_strict_reprojection(library):
    """`squareError > th2` is strict and in float: a masked match whose larger reprojection error equals th2 = (float)(4.0*sigma*sigma) exactly is counted,
    one float step above th2 it is not.  One set only, so F21 and with it the four (R, t) are fixed whatever sigma is, and so is every match's
    squareError; sigma is walked float by float around sqrt(squareError / 4) until th2 lands on the error of a match, and on the float below it.  The
    match must stay an inlier of F at that sigma (its chi-square scales with 1 / sigma^2): candidates are taken from the model's own figures."""
    args, m, _ = case("general_300")
    a = dict(args, sets=args["sets"][m["best_f"]:m["best_f"] + 1])
    base = model(a)
    assert base["n_mot"] == 4 and same_bits(base["F21"], m["F21"])
    k = int(np.argmax(base["mot_good"]))
    R, t = base["mot_R"][k], base["mot_t"][k]
    n = len(args["matches"])

    def th2_of(s):
        return f32(4.0 * np.float64(f32(s) * f32(s)))

    def sigma_for(target):
        s = f32(np.sqrt(np.float64(target) / 4.0))
        for _ in range(8):
            s = np.nextafter(s, f32(0))
        for _ in range(17):
            if th2_of(s) == target:
                return s
            s = np.nextafter(s, f32(np.inf))
        return None
    with np.errstate(all="ignore"):
        _, _, _, e1, e2 = M.check_rt(R, t, Cs.K, args["matches"], np.ones(n, bool), 1.0, 0, detail=True)
        chi = np.maximum(*M.chi_f(base["F21"], args["matches"], f32(1.0)))
    E = np.maximum(e1, e2)
    for image in (1, 2):                                                        # the comparison of squareError1, then that of squareError2
        decides = e1 > e2 if image == 1 else e2 > e1
        found = None
        for i in np.argsort(-E):
            if decides[i] and np.isfinite(E[i]) and E[i] > 0 and chi[i] / (E[i] / 4) <= 3.8:      # an inlier of F21 at the sigma that puts th2 on its error
                s_at, s_above = sigma_for(E[i]), sigma_for(np.nextafter(E[i], f32(0)))
                if s_at is not None and s_above is not None:
                    found = (int(i), s_at, s_above)
                    break
        assert found is not None, "no masked match whose squareError%d both th2 and the float below can reach" % image
        i, s_at, s_above = found
        print(f"image {image}, match {i}: squareError {E[i]!r}, chi-square at sigma 1 {chi[i]!r}; th2 equals it at sigma {s_at!r}, is one float below it at sigma {s_above!r}")
        for s, counted in ((s_at, True), (s_above, False)):
            a2 = dict(a, sigma=float(s))
            mm = model(a2)
            assert same_bits(mm["F21"], m["F21"]) and same_bits(mm["mot_R"][k], R) and mm["mask_f"][i] and mm["n_mot"] == 4
            with np.errstate(all="ignore"):
                st, _, _, f1, f2 = M.check_rt(R, t, Cs.K, args["matches"], mm["mask_f"], float(s), 0, detail=True)
            assert (f1[i], f2[i]) == (e1[i], e2[i]) and (th2_of(s) == E[i] if counted else np.nextafter(th2_of(s), f32(np.inf)) == E[i])
            assert bool(st[i] & 1) == counted and int((st & 1).sum()) == mm["mot_good"][k], (image, counted, st[i])
            assert differences(device(a2, library=library), mm) == [], (image, counted)


def check_non_finite_triangulation_is_skipped(library):
    """CheckRT skips a match whose triangulation is not finite (:841): without the skip every comparison after it is false for a NaN point and the match
    would be counted.  A calibration whose products overflow a float makes E21, every (R, t) and so every triangulation of a masked match non-finite,
    while the scores - which do not read K - stay as they were: F is chosen with its usual mask and no motion hypothesis counts a single match."""
    args, m, _ = case("n65")
    a = dict(args, K=np.array([3e38, 3e38, 320.0, 240.0], f32))
    mm = model(a)
    assert mm["model"] == 1 and same_bits(mm["mask_f"], m["mask_f"]) and mm["mask_f"].sum() >= 50 and mm["n_mot"] == 4
    fx, fy, cx, cy = a["K"]
    P1 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], f32)
    with np.errstate(all="ignore"):
        for j in range(4):
            q = M.triangulate(a["matches"][mm["mask_f"]], P1, M.projection(a["K"], mm["mot_R"][j], mm["mot_t"][j], 0)[0])
            assert not np.isfinite(q).all(axis=1).any()
    assert not mm["mot_good"].any() and mm["returned"] == 0 and not mm["triangulated"].any()
    assert differences(device(a, library=library), mm) == []


def check_tie_keeps_first(library):
    """two sets with the same eight matches in the same order give the same score: the first stays"""
    args, m, _ = case("general_300")
    sets = args["sets"].copy()
    b = m["best_f"]
    other = (b + 7) % len(sets)
    sets[other] = sets[b]
    a = dict(args, sets=sets)
    mm = model(a)
    assert mm["hyp_score"][1, other] == mm["hyp_score"][1, b] and mm["best_f"] == min(b, other) and mm["best_h"] in (m["best_h"], min(b, other))
    assert differences(device(a, library=library), mm) == []


def check_equal_smallest_eigenvalues_keep_the_first(library):
    """eight matches whose normalised u1 is exactly 0 leave columns 0, 3 and 6 of A - H's and F's - exactly zero: A^T A has three eigenvalues that are
    exactly 0, the Jacobi never touches them, and the smallest is the FIRST of them: the null vector is e0, not e6"""
    rng = np.random.default_rng(9)
    n = 24
    matches = np.stack([rng.uniform(-300, 300, n), rng.uniform(-200, 200, n), rng.uniform(-300, 300, n), rng.uniform(-200, 200, n)], 1).astype(f32)
    matches[:8, 0] = 0.0
    norm = np.array([0.0, 0.0, 1.0 / 128, 1.0 / 128], f32)
    a = dict(K=Cs.K, matches=matches, sets=np.arange(8, dtype=np.int32).reshape(1, 8), norm1=norm, norm2=norm, sigma=1.0, min_parallax=1.0, min_triangulated=50, gemm_mode=0)
    for is_f in (False, True):
        v, A, AtA = M.null_vectors(matches, a["sets"], norm, norm, is_f, with_system=True)
        w, _ = M.jacobi_batch(AtA)
        assert (w[0, [0, 3, 6]] == 0).all() and (np.delete(w[0], [0, 3, 6]) > 0).all() and v[0].tolist() == [1.0] + [0.0] * 8, (is_f, w, v)
    tr = {}
    mm = model(a, tr)
    assert tr["hyp"].get("rank2_degenerate", 0) == 1                            # Fpre = e0 has rank 1: the 3 x 3 decomposition takes its rank-2 arm
    assert differences(device(a, library=library), mm) == []


def check_all_scores_zero(library):
    """no hypothesis of either model scores above 0 (every match is an outlier of every hypothesis): returned 0, model -1"""
    rng = np.random.default_rng(5)
    n = 40
    matches = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n), rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1).astype(f32)
    matches[8:] = matches[8:] * f32(1000)                                       # far from anything the first eight determine
    a = dict(K=Cs.K, matches=matches, sets=np.arange(8, dtype=np.int32).reshape(1, 8), norm1=M.normalize(matches[:, 0:2]), norm2=M.normalize(matches[:, 2:4]),
             sigma=1e-4, min_parallax=1.0, min_triangulated=50, gemm_mode=0)
    mm = model(a)
    assert mm["model"] == -1 and mm["returned"] == 0 and mm["SH"] == 0 and mm["SF"] == 0 and not mm["mask_f"].any(), (mm["SH"], mm["SF"])
    dv = device(a, library=library)
    assert differences(dv, mm) == [] and dv["R21"] is None and dv["t21"] is None


def check_similar_rule_is_strict(library):
    """`nGood > 0.7*maxGood` is strict: with maxGood = 0 no hypothesis is similar (0 > 0 is false), so a call whose minimum is 0 goes on to the chain, whose
    first arm equals maxGood and passes a negative min_parallax with the parallax 0 of an empty hypothesis.  One set, and a sigma between the smallest
    and the second smallest chi-square of the winner, so that N = 1 and 0.9 * N truncates to 0."""
    args, m, _ = case("n65")
    a = dict(args, sets=args["sets"][m["best_f"]:m["best_f"] + 1], min_triangulated=0, min_parallax=-1.0)
    with np.errstate(all="ignore"):
        c = np.sort(np.maximum(*M.chi_f(m["F21"], args["matches"], f32(1.0))))
    a["sigma"] = float(np.sqrt((np.float64(c[0]) + np.float64(c[1])) / 2 / 3.841))
    mm, tr = model(a), {}
    model(a, tr)
    assert mm["model"] == 1 and int(mm["mask_f"].sum()) == 1 and not mm["mot_good"].any(), (mm["model"], int(mm["mask_f"].sum()), mm["mot_good"])
    assert mm["returned"] == 1 and mm["best_mot"] == 0 and tr.get("F_arm_0_returns") == 1 and not mm["triangulated"].any()
    assert differences(device(a, library=library), mm) == []


def check_low_parallax_point_is_kept(library):
    """a point behind a camera with cosParallax >= 0.99998 is counted (nGood, vP3D) and not marked triangulated"""
    args, m, _ = case("farkept_80")
    kept = ~m["triangulated"] & (m["p3d"] != 0).any(axis=1)
    behind = kept & (m["p3d"][:, 2] <= 0)
    print(f"{int(kept.sum())} counted points without parallax, {int(behind.sum())} of them behind the first camera, {int(m['triangulated'].sum())} triangulated")
    assert m["returned"] == 1 and behind.sum() >= 1 and m["triangulated"].sum() >= 1
    assert int(kept.sum()) + int(m["triangulated"].sum()) == m["mot_good"][m["best_mot"]]
    assert differences(device(args, library=library), m) == []


def check_non_finite(library):
    """NaN and Inf coordinates in one match: every launch ends, the call returns, and the answer is the model's"""
    args, m, _ = case("n65")
    for bad in (np.nan, np.inf, -np.inf):
        matches = args["matches"].copy()
        i = int(args["sets"][m["best_f"], 0])                                  # a member of the winning set, and of others
        matches[i, 2] = bad
        a = with_matches(args, matches)
        mm = model(a)
        assert (~np.isfinite(mm["hyp_M"]).all(axis=(2, 3))).any()
        assert differences(device(a, library=library), mm) == [], bad


def check_refused_inputs(library):
    args, m, _ = case("n9")
    bad_sets = args["sets"].copy(); bad_sets[3, 2] = 9
    neg_sets = args["sets"].copy(); neg_sets[0, 0] = -1
    for a in (with_matches(args, args["matches"][:7], sets=np.arange(8).reshape(1, 8) % 7), dict(args, sets=bad_sets), dict(args, sets=neg_sets), dict(args, gemm_mode=2),
              dict(args, gemm_mode=3), dict(args, sets=np.zeros((M.MAX_SETS + 1, 8), np.int32) + np.arange(8, dtype=np.int32)),
              with_matches(args, np.zeros((M.MAX_N + 1, 4), f32))):
        with pytest.raises(OH.OrbHipError):
            device(a, library=library)
    # nothing is written: the record of a refused call keeps what it held
    rec = (OH._InitProblem * 1)()
    keep = OH._init_fill(rec[0], dict(args, sets=bad_sets), True)
    rec[0].returned, rec[0].model, rec[0].best_h = 77, 78, 79
    for k in ("mask_h", "mask_f", "triangulated"):
        keep[k][:] = 5
    L = OH.lib(library)
    assert L.orbhip_init_reconstruct(0, C.cast(rec, C.c_void_p)) == 1
    assert (rec[0].returned, rec[0].model, rec[0].best_h) == (77, 78, 79) and all((keep[k] == 5).all() for k in ("mask_h", "mask_f", "triangulated")) and not keep["hyp_score"].any()
    rec[0].gemm_mode = 2
    keep = OH._init_fill(rec[0], dict(args, gemm_mode=2), False)             # (kept: the record points into these arrays)
    assert L.orbhip_init_reconstruct(0, C.cast(rec, C.c_void_p)) == 4              # ORBHIP_ERR_UNSUPPORTED


BATCH = ("n65", "plane_300", "n9", "general_300", "fronto_300", "rotation_300", "n8", "n64")


def check_batch_slots(library):
    """a batch of mixed sizes - an H problem, an F problem, failing ones - gives every slot the single call's bits, in any order"""
    for order in (BATCH, BATCH[::-1]):
        res = orb_slam2_amd.init_reconstruct_batch([case(nm)[0] for nm in order], per_hypothesis=True, library=library)
        for nm, dv in zip(order, res):
            assert differences(dv, case(nm)[1]) == [], (nm, order)
    kinds = {(case(nm)[1]["model"], case(nm)[1]["returned"]) for nm in BATCH}
    assert (0, 1) in kinds and (1, 1) in kinds and any(r == 0 for _, r in kinds)
    assert orb_slam2_amd.init_reconstruct_batch([], library=library) == []


def check_without_optional_outputs(library):
    args, m, _ = case("n65")
    dv = orb_slam2_amd.init_reconstruct(library=library, **args)
    assert "hyp_M" not in dv and [k for k in HEAD if dv[k] != m[k]] == [] and same_bits(dv["p3d"], m["p3d"]) and same_bits(dv["R21"], m["R21"])


def check_repeat(library):
    args, m, _ = case("general_mode1")
    a, b = device(args, library=library), device(args, library=library)
    assert differences(a, b) == [] and differences(a, m) == []


def check_three_threads(library):
    names, out = ("n65", "plane_mode1", "n63"), {}

    def run(nm):
        out[nm] = [differences(device(case(nm)[0], library=library), case(nm)[1]) for _ in range(3)]
    for nm in names:
        case(nm)
    threads = [threading.Thread(target=run, args=(nm,)) for nm in names]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert out == {nm: [[], [], []] for nm in names}, out


# ------------------------------------------------------------------------------------------------ the C++ drop-in (tests/init_cpp)
# which way each scene ends does not hang on the sets: on the device the runtime takes values of rand() between the calls
CPP_SCENES = ("clean_f", "clean_h", "short_7", "rotation_300", "fronto_300", "behind_300")


def build_cpp(tmp, library, sanitize=False):
    """tests/init_cpp/main.cc + orb_slam2_amd/cpp/Initializer.cc as a stand-alone program linked to `library`, in the directory tmp"""
    dd, f = os.path.split(os.path.abspath(library))
    exe = os.path.join(str(tmp), "init_cpp_asan" if sanitize else "init_cpp")
    cmd = ["g++", "-std=c++14", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-DCVLITE_ALGEBRA", "-DORBHIP_USE_OPENCV"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    cmd += ["-I" + os.path.join(ROOT, "tests", "init_cpp"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "cvlite"),
            os.path.join(ROOT, "tests", "init_cpp", "main.cc"), os.path.join(ROOT, "orb_slam2_amd", "cpp", "Initializer.cc"),
            "-o", exe, "-L" + dd, "-l" + f[3:-3], "-Wl,-rpath," + dd]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def cpp_scene(name, rng):
    """the frames of a case as the class sees them: key points of both frames in shuffled order, unmatched ones in between, vMatches12; and the matches
    in mvMatches12 order (rising index in frame 1) as the C ABI gets them"""
    if name == "short_7":
        c = Cs.case("n9")
        m = c["matches"][:7]
    else:
        c = Cs.case(name)
        m = c["matches"]
    n, extra = len(m), 5 + len(m) // 4
    k1 = np.concatenate([m[:, 0:2], np.stack([rng.uniform(0, Cs.W, extra), rng.uniform(0, Cs.H, extra)], 1).astype(f32)])
    k2 = np.concatenate([m[:, 2:4], np.stack([rng.uniform(0, Cs.W, extra), rng.uniform(0, Cs.H, extra)], 1).astype(f32)])
    p1, p2 = rng.permutation(n + extra), rng.permutation(n + extra)               # key point j of the case sits at index p[j] of the frame
    keys1, keys2 = np.zeros_like(k1), np.zeros_like(k2)
    keys1[p1], keys2[p2] = k1, k2
    m12 = np.full(n + extra, -1, np.int32)
    m12[p1[:n]] = p2[:n]
    first = np.flatnonzero(m12 >= 0)
    matches = np.ascontiguousarray(np.concatenate([keys1[first], keys2[m12[first]]], 1), f32)
    return dict(keys1=keys1, keys2=keys2, m12=m12, first=first, matches=matches, sigma=1.0, iterations=40 if name == "short_7" else len(c["sets"]))


def parse_answers(text):
    lines, out, k = text.splitlines(), [], 0
    while k < len(lines):
        if lines[k].startswith("draws "):
            draws = int(lines[k].split()[1]); k += 1
        else:
            draws = None
        drawn = np.array(lines[k].split()[2:], np.int32).reshape(-1, 8); k += 1
        tag, ok, nr, nt, npnt, ntri = lines[k].split()
        rt = np.array([int(x, 16) for x in lines[k + 1].split()], np.uint32).view(f32)
        P = np.array([int(x, 16) for x in lines[k + 2].split()], np.uint32).view(f32).reshape(-1, 3)
        tri = np.array([ch == "1" for ch in lines[k + 3].strip()], bool)
        assert len(rt) == int(nr) + int(nt) and len(P) == int(npnt) and len(tri) == int(ntri)
        out.append(dict(tag=tag, ok=int(ok), R=rt[:int(nr)], t=rt[int(nr):], P=P, tri=tri, draws=draws, sets=drawn))
        k += 4
    return out


def run_cpp(exe, library, tmp, env=None, whole_stream=True):
    """the class equal to the C ABI on the scenes (Initialize, then InitializeBatch over the same scenes with the generator's stream going on), its
    draws equal to the model's restatement of the reference's generator from seed 0, Normalize's sums, the scatter to `first`.  rand() belongs to the
    whole process: with whole_stream every call's sets must continue the one stream; without it (a process in which the device runtime runs between the
    calls and may take values of rand() itself) the first call's sets must, and no later call may start the stream again"""
    rng = np.random.default_rng(77)
    scenes = [cpp_scene(nm, rng) for nm in CPP_SCENES]
    path_in, path_out = os.path.join(str(tmp), "scenes.txt"), os.path.join(str(tmp), "answers.txt")
    with open(path_in, "w") as f:
        for s in scenes:
            f.write("%d %d %.9g %d %.9g %.9g %.9g %.9g\n" % ((len(s["keys1"]), len(s["keys2"]), s["sigma"], s["iterations"]) + tuple(float(k) for k in Cs.K)))
            for (x, y), j in zip(s["keys1"], s["m12"]):
                f.write("%08x %08x %d\n" % (int(np.float32(x).view(np.uint32)), int(np.float32(y).view(np.uint32)), j))
            for x, y in s["keys2"]:
                f.write("%08x %08x\n" % (int(np.float32(x).view(np.uint32)), int(np.float32(y).view(np.uint32))))
    r = subprocess.run([exe, path_in, path_out], capture_output=True, text=True, timeout=300, env=dict(os.environ if env is None else env))
    assert r.returncode == 0 and "init_cpp ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    answers = parse_answers(open(path_out).read())
    assert [a["tag"] for a in answers] == ["single"] * len(scenes) + ["batch"] * len(scenes)
    rand = M.LibcRand(0)                                                        # one stream for the whole process: the second Initialize does not re-seed
    sets = [M.draw_sets(len(s["matches"]), s["iterations"], rand) if len(s["matches"]) >= 8 else None for s in scenes + scenes]
    seen, continued = set(), 0
    for k, (s, a) in enumerate(zip(scenes + scenes, answers)):
        if sets[k] is None:                                                     # fewer than 8 matches: false before any draw, nothing touched
            assert a["ok"] == 0 and a["draws"] in (0, None) and len(a["sets"]) == 0 and (a["tag"] == "batch" or (len(a["R"]) == 4 and len(a["P"]) == 1)), a
            seen.add("short")
            continue
        assert a["draws"] in (8 * s["iterations"], None) and a["sets"].shape == sets[k].shape
        assert a["sets"].min() >= 0 and a["sets"].max() < len(s["matches"]) and all(len(set(row)) == 8 for row in a["sets"].tolist())
        if k == 0 or whole_stream:
            assert np.array_equal(a["sets"], sets[k]), k
        else:
            assert not np.array_equal(a["sets"], M.draw_sets(len(s["matches"]), s["iterations"], M.LibcRand(0))), "a later call started the stream again"
        continued += int(np.array_equal(a["sets"], sets[k]))
        dv = orb_slam2_amd.init_reconstruct(Cs.K, s["matches"], a["sets"], M.normalize(s["keys1"]), M.normalize(s["keys2"]), sigma=s["sigma"], library=library)
        assert a["ok"] == dv["returned"], (k, a["ok"], dv["returned"])
        if dv["returned"]:
            P, tri = np.zeros((len(s["keys1"]), 3), f32), np.zeros(len(s["keys1"]), bool)
            P[s["first"]], tri[s["first"]] = dv["p3d"], dv["triangulated"]
            assert same_bits(a["R"], dv["R21"].ravel()) and same_bits(a["t"], dv["t21"]) and same_bits(a["P"], P) and np.array_equal(a["tri"], tri), k
            assert tri.any() and not np.array_equal(s["first"], np.arange(len(s["first"])))
            seen.add("H" if dv["model"] == 0 else "F")
        else:
            untouched = dv["model"] == 0 and a["tag"] == "single"
            assert len(a["R"]) == (4 if untouched else 0) and len(a["t"]) == (4 if untouched else 0) and len(a["P"]) == (1 if a["tag"] == "single" else 0), (k, a)
            seen.add("fails_H" if dv["model"] == 0 else "fails_F")
    assert seen == {"short", "H", "F", "fails_H", "fails_F"}, seen
    print(r.stdout.splitlines()[-1], sorted(seen), f"{continued} of {len(answers) - 2} drawing calls continue the one stream from seed 0")
