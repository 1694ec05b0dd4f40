"""The checks tests/test_sim3_opt_emu.py (CPU emulation of the kernel) and tests/test_sim3_opt_gpu.py (the device) share: orbhip_sim3_optimize and its
batch form against tests/sim3_opt_model.py on the cases of tests/sim3_opt_cases.py, with the seeds and the per-case tolerance of
tests/golden/sim3_opt_spread.npz.

Tolerance.  Flags and the return value must equal the model's.  S12_out may deviate by 4 x the case's recorded spread plus one double ulp per entry: the
kernel's reduction tree is one more order of the same sums and the device's exp / sin / cos one more jitter, so its deviation is a draw from what the 16
recorded draws sampled, and 4 x the largest of 16 keeps false alarms rare; the ulp stands for a case whose recorded spread is 0.  Per entry:
|dq_i| <= 4 spread_rot + ulp(q_i) (a rotation by an angle a moves no entry of a quaternion of norm 1 +- 1e-7 by more than a / 2 (1 + 1e-7) < a),
|dt_i| <= 4 spread_t + ulp(t_i), |ds| <= 4 spread_s + ulp(s).  The spreads are large next to pose optimisation's (up to 7e-7 rad here against 1e-9 there)
because the reference's numerical Jacobians multiply every last-bit difference by 5e8; a sign error in inverse(), a normalised quaternion, a contracted
product or a forward difference moves S12 by orders of magnitude more, or changes the flags."""
import ctypes as C
import os
import subprocess

import numpy as np

import orb_slam2_amd
import sim3_opt_cases as Cs
import sim3_opt_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sim3_opt_spread.npz")
_golden = None
_cache = {}


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def case(name):
    """(cams, S12, pairs, th2, fix_scale, the model's S12_out / flags / return value, the recorded spread): computed once, shared, never changed"""
    if name not in _cache:
        g = golden()
        cams, S12, pairs, th2, fix, info = Cs.case(name, int(g[name + "/seed"]))
        S, removed, nin = M.optimize_sim3(cams, S12, pairs, th2, fix)
        assert S.tobytes() == g[name + "/S12"].tobytes(), f"{name}: the model no longer gives the recorded S12 - rerun tests/golden/make_golden_sim3_opt_spread.py"
        for a in (cams, S12, pairs, S, removed):
            a.setflags(write=False)
        _cache[name] = (cams, S12, pairs, th2, fix, S, removed, nin, g[name + "/spread"])
    return _cache[name]


def args(name):
    return case(name)[:5]


def s12_close(S, want, spread):
    S = np.asarray(S, np.float64).reshape(8); want = np.asarray(want, np.float64).reshape(8)
    tol = np.spacing(np.abs(want))
    tol[:4] += 4.0 * spread[0]; tol[4:7] += 4.0 * spread[1]; tol[7] += 4.0 * spread[2]
    d = np.abs(S - want)
    return bool((d <= tol).all()), float((d - tol).max())


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2]


def check_case(name, library):
    cams, S12, pairs, th2, fix, S, removed, nin, spread = case(name)
    Sd, rd, nd = orb_slam2_amd.sim3_optimize(cams, S12, pairs, th2, fix, library=library)
    assert np.array_equal(rd, removed), (name, np.flatnonzero(rd != removed)[:8])
    assert nd == nin, (name, nd, nin)
    ok, over = s12_close(Sd, S, spread)
    print(f"{name}: n {len(pairs)}, removed {int(rd.sum())}, inliers {nd}, largest |entry difference| - tolerance {over:.3e}, deviation {Cs.deviation(Sd, S)}, spread {spread}")
    assert ok, (name, over, Sd, S)
    if fix:
        assert Sd[7].tobytes() == np.float64(S12[7]).tobytes(), name                 # the scale keeps its bits
    if S.tobytes() == S12.tobytes():
        assert Sd.tobytes() == S12.tobytes(), name                                   # the member's early return (and an estimate that never moved) leaves g2oS12's bits


def check_case_bits(name, library):
    """Under emulation only: the kernel's exp / sin / cos / pow are then the model's (the C library's) and the model can add in the kernel's own order
    (tree = the workgroup size), so nothing is left to differ: S12_out, flags and return value bit for bit.  This is the check that tells a
    forward-difference Jacobian (right to 1e-9) or a build with contracted products from the shipped kernel: both stay inside 4 x the recorded spread
    in every case (measured with mutated emulation builds), because the spread is itself the effect of last-bit differences times 5e8."""
    cams, S12, pairs, th2, fix = args(name)
    S, removed, nin = M.optimize_sim3(cams, S12, pairs, th2, fix, tree=Cs.WORKGROUP)
    Sd, rd, nd = orb_slam2_amd.sim3_optimize(cams, S12, pairs, th2, fix, library=library)
    assert np.array_equal(rd, removed) and nd == nin, name
    assert Sd.tobytes() == S.tobytes(), (name, Cs.deviation(Sd, S))


def check_repeat(library):
    a = orb_slam2_amd.sim3_optimize(*args("n257_o30_f0"), library=library)
    b = orb_slam2_amd.sim3_optimize(*args("n257_o30_f0"), library=library)
    assert same(a, b)


# (the largest problems, n1025 and n5000, do not stage: a launch sized by them alone and not capped at the staging limit, or sized by the first problem, would leave n1024 without its LDS)
BATCH = ["n257_o30_f0", "n9_o30_f1", "n1024_o30_f0", None, "n1025_o30_f1", "all_removed", "left_9", "n257_o30_f0", "n63_o0_f1", "n64_o30_f0", "far_start", "n255_o0_f0",
         "zero_residual", "n5000_o30_f1", "th2_4", "n257_o30_f0"]


def check_batch_slots(library):
    """a problem alone, and the same problem at slots 0, 7 and 15 of a mixed-size batch with n = 0 and n = 9 in it: the same bits; every other slot equals its
    own single call and the model's flags and count"""
    empty = (Cs.CAMS, case("n10_o0_f0")[1], np.zeros((0, 12), np.float32), 10.0, False)
    probs = [args(n) if n else empty for n in BATCH]
    alone = orb_slam2_amd.sim3_optimize(*args("n257_o30_f0"), library=library)
    out = orb_slam2_amd.sim3_optimize_batch(probs, library=library)
    assert len(out) == 16
    for k in (0, 7, 15):
        assert same(out[k], alone), k
    assert out[3][2] == 0 and len(out[3][1]) == 0 and out[3][0].tobytes() == empty[1].tobytes()
    for k, n in enumerate(BATCH):
        if n is None:
            continue
        one = orb_slam2_amd.sim3_optimize(*args(n), library=library)
        assert same(out[k], one), (k, n)
        assert np.array_equal(out[k][1], case(n)[6]) and out[k][2] == case(n)[7], (k, n)
        assert s12_close(out[k][0], case(n)[5], case(n)[8])[0], (k, n)
    assert orb_slam2_amd.sim3_optimize_batch([], library=library) == []


def check_empty_and_bad_arguments(library):
    """n == 0 returns OK with n_inliers = 0 and writes nothing else; bad arguments are refused"""
    L = orb_slam2_amd.lib(library)
    cams, S12, pairs, th2, fix = args("n10_o0_f0")
    Q = orb_slam2_amd.orbhip._Sim3OptProblem()
    C.memmove(Q.cam, cams.ctypes.data, 32); C.memmove(Q.S12_in, S12.ctypes.data, 64)
    marker = np.full(8, -5.0)
    C.memmove(Q.S12_out, marker.ctypes.data, 64)
    flags = np.full(12, 7, np.uint8)
    p = orb_slam2_amd.orbhip._sim3_pairs(pairs)
    Q.pairs, Q.n, Q.th2, Q.fix_scale, Q.removed, Q.n_inliers = p.ctypes.data, 0, 10.0, 0, flags.ctypes.data, -3
    assert L.orbhip_sim3_optimize(0, C.byref(Q)) == 0
    assert Q.n_inliers == 0 and bytes(Q.S12_out) == marker.tobytes() and (flags == 7).all()
    Q.n = 10; Q.n_inliers = -3
    assert L.orbhip_sim3_optimize(0, C.byref(Q)) == 0
    assert (flags[10:] == 7).all() and (flags[:10] <= 1).all() and Q.n_inliers == case("n10_o0_f0")[7]      # n flags, no more, are written
    Q.removed = None
    assert L.orbhip_sim3_optimize(0, C.byref(Q)) == 1 and L.orbhip_last_error() != b""
    Q.removed = flags.ctypes.data; Q.pairs = None
    assert L.orbhip_sim3_optimize(0, C.byref(Q)) == 1
    Q.pairs = p.ctypes.data; Q.n = -1
    assert L.orbhip_sim3_optimize(0, C.byref(Q)) == 1
    assert L.orbhip_sim3_optimize(0, None) == 1 and L.orbhip_sim3_optimize_batch(0, 2, None) == 1 and L.orbhip_sim3_optimize_batch(0, 0, None) == 0


def check_three_threads(library):
    import threading
    names = ["n65_o30_f0", "n257_o30_f1", "n1025_o30_f0"]
    for n in names:
        case(n)
    out, errs = {}, []

    def work(name):
        try:
            for _ in range(3):
                out[name] = orb_slam2_amd.sim3_optimize(*args(name), library=library)
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
        assert np.array_equal(out[n][1], case(n)[6]) and out[n][2] == case(n)[7], n
        assert s12_close(out[n][0], case(n)[5], case(n)[8])[0], n


def build_cpp(tmp, library, sanitize=False):
    """tests/sim3_opt_cpp/main.cc + orb_slam2_amd/cpp/Sim3Optimizer.cc as a stand-alone program linked to `library`, in the directory tmp"""
    d, f = os.path.split(os.path.abspath(library))
    exe = os.path.join(str(tmp), "sim3_opt_cpp_asan" if sanitize else "sim3_opt_cpp")
    cmd = ["g++", "-std=c++14", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-DCVLITE_ALGEBRA", "-DORBHIP_USE_OPENCV"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    cmd += ["-I" + os.path.join(ROOT, "tests", "sim3_opt_cpp"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "cvlite"),
            os.path.join(ROOT, "tests", "sim3_opt_cpp", "main.cc"), os.path.join(ROOT, "orb_slam2_amd", "cpp", "Sim3Optimizer.cc"),
            "-o", exe, "-L" + d, "-l" + f[3:-3], "-Wl,-rpath," + d]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpp(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "sim3_opt_cpp ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
