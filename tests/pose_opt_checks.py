"""The checks tests/test_pose_opt_emu.py (CPU emulation of the kernel) and tests/test_pose_opt_gpu.py (the device) share: orbhip_pose_optimization and its
batch and frame forms against tests/pose_opt_model.py on the cases of tests/pose_opt_cases.py, with the seeds and the per-case tolerance of
tests/golden/pose_opt_spread.npz.

Tolerance.  Flags and the return value must equal the model's.  The pose may deviate by 4 x the case's recorded permutation spread plus one float ulp per
entry: the kernel's reduction tree is one more order of the same sums (and the device's sin / cos may differ from libm's in a last bit), so its deviation is a
draw from what the 16 recorded permutations sampled, and 4 x the largest of 16 keeps false alarms rare; the ulp is the final rounding to float.  Per entry:
|dR_ij| <= 4 spread_rot + ulp(R_ij) (a rotation by an angle a moves no entry by more than a), |dt_i| <= 4 spread_t + ulp(t_i).  A wrong sign, weight or
update order moves the pose by orders of magnitude more (the recorded spreads are 0 to 1e-9 rad, and 0 in translation)."""
import ctypes as C
import os
import subprocess

import numpy as np

import orb_slam2_amd
import pose_opt_cases as Cs
import pose_opt_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pose_opt_spread.npz")
_golden = None
_cache = {}


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(GOLDEN))
    return _golden


def case(name):
    """(cam, Tcw, obs, the model's pose / flags / inlier count, the recorded spread): computed once, shared, never changed"""
    if name not in _cache:
        g = golden()
        cam, T0, obs, info = Cs.case(name, int(g[name + "/seed"]))
        T, flags, ninl = M.pose_optimization(cam, T0, obs)
        assert T.tobytes() == g[name + "/pose"].tobytes(), f"{name}: the model no longer gives the recorded pose - rerun tests/golden/make_golden_pose_opt_spread.py"
        for a in (cam, T0, obs, T, flags):
            a.setflags(write=False)
        _cache[name] = (cam, T0, obs, T, flags, ninl, g[name + "/spread"])
    return _cache[name]


def pose_close(T, want, spread):
    T = np.asarray(T, np.float32).reshape(4, 4); want = np.asarray(want, np.float32).reshape(4, 4)
    tol = np.zeros((4, 4))
    tol[:3, :3] = 4.0 * spread[0] + np.spacing(np.abs(want[:3, :3]))
    tol[:3, 3] = 4.0 * spread[1] + np.spacing(np.abs(want[:3, 3]))
    d = np.abs(T.astype(np.float64) - want.astype(np.float64))
    return bool((d <= tol).all()), float((d - tol).max())


def check_case(name, library):
    cam, T0, obs, T, flags, ninl, spread = case(name)
    Td, fd, nd = orb_slam2_amd.pose_optimization(cam, T0, obs, library=library)
    assert np.array_equal(fd, flags), (name, np.flatnonzero(fd != flags)[:8])
    assert nd == ninl, (name, nd, ninl)
    ok, over = pose_close(Td, T, spread)
    print(f"{name}: n {len(obs)}, inliers {nd}, largest |entry difference| - tolerance {over:.3e}, spread {spread[0]:.3e} rad {spread[1]:.3e}")
    assert ok, (name, over, Td, T)
    assert nd == len(obs) - int(flags.sum())


def check_repeat(library):
    cam, T0, obs, *_ = case("n257_mixed_30")
    a = orb_slam2_amd.pose_optimization(cam, T0, obs, library=library)
    b = orb_slam2_amd.pose_optimization(cam, T0, obs, library=library)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2]


BATCH = ["n65_mixed_30", "n3_mono_0", "n2000_stereo_30", "n9_mixed_30", "n256_mono_0", "n10_stereo_30", "n5000_mixed_30", "n257_mixed_30", "n63_stereo_0", "n64_mixed_30",
         "far_start", "n255_mono_30", "noisy", "n10_mono_0", "n2000_mono_0", "n257_mixed_30"]


def check_batch_slots(library):
    """a problem alone, and the same problem at slots 0, 7 and 15 of a mixed-size batch: the same bits; every other slot equals its own single call"""
    names = list(BATCH)
    names[0] = names[7] = names[15] = "n257_mixed_30"
    names[3] = None                                                            # a problem with fewer than 3 observations inside the batch
    short = case("n10_mono_0")
    probs = [case(n)[:3] if n else (short[0], short[1], short[2][:2]) for n in names]
    alone = orb_slam2_amd.pose_optimization(*case("n257_mixed_30")[:3], library=library)
    out = orb_slam2_amd.pose_optimization_batch(probs, library=library)
    assert len(out) == 16
    for k in (0, 7, 15):
        assert out[k][0].tobytes() == alone[0].tobytes() and np.array_equal(out[k][1], alone[1]) and out[k][2] == alone[2], k
    assert out[3][2] == 0 and not out[3][1].any() and out[3][0].tobytes() == short[1].tobytes()
    for k, n in enumerate(names):
        if n is None:
            continue
        one = orb_slam2_amd.pose_optimization(*case(n)[:3], library=library)
        assert out[k][0].tobytes() == one[0].tobytes() and np.array_equal(out[k][1], one[1]) and out[k][2] == one[2], (k, n)
        assert np.array_equal(out[k][1], case(n)[4]) and out[k][2] == case(n)[5], (k, n)
    assert orb_slam2_amd.pose_optimization_batch([], library=library) == []


# (the first live problem is the smallest: a launch sized by it, and not by the largest, would leave n2048 without its LDS)
BATCH_EDGES = ["zero_residual", "n2048_mixed_30", "turn_123_m130", None, "n2049_mixed_30", "all_outliers_300", "turn_y_pi_exact", "behind_camera"]


def check_batch_edges(library):
    """the size and degenerate cases side by side in one batch.  The launch takes its LDS size from the largest problem: n2049 (not staged) next to n2048
    (staged, and so in need of all 2048 x 28 bytes) is a batch whose largest problem does not stage.  Every slot equals its own single call bit for bit and
    the model's flags and count; the problem with 2 observations is untouched."""
    short = case("n10_mono_0")
    probs = [case(n)[:3] if n else (short[0], short[1], short[2][:2]) for n in BATCH_EDGES]
    out = orb_slam2_amd.pose_optimization_batch(probs, library=library)
    assert len(out) == len(BATCH_EDGES)
    for k, n in enumerate(BATCH_EDGES):
        if n is None:
            assert out[k][2] == 0 and not out[k][1].any() and len(out[k][1]) == 2 and out[k][0].tobytes() == short[1].tobytes()
            continue
        one = orb_slam2_amd.pose_optimization(*case(n)[:3], library=library)
        assert out[k][0].tobytes() == one[0].tobytes() and np.array_equal(out[k][1], one[1]) and out[k][2] == one[2], (k, n)
        assert np.array_equal(out[k][1], case(n)[4]) and out[k][2] == case(n)[5], (k, n)
        ok, over = pose_close(out[k][0], case(n)[3], case(n)[6])
        assert ok, (k, n, over)
    # what the degenerate slots are there for: nothing left, nothing flagged, and the two poses that may not move
    a, z = out[BATCH_EDGES.index("all_outliers_300")], out[BATCH_EDGES.index("zero_residual")]
    assert a[2] == 0 and a[1].all() and a[0].tobytes() == M.to_cvmat(M.to_se3quat(case("all_outliers_300")[1])).tobytes()
    assert z[2] == 40 and not z[1].any() and z[0].tobytes() == case("zero_residual")[1].tobytes()


def check_short_untouched(library):
    """n < 3 leaves the pose buffer and the flags untouched"""
    L = orb_slam2_amd.lib(library)
    cam, T0, obs, *_ = case("n10_mono_0")
    obs = orb_slam2_amd.orbhip._pose_obs(obs)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for n in (0, 1, 2):
        out = np.full(16, -5.0, np.float32); flags = np.full(4, 7, np.uint8); ninl = C.c_int(-3)
        assert L.orbhip_pose_optimization(0, p(cam), p(np.ascontiguousarray(T0)), p(obs), n, p(out), p(flags), C.byref(ninl)) == 0
        assert ninl.value == 0 and (out == -5.0).all() and (flags == 7).all(), n
    out = np.full(16, -5.0, np.float32); flags = np.full(12, 7, np.uint8); ninl = C.c_int(-3)
    assert L.orbhip_pose_optimization(0, p(cam), p(np.ascontiguousarray(T0)), p(obs), 10, p(out), p(flags), C.byref(ninl)) == 0
    assert (flags[10:] == 7).all() and (flags[:10] <= 1).all() and out[15] == 1.0                 # ... and n flags, no more, are written otherwise
    assert L.orbhip_pose_optimization(0, None, p(np.ascontiguousarray(T0)), p(obs), 10, p(out), p(flags), C.byref(ninl)) == 1 and L.orbhip_last_error() != b""
    assert L.orbhip_pose_optimization(0, p(cam), p(np.ascontiguousarray(T0)), None, 10, p(out), p(flags), C.byref(ninl)) == 1
    assert L.orbhip_pose_optimization(0, p(cam), p(np.ascontiguousarray(T0)), p(obs), -1, p(out), p(flags), C.byref(ninl)) == 1


def check_frame_form(library):
    """the frame form on a resident frame against the host-array form on the same data: the same bits"""
    from orb_slam2_amd import synth
    Wd, Hd = 320, 240
    ex = orb_slam2_amd.ORBextractor(400, 1.2, 8, 20, 7, Wd, Hd, max_batch=1, library=library)
    kps, _ = ex.extract_batch(synth.sequence(Wd, Hd, 1, seed=5))
    kp = kps[0]
    n = len(kp)
    assert n > 150
    rng = np.random.default_rng(9)
    cam = Cs.CAM.copy(); cam[2:4] = (160.2, 119.6)
    fx, fy, cx, cy, bf = cam.astype(np.float64)
    z = rng.uniform(2, 15, n)
    u_right = np.where(np.arange(n) % 3 == 0, -1.0, kp["x"] - bf / z).astype(np.float32)
    ex.set_stereo_columns(u_right)
    idx = rng.permutation(n)[:n - 20].astype(np.int32)                           # not every key point has a map point, and not in key point order
    xyz = np.stack([(kp["x"][idx] - cx) / fx * z[idx], (kp["y"][idx] - cy) / fy * z[idx], z[idx]], 1)
    xyz[::9] += rng.normal(0, 0.5, xyz[::9].shape)                               # some wrong matches
    xyz = xyz.astype(np.float32)
    T0 = np.eye(4, dtype=np.float32); T0[:3, 3] = (0.04, -0.03, 0.05)
    is2 = ex._tables()[3]
    assert np.array_equal(is2, Cs.inv_level_sigma2())                            # the context's table is mvInvLevelSigma2 as ORBextractor computes it
    obs = np.stack([kp["x"][idx], kp["y"][idx], u_right[idx], is2[kp["octave"][idx]], xyz[:, 0], xyz[:, 1], xyz[:, 2]], 1).astype(np.float32)
    a = ex.pose_optimization_frame(cam, T0, idx, xyz)
    b = orb_slam2_amd.pose_optimization(cam, T0, obs, library=library)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2]
    Tm, fm, nm = M.pose_optimization(cam, T0, obs)
    assert np.array_equal(a[1], fm) and a[2] == nm and 0 < fm.sum() < len(fm) and a[0].tobytes() != T0.tobytes()
    few = ex.pose_optimization_frame(cam, T0, idx[:2], xyz[:2])
    assert few[2] == 0 and few[0].tobytes() == T0.tobytes()
    try:
        ex.pose_optimization_frame(cam, T0, np.array([0, 1, ex.capacity + 5], np.int32), xyz[:3])
        raise AssertionError("an index outside the frame must be refused")
    except orb_slam2_amd.OrbHipError as e:
        assert "index" in str(e)
    # ... and so must the first index past the frame's own key points, also on a context whose counts the host has not seen (a device-resident extraction):
    # the count is then read from the device, never taken to be the capacity
    for resident in (False, True):
        if resident:
            img = np.ascontiguousarray(synth.sequence(Wd, Hd, 1, seed=5)[0])
            buf = orb_slam2_amd.DeviceBuffer(img.size, library=library)
            buf.upload(img)
            ex.extract_device(buf.ptr, 1, img.size, Wd)
        try:
            ex.pose_optimization_frame(cam, T0, np.array([0, 1, n], np.int32), xyz[:3])
            raise AssertionError("the index just past the frame's key points must be refused")
        except orb_slam2_amd.OrbHipError as e:
            assert f"outside 0..{n - 1}" in str(e), (resident, str(e))


def check_three_threads(library):
    import threading
    names = ["n65_mixed_30", "n257_mixed_30", "n2000_mono_30"]
    for n in names:
        case(n)
    out, errs = {}, []

    def work(name):
        try:
            cam, T0, obs, *_ = case(name)
            for _ in range(3):
                out[name] = orb_slam2_amd.pose_optimization(cam, T0, obs, library=library)
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
        assert np.array_equal(out[n][1], case(n)[4]) and out[n][2] == case(n)[5], n


def build_cpp(tmp, library, sanitize=False):
    """tests/pose_opt_cpp/main.cc + orb_slam2_amd/cpp/PoseOptimizer.cc as a stand-alone program linked to `library`, in the directory tmp"""
    d, f = os.path.split(os.path.abspath(library))
    exe = os.path.join(str(tmp), "pose_opt_cpp_asan" if sanitize else "pose_opt_cpp")
    cmd = ["g++", "-std=c++14", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-DCVLITE_ALGEBRA", "-DORBHIP_USE_OPENCV"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    cmd += ["-I" + os.path.join(ROOT, "tests", "pose_opt_cpp"), "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "cvlite"),
            os.path.join(ROOT, "tests", "pose_opt_cpp", "main.cc"), os.path.join(ROOT, "orb_slam2_amd", "cpp", "PoseOptimizer.cc"),
            "-o", exe, "-L" + d, "-l" + f[3:-3], "-Wl,-rpath," + d]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpp(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "pose_opt_cpp ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
