#!/usr/bin/env python3
"""Milliseconds per call of Optimizer::PoseOptimization on the device (orbhip_pose_optimization, its frame and batch forms).

    python tools/pose_opt_rate.py [--calls 50] [--out profiles/pose_opt_rate.json]                on the MI355X

Workloads (tests/pose_opt_cases.py, seed 1, mixed monocular / stereo edges, 20 % gross outliers): single calls at n = 300 and n = 1500 on host arrays;
the frame form at the same sizes (observations gathered on the device from a resident frame's key points); one batch of 16 x 300.  Each figure is the
median wall time of --calls calls of the C ABI (upload, the one launch, download) after three warm-up calls, with the minimum and the share
orbhip_thread_api_ms attributes to the library; the clock is time.perf_counter around a synchronous call.  The workgroup size is a compile-time constant
of the kernel (PO_T, orb_slam2_amd/csrc/orbhip_pose_opt.hip); the sweep it was chosen from is recorded in DESIGN.md section 4.
No target is set and NO REFERENCE FIGURE exists: the reference's member needs g2o, which needs Eigen, and cannot be built where this project is developed;
the file says so.  A device that is missing is an error."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(L, fn, calls):
    for _ in range(3):
        fn()
    wall, api = [], []
    for _ in range(calls):
        L.orbhip_thread_api_ms(1)
        t0 = time.perf_counter(); fn(); wall.append((time.perf_counter() - t0) * 1e3)
        api.append(L.orbhip_thread_api_ms(0))
    return {"ms_median": float(np.median(wall)), "ms_min": float(np.min(wall)), "library_share": float(np.median(api) / np.median(wall)), "calls": calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import orb_slam2_amd
    from orb_slam2_amd import synth
    import pose_opt_cases as Cs
    import pose_opt_model as M
    L = orb_slam2_amd.lib()
    if L.orbhip_device_count() < 1:
        sys.exit("no HIP device: the figures are measured on an MI355X or not at all")
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    res = {"workload": "tests/pose_opt_cases.py make(n, 'mixed', 0.2, seed 1): n = 300 and 1500 single and frame form, 16 x 300 batch",
           "reference": "none: Optimizer::PoseOptimization needs g2o, g2o needs Eigen, and neither could be built where this was measured - no ratio is claimed",
           "machine": "MI355X box", "runtime": str(orb_slam2_amd.runtime_info())}
    problems = {}
    for n in (300, 1500):
        cam, T0, obs, _ = Cs.make(n, "mixed", 0.2, 1)
        obs_s = orb_slam2_amd.orbhip._pose_obs(obs)
        T0 = np.ascontiguousarray(T0)
        out, flags, ninl = np.zeros(16, np.float32), np.zeros(n, np.uint8), C.c_int(0)

        def one():
            assert L.orbhip_pose_optimization(0, p(cam), p(T0), p(obs_s), n, p(out), p(flags), C.byref(ninl)) == 0, L.orbhip_last_error()
        res[f"single_n{n}"] = timed(L, one, a.calls)
        Tm, fm, nm = M.pose_optimization(cam, T0, obs)                          # the timed answers are the right ones
        assert np.array_equal(flags.astype(bool), fm) and ninl.value == nm, n
        res[f"single_n{n}"]["inliers"] = nm
        problems[n] = (cam, T0, obs)
    # the frame form: a resident frame with enough key points; the map points are made to fit its key points
    Wd, Hd = 1241, 376
    ex = orb_slam2_amd.ORBextractor(2000, 1.2, 8, 20, 7, Wd, Hd, max_batch=1)
    kps, _ = ex.extract_batch(synth.sequence(Wd, Hd, 1, seed=3))
    kp = kps[0]
    rng = np.random.default_rng(1)
    cam = np.array([718.856, 718.856, 607.19, 185.2, 386.1], np.float32)
    fx, fy, cx, cy, bf = cam.astype(np.float64)
    z = rng.uniform(3, 40, len(kp))
    ex.set_stereo_columns(np.where(np.arange(len(kp)) % 2 == 0, kp["x"] - bf / z, -1.0).astype(np.float32))
    T0 = np.eye(4, dtype=np.float32); T0[:3, 3] = (0.05, -0.02, 0.08)
    for n in (300, 1500):
        if len(kp) < n:
            sys.exit(f"the synthetic frame has {len(kp)} key points, {n} needed")
        idx = rng.permutation(len(kp))[:n].astype(np.int32)
        xyz = np.stack([(kp["x"][idx] - cx) / fx * z[idx], (kp["y"][idx] - cy) / fy * z[idx], z[idx]], 1)
        bad = rng.choice(n, n // 5, replace=False)
        xyz[bad] += rng.normal(0, 1.0, (len(bad), 3))
        xyz = np.ascontiguousarray(xyz, np.float32)
        out, flags, ninl = np.zeros(16, np.float32), np.zeros(n, np.uint8), C.c_int(0)

        def one_frame():
            assert L.orbhip_pose_optimization_frame(ex.h, 0, p(cam), p(T0), p(idx), p(xyz), n, p(out), p(flags), C.byref(ninl)) == 0, L.orbhip_last_error()
        res[f"frame_n{n}"] = timed(L, one_frame, a.calls)
        res[f"frame_n{n}"]["inliers"] = ninl.value
    batch = [Cs.make(300, "mixed", 0.2, 10 + k)[:3] for k in range(16)]
    res["batch_16x300"] = timed(L, lambda: orb_slam2_amd.pose_optimization_batch(batch), a.calls)
    res["batch_16x300"]["note"] = "through the Python mirror: includes building the 16 problem records"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
