#!/usr/bin/env python3
"""Milliseconds per call of Optimizer::OptimizeSim3 on the device (orbhip_sim3_optimize and its batch form).

    python tools/sim3_opt_rate.py [--calls 50] [--out profiles/sim3_opt_rate.json] [--variant NAME=LIBRARY ...]                on the MI355X

Workloads (tests/sim3_opt_cases.py make(), seed 1, true scale 1.7, half a level sigma of pixel noise): single calls at n = 50, 100 and 300 pairs, without outliers (the second phase is
optimize(5)) and with 30 % (optimize(10)), the scale free and fixed; batches of 4 and 16 problems of 100 pairs against the loop of single calls over the
same problems, timed alternately in the same run; orbhip_pose_optimization at 300 observations in the same run, as the yardstick for a one-workgroup
Levenberg-Marquardt launch.  Each figure is the median wall time of --calls synchronous calls of the C ABI (upload, the one launch, download) after three
warm-up calls, with the minimum; the clock is time.perf_counter around the call.

--variant times other builds of the same source on the n = 100 and n = 300 workloads, alternating with the shipped library call by call, and requires
their flags and return values to equal the shipped library's, and S12_out bit for bit unless the name starts with T (another workgroup size is another
order of the sums).  The two that DESIGN.md section 4 records:
    every_trial=...     orbhip_sim3_opt.hip compiled with -DS3O_SYSTEM_EVERY_TRIAL=1 (every LM trial builds the system; the shipped build does after acceptance)
    T64=... T128=... T512=...   compiled with -DS3O_T=64 / 128 / 512 (the shipped build has 256)
(compile that one file with the Makefile's HIPFLAGS plus the -D, link it with the other objects into a library of another name).
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


def timed(fns, calls):
    """the functions called in turn, `calls` rounds after three warm-up rounds: one {"ms_median", "ms_min", "calls"} per function"""
    for _ in range(3):
        for fn in fns:
            fn()
    wall = [[] for _ in fns]
    for _ in range(calls):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter(); fn(); wall[k].append((time.perf_counter() - t0) * 1e3)
    return [{"ms_median": float(np.median(w)), "ms_min": float(np.min(w)), "calls": calls} for w in wall]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variant", action="append", default=[])
    a = ap.parse_args()
    import orb_slam2_amd
    from orb_slam2_amd.orbhip import _Sim3OptProblem, _sim3_pairs
    import pose_opt_cases as Pc
    import sim3_opt_cases as Cs
    import sim3_opt_model as M
    L = orb_slam2_amd.lib()
    if L.orbhip_device_count() < 1:
        sys.exit("no HIP device: the figures are measured on an MI355X or not at all")
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    res = {"workload": "tests/sim3_opt_cases.py make(n, share, fix_scale, seed 1, scale 1.7, noise 0.5): n = 50, 100, 300; share 0 (second phase optimize(5)) and 0.3 (optimize(10)); batches of 4 and 16 x 100",
           "reference": "none: Optimizer::OptimizeSim3 needs g2o, g2o needs Eigen, and neither could be built where this was measured - no ratio is claimed",
           "machine": "MI355X box", "runtime": str(orb_slam2_amd.runtime_info())}

    def record(lib, cams, S12, pairs, th2, fix):
        """one orbhip_sim3_opt_problem, filled once, and the function that runs it"""
        Q = _Sim3OptProblem()
        keep = (_sim3_pairs(pairs), np.zeros(len(pairs), np.uint8), np.ascontiguousarray(cams, np.float32), np.ascontiguousarray(S12, np.float64))
        C.memmove(Q.cam, keep[2].ctypes.data, 32); C.memmove(Q.S12_in, keep[3].ctypes.data, 64)
        Q.pairs, Q.n, Q.th2, Q.fix_scale, Q.removed = keep[0].ctypes.data, len(pairs), float(th2), int(fix), keep[1].ctypes.data

        def one():
            assert lib.orbhip_sim3_optimize(0, C.byref(Q)) == 0, lib.orbhip_last_error()
        return Q, keep, one

    variants = [v.split("=", 1) for v in a.variant]
    vlibs = [(name, orb_slam2_amd.lib(path)) for name, path in variants]
    for n in (50, 100, 300):
        for share in (0.0, 0.3):
            for fix in (0, 1):
                cams, S12, pairs, th2, fx, _ = Cs.make(n, share, bool(fix), 1, scale=1.7, noise=0.5)
                Q, keep, one = record(L, cams, S12, pairs, th2, fx)
                key = f"single_n{n}_o{int(share * 100)}_f{fix}"
                res[key] = timed([one], a.calls)[0]
                Sm, rm, nm, tr = M.optimize_sim3(cams, S12, pairs, th2, fx, want_trace=True)      # the timed answers are the right ones
                assert np.array_equal(keep[1], rm) and Q.n_inliers == nm, key
                res[key].update(inliers=nm, second_phase_iterations_allowed=tr["second_iterations"], lm_iterations=tr["iterations"], lm_trials=tr["accepted"] + tr["rejected"])
                if vlibs and n >= 100 and not fix:
                    recs = [record(lib, cams, S12, pairs, th2, fx) for _, lib in vlibs]
                    t = timed([one] + [r[2] for r in recs], a.calls)
                    res.setdefault("variants", {})[key] = {"shipped": t[0]}
                    for (name, _), r, tv in zip(vlibs, recs, t[1:]):
                        assert np.array_equal(r[1][1], keep[1]) and r[0].n_inliers == Q.n_inliers, (key, name)
                        assert name.startswith("T") or bytes(r[0].S12_out) == bytes(Q.S12_out), (key, name)      # (another workgroup size is another order of the sums)
                        res["variants"][key][name] = tv
    if vlibs:
        res["variants"]["note"] = "timed call by call in turn with the shipped library on the same problem; every variant's flags and return value equal the shipped library's, and so does S12_out bit for bit except under another workgroup size (T...)"
    for nb in (4, 16):
        batch = [Cs.make(100, 0.3, False, 10 + k, scale=1.7, noise=0.5) for k in range(nb)]
        recs = [record(L, *b[:5]) for b in batch]
        arr = (_Sim3OptProblem * nb)()
        for k, r in enumerate(recs):
            C.memmove(C.byref(arr[k]), C.byref(r[0]), C.sizeof(_Sim3OptProblem))

        def one_batch():
            assert L.orbhip_sim3_optimize_batch(0, nb, C.cast(arr, C.c_void_p)) == 0, L.orbhip_last_error()

        def loop():
            for r in recs:
                r[2]()
        tb, tl = timed([one_batch, loop], a.calls)
        for k, r in enumerate(recs):
            assert bytes(arr[k].S12_out) == bytes(r[0].S12_out) and arr[k].n_inliers == r[0].n_inliers
        res[f"batch_{nb}x100"] = dict(tb, loop_of_single_calls=tl, batch_over_loop=tb["ms_median"] / tl["ms_median"])
    cam, T0, obs, _ = Pc.make(300, "mixed", 0.2, 1)
    obs_s = orb_slam2_amd.orbhip._pose_obs(obs)
    T0 = np.ascontiguousarray(T0)
    out, flags, ninl = np.zeros(16, np.float32), np.zeros(300, np.uint8), C.c_int(0)

    def pose():
        assert L.orbhip_pose_optimization(0, p(cam), p(T0), p(obs_s), 300, p(out), p(flags), C.byref(ninl)) == 0, L.orbhip_last_error()
    res["yardstick_pose_optimization_n300"] = timed([pose], a.calls)[0]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
