#!/usr/bin/env python3
"""Milliseconds per call of Sim3Solver::iterate on the device (orbhip_sim3_iterate and its batch form).

    python tools/sim3_rate.py [--calls 50] [--out profiles/sim3_rate.json]                on the MI355X

Workloads (tests/sim3_cases.py scenes: 1 px noise, 20 % wrong matches, free scale 1.3, gemm mode 0; triples drawn ungated, min_inliers above every
count so that every hypothesis is consumed):
  * one solver x 5 hypotheses (LoopClosing's iterate(5)) at n = 100 and n = 300 correspondences;
  * find(): one solver x 300 hypotheses at n = 300;
  * batches of 4 and of 16 solvers x 5 hypotheses at n = 300, against the loop of single calls over the same problems timed in the same run.
Each figure is the median wall time of --calls synchronous calls of the C ABI on prepared problem records (upload, two launches, download) after three
warm-up calls, with the minimum and the share orbhip_thread_api_ms attributes to the library; the clock is time.perf_counter.  The timed answers are
compared with tests/sim3_model.py first (everything after Horn exactly, from the kernel's own R, t, s).
NO REFERENCE FIGURE exists: the reference's class needs cv::eigen and cv::Rodrigues, which the OpenCV stand-in this project is developed against does
not have, so it cannot be built there; no ratio is claimed, and the file says so.  A device that is missing is an error."""
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
    from orb_slam2_amd import orbhip as OH
    import sim3_cases as Cs
    import sim3_checks as K
    L = orb_slam2_amd.lib()
    if L.orbhip_device_count() < 1:
        sys.exit("no HIP device: the figures are measured on an MI355X or not at all")
    res = {"workload": "tests/sim3_cases.py scene(n, 1.3, seed), free scale, gemm mode 0, every hypothesis consumed: 1 x 5 at n = 100 and 300, find = 1 x 300 at n = 300, "
                       "batches of 4 and 16 solvers x 5 at n = 300 against the loop of single calls",
           "reference": "none: Sim3Solver needs cv::eigen and cv::Rodrigues, absent from the OpenCV stand-in, and could not be built where this was measured - no ratio is claimed",
           "machine": "MI355X box", "runtime": str(orb_slam2_amd.runtime_info())}

    def records(n, n_hyp, count, seed0):
        arr = (OH._Sim3Problem * count)()
        keep = []
        for k in range(count):
            corr, _ = Cs.scene(n, 1.3, seed0 + k)
            tri = Cs.draw_triples(corr, n_hyp, seed0 + k, gate=False)
            keep.append(OH._sim3_fill(arr[k], dict(K1=Cs.K1, K2=Cs.K2, corr=corr, triples=tri, fix_scale=False, gemm_mode=0, min_inliers=n, best_inliers_in=0), False))
        return arr, keep

    def check(n, n_hyp, seed):                                                  # the timed answers are the right ones
        corr, _ = Cs.scene(n, 1.3, seed)
        tri = Cs.draw_triples(corr, n_hyp, seed, gate=False)
        d = K.device(corr, tri, False, 0, n)
        K.after_horn_exact(d, corr, tri, 0, n, 0)
        return int(d["best_inliers_out"])

    for n, n_hyp, key in ((100, 5, "single_5_n100"), (300, 5, "single_5_n300"), (300, 300, "find_300_n300")):
        arr, keep = records(n, n_hyp, 1, 1)

        def one():
            assert L.orbhip_sim3_iterate(0, C.byref(arr[0])) == 0, L.orbhip_last_error()
        res[key] = timed(L, one, a.calls)
        res[key]["best_inliers"] = check(n, n_hyp, 1)
        assert arr[0].n_consumed == n_hyp and arr[0].best_inliers_out == res[key]["best_inliers"]
    for count in (4, 16):
        arr, keep = records(300, 5, count, 10)

        def batch():
            assert L.orbhip_sim3_iterate_batch(0, count, C.cast(arr, C.c_void_p)) == 0, L.orbhip_last_error()

        def loop():
            for k in range(count):
                assert L.orbhip_sim3_iterate(0, C.byref(arr[k])) == 0, L.orbhip_last_error()
        res[f"batch_{count}x5_n300"] = timed(L, batch, a.calls)
        res[f"loop_{count}x5_n300"] = timed(L, loop, a.calls)
        res[f"batch_{count}x5_n300"]["loop_over_batch"] = res[f"loop_{count}x5_n300"]["ms_median"] / res[f"batch_{count}x5_n300"]["ms_median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
