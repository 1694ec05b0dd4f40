#!/usr/bin/env python3
"""Milliseconds per call of PnPsolver::iterate on the device (orbhip_pnp_iterate and its batch form).

    python tools/pnp_rate.py [--calls 30] [--out profiles/pnp_rate.json]                 on the MI355X

Workloads (tests/pnp_cases.py scenes: 30 % wrong matches, noise 0.5 px at level 0; quadruples drawn as the solver draws them):
  * one solver x 5 and x 300 hypotheses at n = 100 and n = 300 correspondences, min_inliers = n (out of reach): every hypothesis is consumed and
    nothing is refined;
  * a call that refines: one solver x 300 at n = 300 with min_inliers = 0.5 n, which returns a refined pose;
  * batches of 4 and of 16 solvers x 300 hypotheses at n = 300 (minimum out of reach), against the loop of single calls over the same problems
    timed in the same run.  The criterion is relative: a batch must cost less than its loop.
Each figure is the median wall time of --calls synchronous calls of the C ABI on prepared problem records (upload, four launches, download) after three
warm-up calls, with the minimum and the share orbhip_thread_api_ms attributes to the library; the clock is time.perf_counter.  The timed answers are
compared with tests/pnp_model.py first (bit for bit).
NO REFERENCE FIGURE exists: the reference's class needs OpenCV's legacy C API (cvSVD, cvSolve, cvInvert, cvMulTransposed), which the OpenCV stand-in
this project is developed against does not have, so it cannot be built there; no ratio to it is claimed, and the file says so.  A device that is
missing is an error."""
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
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import orb_slam2_amd
    from orb_slam2_amd import orbhip as OH
    import pnp_cases as Cs
    import pnp_checks as K
    L = orb_slam2_amd.lib()
    if L.orbhip_device_count() < 1:
        sys.exit("no HIP device: the figures are measured on an MI355X or not at all")
    res = {"workload": "tests/pnp_cases.py scene(n, seed, 0.3, 0.5): 1 x 5 and 1 x 300 at n = 100 and 300 with the minimum out of reach, one refining call (1 x 300, n = 300, "
                       "min 150), batches of 4 and 16 solvers x 300 at n = 300 against the loop of single calls",
           "reference": "none: PnPsolver needs cvSVD, cvSolve, cvInvert and cvMulTransposed, absent from the OpenCV stand-in, and could not be built where this was measured - "
                        "no ratio is claimed",
           "machine": "MI355X box", "runtime": str(orb_slam2_amd.runtime_info())}

    def problem(n, n_hyp, seed, mi):
        return dict(K=Cs.K, corr=Cs.scene(n, seed, 0.3, 0.5)[0], quads=Cs.draw_quads(n, n_hyp, seed), min_inliers=mi)

    def records(probs):
        arr = (OH._PnpProblem * len(probs))()
        return arr, [OH._pnp_fill(arr[k], q, False) for k, q in enumerate(probs)]

    def check(q):                                                               # the timed answers are the right ones
        d = K.device(q["corr"], q["quads"], q["min_inliers"])
        assert K.differences(d, K.model(q["corr"], q["quads"], q["min_inliers"])) == []
        return d

    for n, n_hyp, key in ((100, 5, "single_5_n100"), (100, 300, "single_300_n100"), (300, 5, "single_5_n300"), (300, 300, "single_300_n300")):
        q = problem(n, n_hyp, 1, n)
        arr, keep = records([q])

        def one():
            assert L.orbhip_pnp_iterate(0, C.byref(arr[0])) == 0, L.orbhip_last_error()
        res[key] = timed(L, one, a.calls)
        d = check(q)
        assert arr[0].n_consumed == n_hyp == d["n_consumed"] and arr[0].returned == -1
    q = problem(300, 300, 1, 150)
    arr, keep = records([q])

    def refining():
        assert L.orbhip_pnp_iterate(0, C.byref(arr[0])) == 0, L.orbhip_last_error()
    res["refining_300_n300"] = timed(L, refining, a.calls)
    d = check(q)
    assert arr[0].returned >= 0 and arr[0].returned == d["returned"]
    res["refining_300_n300"].update(returned=int(d["returned"]), refined_inliers=int(d["refined_inliers"]))
    for count in (4, 16):
        arr, keep = records([problem(300, 300, 10 + k, 300) for k in range(count)])

        def batch():
            assert L.orbhip_pnp_iterate_batch(0, count, C.cast(arr, C.c_void_p)) == 0, L.orbhip_last_error()

        def loop():
            for k in range(count):
                assert L.orbhip_pnp_iterate(0, C.byref(arr[k])) == 0, L.orbhip_last_error()
        res[f"batch_{count}x300_n300"] = timed(L, batch, a.calls)
        res[f"loop_{count}x300_n300"] = timed(L, loop, a.calls)
        res[f"batch_{count}x300_n300"]["loop_over_batch"] = res[f"loop_{count}x300_n300"]["ms_median"] / res[f"batch_{count}x300_n300"]["ms_median"]
    res["criterion"] = {"batch_16_cheaper_than_loop": bool(res["batch_16x300_n300"]["ms_median"] < res["loop_16x300_n300"]["ms_median"])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
