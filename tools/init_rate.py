#!/usr/bin/env python3
"""Milliseconds per call of Initializer::Initialize on the device (orbhip_init_reconstruct and its batch form).

    python tools/init_rate.py [--calls 50] [--out profiles/init_rate.json]                 on the MI355X

Workloads (tests/init_cases.py scenes: 10 % gross outliers, noise 0.5 px; 200 sets drawn as the initialiser draws them):
  * a general 3-D scene at n = 100, 300, 1000 and 2000 matches (reconstructs from F where it reconstructs) and a tilted plane at n = 300
    (reconstructs from H);
  * batches of 4 and of 16 frame pairs at n = 300 (general scenes of different seeds), against the loop of single calls over the same problems
    timed in the same run.
Each figure is the median wall time of --calls synchronous calls of the C ABI on prepared problem records (one upload, four launches, one download:
the call ends in a device synchronise) after five warm-up calls of the same shape, with the minimum, the 10th and 90th percentiles (the spread of the
run) and the share orbhip_thread_api_ms attributes to the library; the clock is time.perf_counter.  A batch and its loop take turns call by call.  A
call lasts a quarter of a millisecond, so a figure rests on some 12 ms of work: it says what a call costs, not what a busy device sustains.  The timed answers are compared with tests/init_model.py first (bit for bit).  Nothing is asserted
about the times.
NO REFERENCE FIGURE exists: the reference's class needs cv::SVDecomp, Mat::inv, cv::determinant and cv::norm, which the OpenCV stand-in this project
is developed against does not have, so it cannot be built there; no ratio to it is claimed, and the file says so.  A device that is missing is an
error."""
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


def stats(wall, api, calls):
    return {"ms_median": float(np.median(wall)), "ms_min": float(np.min(wall)), "ms_p10": float(np.percentile(wall, 10)), "ms_p90": float(np.percentile(wall, 90)),
            "library_share": float(np.median(api) / np.median(wall)), "calls": calls}


def timed(L, fns, calls):
    """the functions take turns, call by call, so that what else the host and the device are doing meets all of them alike; one stats dict each"""
    for _ in range(5):
        for fn in fns:
            fn()
    wall, api = [[] for _ in fns], [[] for _ in fns]
    for _ in range(calls):
        for k, fn in enumerate(fns):
            L.orbhip_thread_api_ms(1)
            t0 = time.perf_counter(); fn(); wall[k].append((time.perf_counter() - t0) * 1e3)
            api[k].append(L.orbhip_thread_api_ms(0))
    return [stats(wall[k], api[k], calls) for k in range(len(fns))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import orb_slam2_amd
    from orb_slam2_amd import orbhip as OH
    import init_cases as Cs
    import init_checks as K
    L = orb_slam2_amd.lib()
    if L.orbhip_device_count() < 1:
        sys.exit("no HIP device: the figures are measured on an MI355X or not at all")
    res = {"workload": "tests/init_cases.py scenes, 200 sets: general 3-D at n = 100, 300, 1000, 2000; a tilted plane at n = 300; batches of 4 and 16 general scenes at "
                       "n = 300 against the loop of single calls",
           "reference": "none: Initializer needs cv::SVDecomp, Mat::inv, cv::determinant and cv::norm, absent from the OpenCV stand-in, and could not be built where this was "
                        "measured - no ratio is claimed",
           "runtime": str(orb_slam2_amd.runtime_info())}

    def problem(kind, n, seed, **opt):
        name = "rate_%s_%d_%d" % (kind, n, seed)
        Cs.SCENES[name] = (kind, n, 200, seed, opt)
        return Cs.arguments(Cs.case(name))

    def records(probs):
        arr = (OH._InitProblem * len(probs))()
        return arr, [OH._init_fill(arr[k], q, False) for k, q in enumerate(probs)]

    def check(q):                                                               # the timed answers are the right ones
        d = K.device(q)
        assert K.differences(d, K.model(q)) == []
        return d

    for kind, n, key, opt in (("general", 100, "general_n100", {}), ("general", 300, "general_n300", {}), ("general", 1000, "general_n1000", {}),
                              ("general", 2000, "general_n2000", {}), ("plane", 300, "plane_n300", dict(tilt=1.4))):
        q = problem(kind, n, 41, **opt)
        arr, keep = records([q])

        def one():
            assert L.orbhip_init_reconstruct(0, C.byref(arr[0])) == 0, L.orbhip_last_error()
        res[key] = timed(L, [one], a.calls)[0]
        d = check(q)
        res[key].update(returned=d["returned"], model=d["model"], triangulated=int(d["triangulated"].sum()))
        print(key, res[key], flush=True)
    for nb in (4, 16):
        probs = [problem("general", 300, 50 + k) for k in range(nb)]
        arr, keep = records(probs)

        def batch():
            assert L.orbhip_init_reconstruct_batch(0, nb, C.cast(arr, C.c_void_p)) == 0, L.orbhip_last_error()

        def loop():
            for k in range(nb):
                assert L.orbhip_init_reconstruct(0, C.byref(arr[k])) == 0, L.orbhip_last_error()
        kb, kl = "batch_%dx_n300" % nb, "loop_%dx_n300" % nb
        res[kb], res[kl] = timed(L, [batch, loop], a.calls)
        res[kb]["loop_over_batch"] = res[kl]["ms_median"] / res[kb]["ms_median"]
        for q, dv in zip(probs[:2], orb_slam2_amd.init_reconstruct_batch(probs[:2], per_hypothesis=True)):
            assert K.differences(dv, K.model(q)) == []
        print(kb, res[kb], kl, res[kl], flush=True)
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
