#!/usr/bin/env python3
"""Time of MapPoint::ComputeDistinctiveDescriptors over one key frame's map points: the device call, and the reference's member on a host.

    python tools/distinct_rate.py [--calls 30] [--out profiles/distinct_rate.json]                on the MI355X: orbhip_distinctive_descriptors
    python tools/distinct_rate.py --reference /path/to/ORB_SLAM2 --out profiles/distinct_rate.json   on a host that has the reference's sources: its member,
                                                                                                  one thread; the result is MERGED into --out

The workload: 2000 groups (map points); 70 % hold 2-10 descriptors, 25 % 11-40, 5 % 41-64, and three groups hold 300 (seed 1).  The device figure is the
median wall time of --calls calls of the C ABI on host arrays (upload, both kernels, download) after two warm-up calls, with the share
orbhip_thread_api_ms attributes to the library.  The reference figure is the wall time of a C loop over the points calling the member (median of --calls
passes), on whatever CPU the tool runs on: the two figures come from different machines and the file says which.  A device that is missing is an error."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MIX = "2000 groups: 70 % of 2-10 descriptors, 25 % of 11-40, 5 % of 41-64, plus three groups of 300 (seed 1)"


def workload(seed=1):
    rng = np.random.default_rng(seed)
    u = rng.random(2000)
    sizes = np.where(u < 0.70, rng.integers(2, 11, 2000), np.where(u < 0.95, rng.integers(11, 41, 2000), rng.integers(41, 65, 2000)))
    sizes[rng.choice(2000, 3, replace=False)] = 300
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    desc = np.zeros((off[-1], 32), np.uint8)
    for g in range(2000):                                                     # observations of one point: one descriptor with about 12 % of its bits flipped
        base = np.unpackbits(rng.integers(0, 256, 32, dtype=np.uint8))
        desc[off[g]:off[g + 1]] = np.packbits(base[None] ^ (rng.random((sizes[g], 256)) < 0.12), axis=1)
    return desc, off


def device(calls):
    import orb_slam2_amd
    L = orb_slam2_amd.lib()
    if L.orbhip_device_count() < 1:
        sys.exit("no HIP device: the device figure is measured on an MI355X or not at all")
    desc, off = workload()
    n = len(off) - 1
    bi, bm = np.zeros(n, np.int32), np.zeros(n, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def one():
        st = L.orbhip_distinctive_descriptors(0, p(desc), p(off), n, p(bi), p(bm))
        assert st == 0, L.orbhip_last_error()
    one(); one()
    wall, api = [], []
    for _ in range(calls):
        L.orbhip_thread_api_ms(1)
        t0 = time.perf_counter(); one(); wall.append((time.perf_counter() - t0) * 1e3)
        api.append(L.orbhip_thread_api_ms(0))
    import distinct_model as M                                                # the timed answers are the right ones (a sample of the groups; all the large ones)
    sizes = np.diff(off)
    for g in list(range(0, n, 40)) + [int(x) for x in np.flatnonzero(sizes > 64)]:
        assert (int(bi[g]), int(bm[g])) == M.best(desc[off[g]:off[g + 1]]), g
    info = orb_slam2_amd.runtime_info()
    return {"ms_median": float(np.median(wall)), "ms_min": float(np.min(wall)), "library_share": float(np.median(api) / np.median(wall)), "calls": calls,
            "descriptors": int(off[-1]), "distance_pairs": int((sizes.astype(np.int64) ** 2).sum()), "machine": "MI355X box", "runtime": info if isinstance(info, str) else str(info)}


def reference(ref, calls):
    import distinct_harness as H
    desc, off = workload()
    sizes = np.diff(off)
    nkf = int(sizes.max())
    with tempfile.TemporaryDirectory() as tmp:
        lib = H.build(tmp, reference=ref)
        # point g is observed in key frames 0 .. sizes[g]-1, row g' of each = its own descriptor there
        rows = [[] for _ in range(nkf)]
        obs = []
        for g in range(len(sizes)):
            r = []
            for k in range(sizes[g]):
                r.append(len(rows[k])); rows[k].append(off[g] + k)
            obs.append(r)
        order = np.array([i for r in rows for i in r])
        w = H.World(lib, [len(r) for r in rows], desc[order], np.zeros(nkf, np.uint8))
        for g in range(len(sizes)):
            w.point(desc[off[g]], np.arange(sizes[g]), obs[g])
        pts = np.arange(len(sizes))
        w.member(pts)
        ms = [w.member(pts) for _ in range(calls)]
        w.close()
    cpu = next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "unknown")
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "calls": calls, "threads": 1, "machine": "a DIFFERENT host from the device figure's", "cpu": cpu,
            "what": "the reference's own src/MapPoint.cc (g++ -O1) called point after point from a C loop, key-frame stand-ins of tests/distinct/"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if a.out and os.path.exists(a.out):
        res = json.loads(open(a.out).read())
    res["workload"] = MIX
    if a.reference:
        res["reference_member_on_host"] = reference(a.reference, a.calls)
    else:
        res["device_call"] = device(a.calls)
    res["note"] = "device_call and reference_member_on_host were measured on different machines; no ratio between them is claimed beyond these two figures"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
