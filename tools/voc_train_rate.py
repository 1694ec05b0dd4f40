#!/usr/bin/env python3
"""Time of DBoW2's TemplatedVocabulary::create on one training set: the device call, and the reference's own create() on one thread of a host.

    python tools/voc_train_rate.py [--calls 5] [--out profiles/voc_train_rate.json]                  on the MI355X: orbhip_voc_create
    python tools/voc_train_rate.py --reference /path/to/ORB_SLAM2 --out profiles/voc_train_rate.json   on a host that has the reference's sources: its create(),
                                                                                                     driven through tests/voc_train_harness.py; MERGED into --out

The workload: k = 10, L = 6, TF_IDF / L1_NORM, 400 000 descriptors in 400 images of 1000, drawn from 3000 random prototypes with 20 % of the bits flipped
(seed 7), base seed 3 for the per-node random streams (with base seeds 1 and 2 a cluster empties and the reference faults).  The device figure is the median wall time of --calls calls of the C ABI on host arrays (upload,
every level, weights, download) after one warm-up call on a small set, with the per-level device times the library reports for the last call; the reference figure is the time inside create() alone.  Each run records
the SHA-256 of the vocabulary file it saved: when both figures are in the file, `same_file` says whether the two machines built the same vocabulary.  The
two figures come from different machines and the file says which.  A device that is missing is an error."""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
K, DEPTH, SEED = 10, 6, 3
WORKLOAD = "k = 10, L = 6, TF_IDF, L1_NORM; 400000 descriptors in 400 images of 1000: 3000 random prototypes, 20 % of the bits flipped (seed 7); base seed 3 (the reference faults on base seeds 1 and 2: an empty cluster, DESIGN.md H14)"


def workload():
    import voc_train_model as M
    return M.make_set(7, [1000] * 400, 3000, 0.2)


def cpu_name():
    return next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "unknown")


def device(calls):
    import orb_slam2_amd
    import voc_train_model as M
    if orb_slam2_amd.lib().orbhip_device_count() < 1:
        sys.exit("no HIP device: the device figure is measured on an MI355X or not at all")
    orb_slam2_amd.ORBVocabulary.create(M.make_set(1, [300] * 4, 40, 0.2), 5, 2)         # warm-up: the runtime's first launches are not the routine's
    imgs = workload()
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        v = orb_slam2_amd.ORBVocabulary.create(imgs, K, DEPTH, 0, 0, SEED)
        wall.append(time.perf_counter() - t0)
    with tempfile.TemporaryDirectory() as tmp:
        v.saveToTextFile(os.path.join(tmp, "voc.txt"))
        sha = hashlib.sha256(open(os.path.join(tmp, "voc.txt"), "rb").read()).hexdigest()
    info = orb_slam2_amd.runtime_info()
    return {"seconds": float(np.median(wall)), "seconds_min": float(np.min(wall)), "calls": calls, "level_kernel_ms": [float(x) for x in v.level_ms], "weights_kernel_ms": v.weights_ms, "descriptors": int(sum(len(f) for f in imgs)),
            "nodes": v.nnodes, "words": v.nwords, "words_without_documents": int((v.word_docs == 0).sum()), "file_sha256": sha, "machine": "MI355X box", "host_cpu": cpu_name(),
            "runtime": info if isinstance(info, str) else str(info)}


def reference(ref):
    import voc_train_harness as H
    imgs = workload()
    with tempfile.TemporaryDirectory() as tmp:
        lib = H.build(tmp, ref, opt="-O3")
        r = H.train_isolated(lib, imgs, K, DEPTH, 0, 0, SEED, text_path=os.path.join(tmp, "voc.txt"))
    if r is None:
        sys.exit("the reference faulted on the workload")
    return {"seconds": r["seconds"], "threads": 1, "descriptors": int(sum(len(f) for f in imgs)), "nodes": int(len(r["parent"])), "words": int(len(r["ni"])),
            "file_sha256": hashlib.sha256(r["text"]).hexdigest(), "machine": "a DIFFERENT host from the device figure's", "cpu": cpu_name(),
            "what": "the reference's own TemplatedVocabulary::create (g++ -O3), its k-means++ stream reseeded per node by the harness's subclass"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if a.out and os.path.exists(a.out):
        res = json.loads(open(a.out).read())
    res["workload"] = WORKLOAD
    if a.reference:
        res["reference_create_on_host"] = reference(a.reference)
    else:
        res["device_call"] = device(a.calls)
    if "device_call" in res and "reference_create_on_host" in res:
        res["same_file"] = res["device_call"]["file_sha256"] == res["reference_create_on_host"]["file_sha256"]
    res["note"] = "device_call and reference_create_on_host were measured on different machines; no ratio between them is claimed beyond these two figures"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
