#!/usr/bin/env python3
"""Rate of the device key-frame database (orbhip_kfdb_*): milliseconds per call and scanned bytes / time as a fraction of the HBM peak.

    python tools/kfdb_rate.py [--kfs 10000] [--words 1500] [--reps 30] [--scoring 0] [--out profiles/NAME.json]

Two measurements:
  query       orbhip_kfdb_query (RELOC) of a 1500-word BowVector against --kfs key frames of about --words words each, nwords = 10^6
  reloc       the full relocalisation sequence on a resident frame: compute_bow -> query_frame -> select, with the vocabulary of tests/golden (216 words:
              the only vocabulary file this repository carries; the key frames then hold at most 216 words each, the count is the same)
--scoring: the scoring object of the `query` measurement (orbhip_kfdb_set_scoring: 0 L1, 1 L2, 2 chi-square, 4 Bhattacharyya, 5 dot product), with BowVectors
normalised as that scoring's transform leaves them; the `reloc` sequence runs under the vocabulary file's own scoring.
Every timed call is synchronous: it returns behind a synchronise of its stream, after the device has delivered the hits.
Scanned bytes = the word ids of every live key frame (4 B each) + the slot records: what k_kfdb_scan must read; weights are read for shared words only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import orb_slam2_amd                                                       # noqa: E402
from orb_slam2_amd import synth                                            # noqa: E402

HBM_PEAK = 8.0e12                                                          # MI355X, bytes / s


def bow(rng, nwords, n):
    ids = np.unique(rng.choice(nwords, n, replace=False)).astype(np.uint32)
    v = rng.random(len(ids)) + 1e-3
    return ids, v / v.sum()


def normalise(scoring, v):
    """ScoringObject.h:73-90: L2 for L2_NORM, none for DOT_PRODUCT, L1 otherwise"""
    return v / np.sqrt(np.sum(v * v)) if scoring == 1 else v if scoring == 5 else v / v.sum()


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kfs", type=int, default=10000)
    ap.add_argument("--words", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--scoring", type=int, default=0, choices=[0, 1, 2, 4, 5])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    res = {"kfs": a.kfs, "words": a.words, "scoring": a.scoring}
    # ---- query
    nwords = 10**6
    pool = rng.choice(nwords, 20 * a.words, replace=False)                  # the key frames and the query draw from one pool: they share words
    db = orb_slam2_amd.KeyFrameDatabase(nwords)
    db.set_scoring(a.scoring)
    total = 0
    t0 = time.perf_counter()
    for k in range(a.kfs):
        ids = np.unique(rng.choice(pool, int(a.words * rng.uniform(0.8, 1.2)), replace=False)).astype(np.uint32)
        v = rng.random(len(ids)) + 1e-3
        db.add(ids, normalise(a.scoring, v)); total += len(ids)
    res["add_ms_per_key_frame"] = (time.perf_counter() - t0) * 1e3 / a.kfs
    q = np.unique(rng.choice(pool, a.words, replace=False)).astype(np.uint32)
    qv = normalise(a.scoring, rng.random(len(q)) + 1e-3)
    qid = [1]

    def one():
        qid[0] += 1
        return db.query(orb_slam2_amd.KFDB_RELOC, qid[0], q, qv)
    hits, nsharing, minc = one()
    med, best = timed(one, a.reps)
    scanned = 4 * total + 24 * a.kfs
    res["query"] = {"ms_median": med, "ms_min": best, "scanned_bytes": scanned, "fraction_of_hbm_peak": scanned / (med * 1e-3) / HBM_PEAK,
                    "nsharing": int(nsharing), "nhits": int(len(hits)), "min_common": int(minc)}
    db.close()
    # ---- the full RELOC sequence on a resident frame
    voc = orb_slam2_amd.ORBVocabulary(os.path.join(ROOT, "tests", "golden", "voc_k6_L3_ref.txt"))
    w, h = 640, 480
    ex = orb_slam2_amd.ORBextractor(1000, 1.2, 8, 20, 7, w, h, max_batch=1)
    ex.extract_batch([synth.frame(w, h, seed=5)])
    db = orb_slam2_amd.KeyFrameDatabase(voc.size())
    total = 0
    for k in range(a.kfs):
        b = bow(rng, voc.size(), int(rng.integers(60, 200)))
        db.add(*b); total += len(b[0])
    neigh_of = rng.integers(0, a.kfs, (a.kfs, 10)).astype(np.int32)

    def seq():
        qid[0] += 1
        voc.compute_bow(ex, 1, levelsup=4)
        hits, ns, mc = db.query_frame(orb_slam2_amd.KFDB_RELOC, qid[0], ex, voc, frame=0)
        return db.select(orb_slam2_amd.KFDB_RELOC, qid[0], mc, hits, [neigh_of[int(s)] for s in hits["slot"]]), len(hits)
    cand, nh = seq()
    med, best = timed(seq, a.reps)
    res["reloc_sequence"] = {"ms_median": med, "ms_min": best, "key_frame_words": total, "nhits": int(nh), "ncandidates": int(len(cand)), "vocabulary_words": voc.size()}
    orb_slam2_amd.orbhip.device_synchronize(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
