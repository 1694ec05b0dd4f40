#!/usr/bin/env python3
"""Rate of the device key-frame database (orbhip_kfdb_*): milliseconds per call and scanned bytes / time as a fraction of the HBM peak.

    python tools/kfdb_rate.py [--kfs 10000] [--words 1500] [--reps 30] [--scoring 0] [--out profiles/NAME.json]
    python tools/kfdb_rate.py --batch [Q1,Q2,...] [--out profiles/kfdb_batch_rate.json]       the batched entries (below)

Two measurements:
  query       orbhip_kfdb_query (RELOC) of a 1500-word BowVector against --kfs key frames of about --words words each, nwords = 10^6
  reloc       the full relocalisation sequence on a resident frame: compute_bow -> query_frame -> select, with the vocabulary of tests/golden (216 words:
              the only vocabulary file this repository carries; the key frames then hold at most 216 words each, the count is the same)
--scoring: the scoring object of the `query` measurement (orbhip_kfdb_set_scoring: 0 L1, 1 L2, 2 chi-square, 4 Bhattacharyya, 5 dot product), with BowVectors
normalised as that scoring's transform leaves them; the `reloc` sequence runs under the vocabulary file's own scoring.
Every timed call is synchronous: it returns behind a synchronise of its stream, after the device has delivered the hits.
--batch (default 1,8,64,512): per batch size Q, orbhip_kfdb_query_batch of Q different 1500-word queries against the same database, and IN THE SAME RUN the loop
of Q single orbhip_kfdb_query calls of the same queries; both through the C ABI with the arrays prepared beforehand.  Required bytes of a batch = the key
frames' word ids and slot records once per TILE of the scan's plan (at most 16 queries and 8192 ids a tile); the queries' own ids, staged
once per workgroup, are not counted.  Then the resident sequence compute_bow -> query_frames -> select_batch beside the single one.
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


def tiles(lengths, max_q=16, max_ids=8192):
    """the scan's tile plan (kf_batch_core): consecutive queries while their ids fit"""
    n, nq, ids = 1, 0, 0
    for l in lengths:
        if nq and (nq == max_q or ids + l > max_ids):
            n, nq, ids = n + 1, 0, 0
        nq, ids = nq + 1, ids + l
    return n


def batch_main(a):
    import ctypes as C
    KF = orb_slam2_amd
    L = KF.lib()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    sizes = [int(x) for x in a.batch.split(",")]
    rng = np.random.default_rng(1)
    res = {"kfs": a.kfs, "words": a.words, "scoring": a.scoring, "batch": {}}
    nwords = 10**6
    pool = rng.choice(nwords, 20 * a.words, replace=False)
    db = KF.KeyFrameDatabase(nwords)
    db.set_scoring(a.scoring)
    total = 0
    for k in range(a.kfs):
        ids = np.unique(rng.choice(pool, int(a.words * rng.uniform(0.8, 1.2)), replace=False)).astype(np.uint32)
        db.add(ids, normalise(a.scoring, rng.random(len(ids)) + 1e-3)); total += len(ids)
    qmax = max(sizes)
    bows = []
    for i in range(qmax):
        q = np.unique(rng.choice(pool, a.words, replace=False)).astype(np.uint32)
        bows.append((q, normalise(a.scoring, rng.random(len(q)) + 1e-3)))
    once = 4 * total + 24 * a.kfs
    next_id = [1]
    hits = np.zeros(qmax * a.kfs, KF.KFDB_HIT)
    for Q in sizes:
        boff = np.concatenate([[0], np.cumsum([len(b[0]) for b in bows[:Q]])]).astype(np.int32)
        bid, bval = np.concatenate([b[0] for b in bows[:Q]]), np.concatenate([b[1] for b in bows[:Q]])
        hit_off, ns, mc, tok, n1, ns1, mc1 = np.zeros(Q + 1, np.int32), np.zeros(Q, np.int32), np.zeros(Q, np.int32), C.c_uint64(0), C.c_int(0), C.c_int(0), C.c_int(0)
        got = {}

        def batch():
            qids = np.arange(next_id[0], next_id[0] + Q, dtype=np.uint64); next_id[0] += Q
            st = L.orbhip_kfdb_query_batch(db.h, 0, Q, p(qids), p(boff), p(bid), p(bval), None, None, None, p(hit_off), p(ns), p(mc), p(hits), len(hits), C.byref(tok))
            assert st == 0, L.orbhip_last_error()
            got["batch"] = hits[:hit_off[Q]].tobytes()

        def singles():
            out = []
            for i in range(Q):
                st = L.orbhip_kfdb_query(db.h, 0, next_id[0], p(bows[i][0]), p(bows[i][1]), len(bows[i][0]), None, 0, 0.0, p(hits), a.kfs, C.byref(n1), C.byref(ns1), C.byref(mc1))
                assert st == 0, L.orbhip_last_error()
                next_id[0] += 1
                out.append(hits[:n1.value].tobytes())
            got["singles"] = b"".join(out)

        reps = max(3, min(a.reps, 2000 // Q))
        bm, bb = timed(batch, reps)
        sm, sb = timed(singles, reps)
        assert got["batch"] == got["singles"], "the batch and the single calls disagree"
        nt = tiles([len(b[0]) for b in bows[:Q]])
        need = nt * once
        res["batch"][str(Q)] = {"reps": reps, "batch_ms_median": bm, "batch_ms_min": bb, "batch_ms_per_query_median": bm / Q, "batch_ms_per_query_min": bb / Q,
                                "singles_ms_median": sm, "singles_ms_min": sb, "singles_ms_per_query_median": sm / Q, "ratio_singles_over_batch_median": sm / bm,
                                "tiles": nt, "required_bytes": need, "fraction_of_hbm_peak": need / (bm * 1e-3) / HBM_PEAK, "nhits": int(hit_off[Q])}
    db.close()
    # ---- the resident sequence: compute_bow -> query_frames -> select_batch, beside compute_bow -> query_frame -> select per frame
    Q = min(64, qmax)
    voc = KF.ORBVocabulary(os.path.join(ROOT, "tests", "golden", "voc_k6_L3_ref.txt"))
    w, h = 640, 480
    ex = KF.ORBextractor(1000, 1.2, 8, 20, 7, w, h, max_batch=Q)
    ex.extract_batch([synth.frame(w, h, seed=5 + f) for f in range(Q)])
    db = KF.KeyFrameDatabase(voc.size())
    for k in range(a.kfs):
        db.add(*bow(rng, voc.size(), int(rng.integers(60, 200))))
    neigh_of = rng.integers(0, a.kfs, (a.kfs, 10)).astype(np.int32)

    def seq_batch():
        qids = np.arange(next_id[0], next_id[0] + Q, dtype=np.uint64); next_id[0] += Q
        voc.compute_bow(ex, Q, levelsup=4)
        b = db.query_frames(KF.KFDB_RELOC, qids, ex, voc, first_frame=0)
        return db.select_batch(b, neigh_of[b.hits["slot"]]), len(b.hits)

    def seq_single():
        voc.compute_bow(ex, Q, levelsup=4)
        out = []
        for f in range(Q):
            next_id[0] += 1
            hits1, _, mc0 = db.query_frame(KF.KFDB_RELOC, next_id[0], ex, voc, frame=f)
            out.append(db.select(KF.KFDB_RELOC, next_id[0], mc0, hits1, neigh_of[hits1["slot"]]))
        return out

    cand, nh = seq_batch()
    reps = max(3, min(a.reps, 10))
    bm, bb = timed(seq_batch, reps)
    sm, sb = timed(seq_single, reps)
    res["reloc_sequence_batch"] = {"frames": Q, "reps": reps, "ms_median": bm, "ms_min": bb, "ms_per_frame_median": bm / Q, "single_sequence_ms_median": sm, "single_sequence_ms_min": sb,
                                   "single_sequence_ms_per_frame_median": sm / Q, "nhits": int(nh), "ncandidates": int(sum(len(c) for c in cand)), "vocabulary_words": voc.size()}
    KF.orbhip.device_synchronize(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kfs", type=int, default=10000)
    ap.add_argument("--words", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--scoring", type=int, default=0, choices=[0, 1, 2, 4, 5])
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", nargs="?", const="1,8,64,512", default=None, help="batch sizes of the batched-query measurement")
    a = ap.parse_args()
    if a.batch:
        return batch_main(a)
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
