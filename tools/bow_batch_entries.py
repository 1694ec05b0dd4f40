#!/usr/bin/env python3
"""Secondary measurement: the BoW matcher calls of tools/secondary_units.py's `abi` block on their own, without the reference around them: orbhip_search_by_bow x 5 vs
_batch(5) and orbhip_search_for_triangulation x 10 vs _batch(10) on KITTI-sized frames (2000 features), FeatureVectors = the 100-node partition of
tools/matcher_latency.py (ORBvoc's shape at levelsup 4).  Median of 7 per figure, ms; `answers` = nmatches and a digest of match12 of one call each.  Prints one
JSON line; ORBHIP_LIBRARY selects the library (an A/B run alternates two builds as fresh processes: profiles/bow_pair_fold_latency.json)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import orb_slam2_amd as A  # noqa: E402
from orb_slam2_amd import synth  # noqa: E402


def t(fn, reps=7):
    fn(); ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e3, 4)


def partition(desc):
    node = desc[:, 0].astype(np.int64) % 100
    order = np.argsort(node, kind="stable")
    ids, counts = np.unique(node, return_counts=True)
    return ids.astype(np.uint32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), order.astype(np.uint32)


def main():
    W, H, N = 1241, 376, 2000
    seq = synth.sequence(W, H, 2, seed=5)
    ex = A.ORBextractor(N, 1.2, 8, 20, 7, W, H, max_batch=2)
    ks, ds = ex.extract_batch(seq)
    (k0, d0), (k1, d1) = (ks[0], ds[0]), (ks[1], ds[1])
    rng = np.random.default_rng(11)
    fva, fvb = partition(d0), partition(d1)
    sf = (1.2 ** np.arange(8)).astype(np.float32)
    Fm = np.array([[0, -1e-3, 1.0 / 300], [1e-3, 0, -3.0 / 300], [-1.0 / 300, 3.0 / 300, 0]], np.float32)
    hmp1 = (rng.random(len(k0)) < 0.3).astype(np.uint8); hmp2 = (rng.random(len(k1)) < 0.3).astype(np.uint8)
    v1 = (rng.random(len(k0)) < 0.75).astype(np.uint8)
    z0, z1 = np.zeros(len(k0), np.uint8), np.zeros(len(k1), np.uint8)
    NB = 10
    kf1 = dict(desc=d0, kps=k0, has_mp=hmp1, stereo=z0, fv=fva, scale_factors=sf, level_sigma2=sf * sf)
    nbs = [dict(kf=dict(desc=d1, kps=k1, has_mp=hmp2, stereo=z1, fv=fvb, scale_factors=sf, level_sigma2=sf * sf), F12=Fm, ex=620.0, ey=190.0) for _ in range(NB)]
    tri_call = t(lambda: [A.search_for_triangulation(d0, k0, hmp1, z0, fva, d1, k1, hmp2, z1, fvb, Fm, 620.0, 190.0, sf, sf * sf, check_ori=False) for _ in range(NB)])
    tri_batch = t(lambda: A.search_for_triangulation_batch(kf1, nbs, check_ori=False))
    frame_side = dict(desc=d1, angle=k1["angle"], valid=None, fv=fvb)
    cands = [dict(desc=d0, angle=k0["angle"], valid=v1, fv=fva) for _ in range(5)]
    bow_call = t(lambda: [A.search_by_bow(0, d0, k0["angle"], v1, fva, d1, k1["angle"], None, fvb, nnratio=0.75) for _ in range(5)])
    bow_batch = t(lambda: A.search_by_bow_batch(0, [(c, frame_side) for c in cands], nnratio=0.75))
    n_s, m_s = A.search_by_bow(0, d0, k0["angle"], v1, fva, d1, k1["angle"], None, fvb, nnratio=0.75)
    n_t, m_t = A.search_for_triangulation(d0, k0, hmp1, z0, fva, d1, k1, hmp2, z1, fvb, Fm, 620.0, 190.0, sf, sf * sf, check_ori=False)
    import hashlib
    print(json.dumps({"orbhip_search_for_triangulation x 10 vs _batch(10)": {"per_call_ms": tri_call, "batch_ms": tri_batch},
                      "orbhip_search_by_bow x 5 vs _batch(5)": {"per_call_ms": bow_call, "batch_ms": bow_batch},
                      "answers": [n_s, hashlib.sha1(m_s.tobytes()).hexdigest()[:12], n_t, hashlib.sha1(m_t.tobytes()).hexdigest()[:12]]}))


if __name__ == "__main__":
    main()
