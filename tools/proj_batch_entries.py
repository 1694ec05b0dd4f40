#!/usr/bin/env python3
"""Secondary measurement: the batch forms of the projection-guided and the best-in-window search on their own, five slots of tools/matcher_latency.py's
KITTI-sized inputs (2000 features per frame, ~1500 queries): orbhip_search_by_projection_batch, orbhip_search_best_in_window_batch, and
orbhip_project_best_in_window_shared followed by one orbhip_project_best_in_window_held per slot (Fuse over five targets, a tenth of the points offered again).
Median of 15 per figure, ms; `answers` = a digest of what one call of each returned.  Prints one JSON line; ORBHIP_LIBRARY selects the library (an A/B run
alternates two builds as fresh processes: profiles/proj_slot_fold_latency.json)."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import orb_slam2_amd as A  # noqa: E402
from orb_slam2_amd import orbhip as H  # noqa: E402
from orb_slam2_amd import synth  # noqa: E402

NS = 5


def t(fn, reps=15):
    fn(); fn(); ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e3, 4)


def main():
    W, HT, N = 1241, 376, 2000
    FX, CX, CY = 718.856, 607.1928, 185.2157
    seq = synth.sequence(W, HT, 2, seed=5)
    ex = A.ORBextractor(N, 1.2, 8, 20, 7, W, HT, max_batch=2)
    ks, ds = ex.extract_batch(seq)
    sf = ex.GetScaleFactors(); inv = ex.GetInverseScaleSigmaSquares()
    (k1, d1), (k2, d2) = (ks[0], ds[0]), (ks[1], ds[1])
    rng = np.random.default_rng(1)
    keep = rng.random(len(k1)) < 0.75
    q = np.zeros(int(keep.sum()), A.PROJ_QUERY_DTYPE)
    q["x"], q["y"] = k1["x"][keep] - 3, k1["y"][keep] - 1
    q["radius"] = (7.0 * sf[k1["octave"][keep]]).astype(np.float32)
    q["min_level"], q["max_level"], q["blocks"], q["angle"] = k1["octave"][keep] - 1, k1["octave"][keep] + 1, 1, k1["angle"][keep]
    bq = np.zeros(len(q), A.BEST_QUERY_DTYPE)
    bq["x"], bq["y"], bq["radius"], bq["level"] = q["x"], q["y"], q["radius"], k1["octave"][keep]
    qd = d1[keep]
    bounds = (0.0, 0.0, float(W), float(HT))
    # the same queries as map points in front of a camera at the origin
    z = rng.uniform(4, 30, len(q))
    pts = np.zeros(len(q), H.MAP_POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = (q["x"] - CX) / FX * z, (q["y"] - CY) / FX * z, z
    p = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(np.float64); d = np.linalg.norm(p, axis=1)
    pts["nx"], pts["ny"], pts["nz"] = (p / d[:, None]).T
    pts["scale_dist"] = (d * sf[k1["octave"][keep]] * 0.97).astype(np.float32); pts["max_dist"] = 1e30; pts["level"] = -1
    lr = H.predict_scale_table(np.float32(np.log(np.float32(1.2))), 8)
    P = H.make_projection(H.PROJ_FUSE, np.eye(3), np.zeros(3), FX, FX, CX, CY, bounds, 3.0, sf, lr, bf=386.1448)
    again = pts[::10].copy(); again_d = np.ascontiguousarray(qd[::10])
    skip = np.zeros(len(pts), np.uint64)

    frames = [(k2, d2, q, qd)] * NS
    slots = [dict(kps=k2, desc=d2, bounds=bounds, inv_level_sigma2=inv, queries=bq, qdesc=qd)] * NS
    pslots = [dict(kps=k2, desc=d2, bounds=bounds, inv_level_sigma2=inv, proj=P)] * NS

    def fuse():
        out = H.project_best_in_window_shared(pslots, pts, qd, skip, True)
        return out, [H.project_best_in_window_held(s, P, again, again_d, True) for s in range(NS)]
    out = {
        "features": [len(k1), len(k2)], "queries": len(q), "slots": NS,
        "search_by_projection_batch_ms": t(lambda: A.search_by_projection_batch(frames, W, HT, 0, nnratio=0.8)),
        "search_by_projection x 5_ms": t(lambda: [A.search_by_projection(k2, d2, W, HT, q, qd, 0, nnratio=0.8) for _ in range(NS)]),
        "search_best_in_window_batch_ms": t(lambda: H.search_best_in_window_batch(slots, True)),
        "search_best_in_window x 5_ms": t(lambda: [A.search_best_in_window(k2, d2, W, HT, inv, bq, qd, True) for _ in range(NS)]),
        "project_best_in_window_shared_and_held_ms": t(fuse),
    }
    dig = lambda *a: hashlib.sha1(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()[:12]
    pb = A.search_by_projection_batch(frames, W, HT, 0, nnratio=0.8); wb = H.search_best_in_window_batch(slots, True); sh, held = fuse()
    out["answers"] = [int(pb[0][0]), dig(*[f for _, f in pb]), dig(*[x for pair in wb for x in pair]), dig(*[x for pair in sh + held for x in pair]), int((sh[0][1] <= 50).sum())]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
