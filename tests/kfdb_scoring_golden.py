"""Reader of tests/golden/kfdb_scoring_ref.npz (tests/golden/make_golden_kfdb_scoring.py): what the reference's KeyFrameDatabase returned and left in the key
frames for the script of kfdb_ref.npz under the scoring objects 1 (L2_NORM), 2 (CHI_SQUARE), 4 (BHATTACHARYYA) and 5 (DOT_PRODUCT)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kfdb_scoring_ref.npz")
VOC = os.path.join(ROOT, "tests", "golden", "voc_k6_L3_ref.txt")
SCORINGS = (1, 2, 4, 5)
NAMES = {0: "L1_NORM", 1: "L2_NORM", 2: "CHI_SQUARE", 3: "KL", 4: "BHATTACHARYYA", 5: "DOT_PRODUCT"}


def load(scoring, path=GOLDEN):
    """-> (nkf, bows [(ids, vals)], ops [dict], per op: (candidates as key-frame indices or None, fields[key frame][kind] = (query, words, float32 score bits)),
    pairs [(query bow, key frame)] that the script's queries score, the reference's DBoW2 score of each)"""
    g = np.load(path)
    assert scoring in [int(s) for s in g["scorings"]]
    p = f"s{scoring}_"
    off = g["bow_off"]
    bows = [(g["bow_id"][off[i]:off[i + 1]].copy(), g[p + "bow_val"][off[i]:off[i + 1]].copy()) for i in range(len(off) - 1)]
    ops = json.loads(bytes(g[p + "ops"]).decode())
    nkf = int(g["nkf"])
    res = []
    for i in range(len(ops)):
        cand = [int(c) for c in g[p + "cand"][g[p + "cand_off"][i]:g[p + "cand_off"][i + 1]]] if g[p + "is_query"][i] else None
        fields = [[(int(g[p + "field_query"][i, k, kind]), int(g[p + "field_words"][i, k, kind]), int(g[p + "field_score_bits"][i, k, kind])) for kind in (0, 1)] for k in range(nkf)]
        res.append((cand, fields))
    return nkf, bows, ops, res, [(int(q), int(k)) for q, k in g[p + "pair"]], g[p + "pair_dbow2"].copy()


def write_vocabulary(scoring, path):
    """tests/golden/voc_k6_L3_ref.txt with the scoring field of its header replaced"""
    head, rest = open(VOC).read().split("\n", 1)
    assert head.split() == ["6", "3", "0", "0"]
    with open(path, "w") as f:
        f.write(f"6 3  {scoring} 0\n" + rest)
    return str(path)


def sbow(rng, scoring, ids):
    """a random BowVector over `ids`, normalised as `scoring`'s transform leaves it (ScoringObject.h:73-90): L2 for 1, none for 5 (values 0.05 .. 3), L1 otherwise"""
    ids = np.unique(np.asarray(ids, np.int64)).astype(np.uint32)
    if scoring == 5:
        return ids, rng.uniform(0.05, 3.0, len(ids))
    v = rng.random(len(ids)) + 1e-3
    return ids, v / np.sqrt(np.sum(v * v)) if scoring == 1 else v / v.sum()
