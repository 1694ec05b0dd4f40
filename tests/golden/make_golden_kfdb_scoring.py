"""Freezes what ORB_SLAM2's own KeyFrameDatabase does under the scoring objects other than L1 -> tests/golden/kfdb_scoring_ref.npz (data only).

The script of tests/golden/make_golden_kfdb.py (its ops and its word ids) is played once per scoring 1 (L2_NORM), 2 (CHI_SQUARE), 4 (BHATTACHARYYA) and
5 (DOT_PRODUCT) through the reference's own src/KeyFrameDatabase.cc, built in a temporary directory exactly as that generator builds it.  The vocabulary is
tests/golden/voc_k6_L3_ref.txt with the scoring field of its header replaced, written to the temporary directory.  The BowVectors' values are normalised as
that scoring's transform would leave them (ScoringObject.h:73-90): L2 for scoring 1, L1 for 2 and 4, not at all for 5 (values between 0.05 and 3: scores pass 1).
Frame "A" carries key frame 3's own vector and the LOOP query of key frame 10 meets key frame 10 itself: two self-products, which under L2 fall on either side
of the `s >= 1` clamp.  Under chi-square one word of that vector weighs 0 in both.

For every (query, key frame) pair that a query scores, the double that the reference's DBoW2 returns (oracle/dbow2_ref.py) is recorded too.

Refuses to write unless every scoring's script reaches the situations make_golden_kfdb.check_script names, and: L2 a scored pair with s >= 1 and a scored
SELF pair with s < 1; chi-square a scored pair with a shared word of weight 0 on both sides.

    python tests/golden/make_golden_kfdb_scoring.py
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import make_golden_kfdb as G                                               # noqa: E402

OUT = os.path.join(HERE, "kfdb_scoring_ref.npz")
SCORINGS = (1, 2, 4, 5)
SELF_OF = {"A": 3}                                                         # frame A carries key frame 3's vector


def normalise(scoring, v):
    if scoring == 1:
        return v / np.sqrt(np.sum(v * v))
    if scoring == 5:
        return v
    return v / v.sum()


def make_script(scoring, seed):
    """the ops and word ids of make_golden_kfdb.make_script; values drawn anew and normalised for `scoring`"""
    nkf, bows, ops = G.make_script()
    rng = np.random.default_rng(seed)
    out = []
    for ids, _ in bows:
        raw = rng.uniform(0.05, 3.0, len(ids)) if scoring == 5 else rng.random(len(ids)) + 0.05
        out.append([ids, raw])
    if scoring == 2:
        out[3][1][5] = 0.0                                                 # a word that weighs nothing (in key frame 3 and, below, in frame A)
    bows = [(ids, normalise(scoring, raw)) for ids, raw in out]
    a = nkf + 0                                                            # frames follow the key frames in make_script's order: A is the first
    assert np.array_equal(bows[a][0], bows[SELF_OF["A"]][0])
    bows[a] = (bows[a][0], bows[SELF_OF["A"]][1].copy())
    return nkf, bows, ops


def fill_min_score(nkf, bows, ops, score):
    """minScore of the LOOP query that must remove some hits: the median of what it scores with minScore 0 (as make_golden_kfdb.main)"""
    for op in ops:
        if op["op"] == "loop" and op["min_score"] is None:
            trial = [dict(o) for o in ops]
            for o in trial:
                if o["op"] == "loop" and o["min_score"] is None:
                    o["min_score"] = 0.0
            res = G.play_model(nkf, bows, trial, score)[ops.index(op)][2]
            sc = sorted(float(s) for s, _ in res.scored)
            assert len(sc) >= 3, "the LOOP query of the script scores fewer than three key frames"
            op["min_score"] = float(np.float32((sc[len(sc) // 2 - 1] + sc[len(sc) // 2]) / 2))


def index_of(bows, ids, vals):
    for i, (bi, bv) in enumerate(bows):
        if len(bi) == len(ids) and np.array_equal(bi, ids) and bv.tobytes() == np.asarray(vals).tobytes():
            return i
    raise AssertionError("a scored BowVector that the script does not hold")


def scored_pairs(nkf, bows, ops, score):
    """the model's run with every call of the score function recorded -> (model results, [(query bow, key frame)] in call order)"""
    pairs = []

    def recording(a, b, c, d):
        pairs.append((index_of(bows, a, b), index_of(bows[:nkf], c, d)))   # (frame A and key frame 3 hold the same vector: the first is named)
        return score(a, b, c, d)
    model = G.play_model(nkf, bows, ops, recording)
    return model, pairs


def extra_situations(scoring, bows, pairs, O):
    if scoring == 1:
        s = {(q, k): O.voc_score(5, *bows[q], *bows[k]) for q, k in pairs}  # the chain of products itself
        is_self = lambda q, k: bows[q][0].tobytes() == bows[k][0].tobytes() and bows[q][1].tobytes() == bows[k][1].tobytes()
        return any(v >= 1 for v in s.values()) and any(v < 1 and is_self(q, k) for (q, k), v in s.items())
    if scoring == 2:
        for q, k in pairs:
            common, iq, ik = np.intersect1d(bows[q][0], bows[k][0], return_indices=True)
            if np.any((bows[q][1][iq] == 0) & (bows[k][1][ik] == 0)):
                return True
        return False
    return True


def main():
    if not os.path.isdir(os.path.join(G.REF, "src")):
        sys.exit(f"{G.REF} is not mounted: the golden is made where the reference is")
    from oracle import orb_oracle as O
    from oracle import dbow2_ref as D
    O.build()
    assert D.build(), "the reference's DBoW2 could not be built"
    save = {"scorings": np.array(SCORINGS, np.int32), "nwords": np.int32(G.NWORDS)}
    text = open(G.VOC).read().split("\n", 1)
    assert text[0].split() == ["6", "3", "0", "0"], text[0]
    with tempfile.TemporaryDirectory() as tmp:
        lib = G.build_reference(tmp)
        for scoring in SCORINGS:
            score = lambda a, b, c, d, s=scoring: O.voc_score(s, a, b, c, d)
            for seed in range(1000 * scoring, 1000 * scoring + 200):         # the first seed whose draws reach every situation
                nkf, bows, ops = make_script(scoring, seed)
                fill_min_score(nkf, bows, ops, score)
                model, pairs = scored_pairs(nkf, bows, ops, score)
                try:
                    G.check_script(ops, bows, model)
                except AssertionError:
                    continue
                if extra_situations(scoring, bows, pairs, O):
                    break
            else:
                raise AssertionError(f"scoring {scoring}: no seed reaches every situation")
            voc = os.path.join(tmp, f"voc_scoring{scoring}.txt")
            with open(voc, "w") as f:
                f.write(f"6 3  {scoring} 0\n" + text[1])
            G.VOC = voc                                                     # play_reference loads the vocabulary it names
            ref = G.play_reference(lib, nkf, bows, ops)
            rv = D.RefVocabulary()
            assert rv.load_text(voc)
            dbow2 = np.array([rv.score(*bows[q], *bows[k]) for q, k in pairs], np.float64)
            rv.close()
            nops = len(ops)
            q = np.zeros((nops, nkf, 2), np.uint64); w = np.zeros((nops, nkf, 2), np.int32); s = np.zeros((nops, nkf, 2), np.uint32)
            cand, cand_off = [], [0]
            for i, (c, fields, _) in enumerate(ref):
                for k in range(nkf):
                    for kind in (0, 1):
                        q[i, k, kind], w[i, k, kind] = fields[k][kind][0], fields[k][kind][1]
                        s[i, k, kind] = np.float32(fields[k][kind][2]).view(np.uint32)
                cand += c or []
                cand_off.append(len(cand))
            p = f"s{scoring}_"
            ids = {"nkf": np.int32(nkf), "bow_off": np.cumsum([0] + [len(b[0]) for b in bows]).astype(np.int32), "bow_id": np.concatenate([b[0] for b in bows]).astype(np.uint32)}
            assert all(np.array_equal(save.get(k, v), v) for k, v in ids.items())       # the word ids are the script's: the same under every scoring, kept once
            save.update(ids)
            save.update({p + "ops": np.frombuffer(json.dumps(ops).encode(), np.uint8), p + "seed": np.int32(seed),
                         p + "bow_val": np.concatenate([b[1] for b in bows]).astype(np.float64),
                         p + "is_query": np.array([c is not None for c, _, _ in ref], np.uint8), p + "cand_off": np.array(cand_off, np.int32), p + "cand": np.array(cand, np.int32),
                         p + "field_query": q, p + "field_words": w, p + "field_score_bits": s,
                         p + "pair": np.array(pairs, np.int32).reshape(-1, 2), p + "pair_dbow2": dbow2})
            agree = all(rc == mc for (rc, _, _), (mc, _, _) in zip(ref, model))
            print(f"scoring {scoring}: seed {seed}, {nops} calls, {int(sum(c is not None for c, _, _ in ref))} queries, {len(cand)} candidates, {len(pairs)} scored pairs; "
                  f"the model's candidates agree: {agree}")
    np.savez_compressed(OUT, **save)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
