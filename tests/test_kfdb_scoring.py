"""The device key-frame database under the vocabulary's own scoring object (orbhip_kfdb_set_scoring; KeyFrameDatabase.set_scoring): L2_NORM (1), CHI_SQUARE (2),
BHATTACHARYYA (4) and DOT_PRODUCT (5) beside the L1_NORM (0) of tests/test_kfdb.py.

The chain is the one of that file: tests/golden/kfdb_scoring_ref.npz holds what the reference's own KeyFrameDatabase returned for the recorded script under each
scoring (tests/golden/make_golden_kfdb_scoring.py); tests/kfdb_model.py, given oracle.voc_score(scoring, ...), must reproduce it; the product must reproduce the
golden, and the model and the oracle at the shapes at which k_kfdb_scan can go wrong.  Every comparison is exact: slots, counts, the raw bits of every float
and double.  The last test is the check that the device's double sqrt and division equal the host's in every bit."""
import threading

import numpy as np
import pytest

import orb_slam2_amd
from orb_slam2_amd import KFDB_LOOP, KFDB_RELOC
import kfdb_model as M
import kfdb_scoring_golden as SG
from kfdb_scoring_golden import SCORINGS, sbow
from test_kfdb import Pair, bits, covis

ERR_INVALID, ERR_UNSUPPORTED = orb_slam2_amd.orbhip.ERR_INVALID, orb_slam2_amd.orbhip.ERR_UNSUPPORTED


def scorer(oracle, scoring):
    return lambda a, b, c, d: oracle.voc_score(scoring, a, b, c, d)


def pair(backend, nwords, oracle, scoring, check_state=True):
    P = Pair(backend, nwords, scorer(oracle, scoring), check_state)
    P.db.set_scoring(scoring)
    assert P.db.scoring == scoring
    return P


def dbits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ 1: the golden
@pytest.mark.parametrize("scoring", SCORINGS)
def test_model_reproduces_reference(oracle, scoring):
    nkf, bows, ops, res, pairs, dbow2 = SG.load(scoring)
    kfs = [M.KF(k, *bows[k]) for k in range(nkf)]
    db = M.ModelDatabase(scorer(oracle, scoring))
    nq = 0
    for i, (op, (cand, fields)) in enumerate(zip(ops, res)):
        r = None
        if op["op"] == "add":
            db.add(kfs[op["kf"]])
        elif op["op"] == "erase":
            db.erase(kfs[op["kf"]])
        elif op["op"] == "clear":
            db.clear()
        elif op["op"] == "connect":
            kfs[op["kf"]].connected.append(kfs[op["other"]])
            if op["w"] > 0:
                kfs[op["kf"]].ordered.append(kfs[op["other"]])
        elif op["op"] == "loop":
            r = db.detect_loop(kfs[op["kf"]], op["min_score"])
        else:
            r = db.detect_reloc(M.KF(op["qid"], *bows[op["bow"]]))
        assert (cand is None) == (r is None), i
        if r is not None:
            nq += 1
            assert [k.mnId for k in r.candidates] == cand, (i, op)
        for k in range(nkf):
            for kind in (0, 1):
                q, w, s = kfs[k].fields(kind)
                assert (q, w, bits(s)) == fields[k][kind], (i, op, k, kind)
    assert nq >= 10 and any(c for c, _ in res)


@pytest.mark.parametrize("scoring", SCORINGS)
def test_recorded_dbow2_scores_equal_the_oracle(oracle, scoring):
    """the doubles the reference's DBoW2 returned for every pair the script scores, and the situations the generator insisted on"""
    nkf, bows, ops, res, pairs, dbow2 = SG.load(scoring)
    assert len(pairs) == len(dbow2) >= 20
    want = np.array([oracle.voc_score(scoring, *bows[q], *bows[k]) for q, k in pairs])
    assert np.array_equal(dbits(want), dbits(dbow2))
    if scoring == 1:
        s = np.array([oracle.voc_score(5, *bows[q], *bows[k]) for q, k in pairs])      # the chain of products before the epilogue
        assert np.any(s >= 1) and np.any(dbow2 == 1.0)
        assert any(v < 1 and q == k for v, (q, k) in zip(s, pairs))                   # a self-product below 1 (frame A is named as key frame 3, whose vector it holds)
    if scoring == 2:
        zero = [np.any((bows[q][1][np.isin(bows[q][0], bows[k][0])] == 0) & (bows[k][1][np.isin(bows[k][0], bows[q][0])] == 0)) for q, k in pairs]
        assert any(zero)
    if scoring == 5:
        assert np.any(dbow2 > 1)


@pytest.mark.parametrize("scoring", SCORINGS)
def test_product_reproduces_reference(backend, oracle, scoring):
    nkf, bows, ops, res, _, _ = SG.load(scoring)
    kfs = [M.KF(k, *bows[k]) for k in range(nkf)]
    P = pair(backend, 216, oracle, scoring)
    for i, (op, (cand, fields)) in enumerate(zip(ops, res)):
        if op["op"] == "add":
            P.add(kfs[op["kf"]])
        elif op["op"] == "erase":
            P.erase(kfs[op["kf"]])
        elif op["op"] == "clear":
            P.clear()
        elif op["op"] == "connect":
            kfs[op["kf"]].connected.append(kfs[op["other"]])
            if op["w"] > 0:
                kfs[op["kf"]].ordered.append(kfs[op["other"]])
        elif op["op"] == "loop":
            r = P.query(KFDB_LOOP, kfs[op["kf"]], op["min_score"])                  # (hits, counts and every live key frame's state against the model's)
            assert [k.mnId for k in r.candidates] == cand, (i, op)
        else:
            r = P.query(KFDB_RELOC, M.KF(op["qid"], *bows[op["bow"]]))
            assert [k.mnId for k in r.candidates] == cand, (i, op)
        for kf in P.live:                                                          # the product's state against the GOLDEN's fields
            for kind in (0, 1):
                q, w, s = P.db.state(kind, P.slot[id(kf)])
                assert (q, w, bits(s)) == fields[kf.mnId][kind], (i, op, kf.mnId, kind)
    assert P.db.scoring == scoring


# ------------------------------------------------------------------------------------------------ 2: scores at the scan's shapes
def shared_bows(rng, scoring, nwords, nq, kf_words, shared):
    """tests/test_kfdb.py::shared_bows with this scoring's normalisation: exactly `shared` common words, ids 0 and nwords - 1 among them when there are two"""
    ids = rng.choice(nwords - 2, nq + kf_words - shared, replace=False) + 1
    common, q_only, k_only = ids[:shared], ids[shared:nq], ids[nq:]
    if shared >= 2:
        common[0], common[1] = 0, nwords - 1
    return sbow(rng, scoring, np.concatenate([common, q_only])), sbow(rng, scoring, np.concatenate([common, k_only]))


@pytest.mark.parametrize("scoring", SCORINGS)
def test_scores_double_for_double(backend, oracle, scoring):
    """64 words of a key frame per round of the scan, the ONE chain across rounds, the LDS-staged query: db.scores must equal oracle.voc_score double for
    double, db.query its float"""
    rng = np.random.default_rng(50 + scoring)
    nwords = 10**6
    db = orb_slam2_amd.KeyFrameDatabase(nwords, library=backend)
    db.set_scoring(scoring)
    for nq, cases in [(300, [(1, 0), (1, 1), (63, 1), (64, 64), (65, 65), (200, 130), (8192, 300)]), (1, [(1, 1), (200, 1)]), (257, [(8192, 257)]), (8192, [(8192, 8192)])]:
        for kw, sh in cases:
            (qi, qv), (ki, kv) = shared_bows(rng, scoring, nwords, nq, kw, sh)
            assert len(qi) == nq and len(ki) == kw and len(np.intersect1d(qi, ki)) == sh
            s0, s1 = db.add(ki, kv), db.add(qi, qv)
            got = db.scores(qi, qv, [s0, s1, s0])
            want = np.array([oracle.voc_score(scoring, qi, qv, ki, kv), oracle.voc_score(scoring, qi, qv, qi, qv), oracle.voc_score(scoring, qi, qv, ki, kv)])
            assert np.array_equal(dbits(got), dbits(want)), (nq, kw, sh, got, want)
            s2 = db.add(ki, kv)
            hits, nsharing, minc = db.query(KFDB_RELOC, 1, qi, qv)
            assert nsharing == 1 + 2 * (sh > 0) and minc == int(np.float32(nq) * np.float32(0.8))
            by_slot = {int(h["slot"]): h for h in hits}
            assert int(by_slot[s1]["words"]) == nq and bits(by_slot[s1]["score"]) == bits(np.float32(want[1]))
            assert (s0 in by_slot) == (s2 in by_slot) == (sh > minc)
            if sh > minc:
                assert int(by_slot[s0]["words"]) == sh and bits(by_slot[s2]["score"]) == bits(np.float32(want[0])) and [int(h["slot"]) for h in hits] == [s0, s1, s2]
            db.clear()


# ------------------------------------------------------------------------------------------------ 3: switching
def test_switching_leaves_earlier_scores_in_place(backend, oracle):
    """One database queried under L1, then set_scoring(1), then queried under a new id: the second query's hits carry L2 scores; a key frame it does not score
    keeps the bits of its L1 mRelocScore.  The model's score function is switched at the same point."""
    rng = np.random.default_rng(31)
    nwords = 5000
    base = rng.choice(nwords, 80, replace=False)
    kfs = [M.KF(k + 1, *sbow(rng, 0, rng.choice(base, 60, replace=False))) for k in range(10)]
    kfs.append(M.KF(11, *sbow(rng, 0, np.concatenate([base[:70], 4000 + np.arange(30)]))))
    covis(rng, kfs)
    P = Pair(backend, nwords, scorer(oracle, 0))
    assert P.db.scoring == 0
    for k in kfs:
        P.add(k)
    r1 = P.query(KFDB_RELOC, M.KF(100, *sbow(rng, 0, base)))
    assert len(r1.scored) == len(kfs)
    l1_bits = {k.mnId: bits(k.mRelocScore) for k in kfs}
    P.db.set_scoring(1)
    P.model.score = scorer(oracle, 1)
    q2 = M.KF(101, *sbow(rng, 1, np.concatenate([4000 + np.arange(30), base[:2]])))  # key frame 11's own 30 words and two of everybody's
    r2 = P.query(KFDB_RELOC, q2)                                                     # (hits and every key frame's state are compared inside)
    assert [k.mnId for _, k in r2.scored] == [11] and len(r2.sharing) > 1
    assert bits(r2.scored[0][0]) == bits(np.float32(oracle.voc_score(1, q2.bow_id, q2.bow_val, kfs[10].bow_id, kfs[10].bow_val))) != l1_bits[11]
    for k in kfs[:10]:
        q, w, s = P.db.state(KFDB_RELOC, P.slot[id(k)])
        if q == 101:                                                                 # met by the second query, below minCommonWords: not scored
            assert bits(s) == l1_bits[k.mnId] and bits(s) != 0
    assert any(P.db.state(KFDB_RELOC, P.slot[id(k)])[0] == 101 for k in kfs[:10])
    P.db.scoring = 0                                                                 # and back, through the property
    P.model.score = scorer(oracle, 0)
    P.query(KFDB_RELOC, M.KF(102, *sbow(rng, 0, base)))


# ------------------------------------------------------------------------------------------------ 4: a resident frame
@pytest.mark.parametrize("scoring", [1, 4])
def test_query_frame_under_the_vocabulary_scoring(backend, scoring):
    from orb_slam2_amd import synth
    w, h, n = 320, 240, 300
    ex = orb_slam2_amd.ORBextractor(n, 1.2, 8, 20, 7, w, h, max_batch=2, library=backend)
    voc = orb_slam2_amd.ORBVocabulary(SG.VOC, library=backend)
    assert voc.getScoringType() == 0
    voc.setScoringType(scoring)
    assert voc.getScoringType() == scoring == voc.scoring
    ex.extract_batch([synth.frame(w, h, seed=21), synth.frame(w, h, seed=22)])
    voc.compute_bow(ex, 2, levelsup=4)
    bows = [voc.fetch_bow(ex, f)[:2] for f in range(2)]
    assert len(bows[0][0]) > 10 and len(bows[1][0]) > 10
    norm = [np.sum(b[1] * b[1]) if scoring == 1 else np.sum(b[1]) for b in bows]     # transform normalises as the scoring demands
    assert all(abs(x - 1) < 1e-12 for x in norm) and (scoring != 1 or all(np.sum(b[1]) > 1.5 for b in bows))
    rng = np.random.default_rng(3)
    a, b = orb_slam2_amd.KeyFrameDatabase(voc.size(), library=backend), orb_slam2_amd.KeyFrameDatabase(voc.size(), library=backend)
    a.set_scoring(scoring); b.set_scoring(scoring)
    kf = []
    for k in range(40):
        kf.append(sbow(rng, scoring, rng.choice(voc.size(), int(rng.integers(5, 120)), replace=False)))
        assert a.add(*kf[-1]) == b.add(*kf[-1])
    for f in range(2):
        for kind in (KFDB_RELOC, KFDB_LOOP):
            ha, na, ma = a.query_frame(kind, 5 + f, ex, voc, frame=f, excluded=[1, 2], min_score=0.01)
            hb, nb, mb = b.query(kind, 5 + f, bows[f][0], bows[f][1], excluded=[1, 2], min_score=0.01)
            assert na == nb > 0 and ma == mb and ha.tobytes() == hb.tobytes() and len(ha) > 0
            for hit in ha:                                                          # ... and they are this scoring's scores
                assert bits(hit["score"]) == bits(np.float32(voc.score(bows[f][0], bows[f][1], *kf[int(hit["slot"])])))
    for s in range(40):
        for kind in (KFDB_RELOC, KFDB_LOOP):
            assert a.state(kind, s) == b.state(kind, s)


# ------------------------------------------------------------------------------------------------ 5: errors
def test_refused_scorings_leave_the_database_as_it_was(backend, oracle):
    rng = np.random.default_rng(6)
    P = pair(backend, 20000, oracle, 4)
    kfs = [M.KF(k + 1, *sbow(rng, 4, rng.choice(400, 100, replace=False))) for k in range(12)]
    covis(rng, kfs)
    for k in kfs:
        P.add(k)
    frame = M.KF(21, *sbow(rng, 4, rng.choice(400, 150, replace=False)))
    assert len(P.query(KFDB_RELOC, frame).scored) >= 1
    with pytest.raises(orb_slam2_amd.OrbHipError) as e:
        P.db.set_scoring(3)
    assert e.value.status == ERR_UNSUPPORTED and "KL" in str(e.value)
    for bad in (6, -1):
        with pytest.raises(orb_slam2_amd.OrbHipError) as e:
            P.db.set_scoring(bad)
        assert e.value.status == ERR_INVALID
    L = orb_slam2_amd.lib(backend)
    assert L.orbhip_kfdb_set_scoring(None, 1) == ERR_INVALID and L.orbhip_voc_set_scoring(None, 1) == ERR_INVALID
    assert P.db.scoring == 4
    frame.mnId = 22
    assert len(P.query(KFDB_RELOC, frame).scored) >= 1                               # still Bhattacharyya, exact
    voc = orb_slam2_amd.ORBVocabulary(SG.VOC, library=backend)
    for bad in (6, -1):
        with pytest.raises(orb_slam2_amd.OrbHipError) as e:
            voc.setScoringType(bad)
        assert e.value.status == ERR_INVALID
    voc.setScoringType(3)                                                            # the vocabulary itself scores KL (host arithmetic)
    assert voc.getScoringType() == 3
    assert voc.score(frame.bow_id, frame.bow_val, kfs[0].bow_id, kfs[0].bow_val) == oracle.voc_score(3, frame.bow_id, frame.bow_val, kfs[0].bow_id, kfs[0].bow_val)


def test_vocabulary_set_scoring_reaches_score_and_the_saved_header(backend, oracle, tmp_path):
    rng = np.random.default_rng(8)
    voc = orb_slam2_amd.ORBVocabulary(SG.VOC, library=backend)
    a, b = sbow(rng, 0, rng.choice(216, 60, replace=False)), sbow(rng, 0, rng.choice(216, 60, replace=False))
    for s in range(6):
        voc.setScoringType(s)
        assert dbits(voc.score(*a, *b)) == dbits(oracle.voc_score(s, *a, *b))
        out = tmp_path / f"v{s}.txt"
        voc.saveToTextFile(out)
        lines = open(out).read().split("\n")
        assert lines[0] == f"6 3  {s} 0" and lines[1:] == open(SG.VOC).read().split("\n")[1:]


# ------------------------------------------------------------------------------------------------ 6: three threads
def test_two_threads_query_while_a_third_adds(backend, oracle):
    """tests/test_kfdb.py's thread test under chi-square: the key frames added during a phase share no word with that phase's queries"""
    scoring = 2
    rng = np.random.default_rng(7)
    nwords, nphase, per_phase = 10**6, 2, 40
    P = pair(backend, nwords, oracle, scoring, check_state=False)
    band = lambda p: 1000 * p + rng.choice(200, 60, replace=False)
    for k in range(30):
        P.add(M.KF(k + 1, *sbow(rng, scoring, band(0))))
    next_id = 100
    for p in range(nphase):
        new = [M.KF(next_id + i, *sbow(rng, scoring, band(p + 1))) for i in range(per_phase)]
        next_id += per_phase
        frames = [M.KF(1000 + 10 * p + i, *sbow(rng, scoring, np.concatenate([band(q) for q in range(p + 1)]))) for i in range(4)]
        loops = [M.KF(2000 + 10 * p + i, *sbow(rng, scoring, np.concatenate([band(q) for q in range(p + 1)]))) for i in range(4)]
        for q in loops:
            q.connected = [P.live[int(j)] for j in rng.integers(0, len(P.live), 4)]
        want = {}
        for q in frames:
            r = P.model.detect_reloc(q)
            want[q.mnId] = (len(r.sharing), r.min_common, [(P.slot[id(k)], bits(s), k.fields(0)[1]) for s, k in r.scored])
        for q in loops:
            r = P.model.detect_loop(q, 0.05)
            want[q.mnId] = (len(r.sharing), r.min_common, [(P.slot[id(k)], bits(s), k.fields(1)[1]) for s, k in r.scored])
        got, errors = {}, []

        def run_queries(kind, qs):
            try:
                for q in qs:
                    ex = [P.slot[id(k)] for k in q.connected] if kind == KFDB_LOOP else None
                    hits, ns, mc = P.db.query(kind, q.mnId, q.bow_id, q.bow_val, excluded=ex, min_score=0.05 if kind == KFDB_LOOP else 0.0, cap=4096)
                    got[q.mnId] = (ns, mc, [(int(h["slot"]), bits(h["score"]), int(h["words"])) for h in hits])
            except Exception as e:                                         # noqa: BLE001
                errors.append(e)

        def run_adds():
            try:
                for k in new:
                    s = P.db.add(k.bow_id, k.bow_val)
                    P.slot[id(k)], P.kf_of[s] = s, k
            except Exception as e:                                         # noqa: BLE001
                errors.append(e)

        ts = [threading.Thread(target=run_queries, args=(KFDB_RELOC, frames)), threading.Thread(target=run_queries, args=(KFDB_LOOP, loops)), threading.Thread(target=run_adds)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert got == want, p
        assert any(len(v[2]) for v in got.values())
        for k in new:
            P.model.add(k)
            P.live.append(k)
        P.states()
    assert len(P.db) == 30 + nphase * per_phase and P.db.scoring == scoring


# ------------------------------------------------------------------------------------------------ 7: the device's double sqrt and division
def probe_weights():
    """4096 doubles: a spread of exponents down to subnormals, runs of ADJACENT doubles around 0.25, 0.5, 1, 2 and 4 (where the rounding decision of a square
    root flips from one neighbour to the next, and where L2's 1 - s and its clamp at s >= 1 change), the smallest subnormals, squares and their neighbours
    (roots that are exact or just off a double), uniform draws."""
    rng = np.random.default_rng(4096)
    w = [np.ldexp(rng.uniform(1.0, 2.0, 1024), rng.integers(-1074, 64, 1024))]
    for c in (0.25, 0.5, 1.0, 2.0, 4.0):
        w.append((np.array(c).view(np.int64) + np.arange(-128, 128)).view(np.float64))
    w.append(np.arange(1, 257) * 5e-324)
    m = rng.uniform(0.5, 1.0, 170)
    sq = m * m
    w.append(np.concatenate([sq, np.nextafter(sq, 0.0), np.nextafter(sq, 2.0)]))
    w = np.concatenate(w)
    w = np.concatenate([w, rng.random(4096 - len(w))])
    assert len(w) == 4096 and np.all(w > 0) and np.all(np.isfinite(w)) and np.sum(w < 2.3e-308) > 200
    return w


@pytest.mark.parametrize("scoring,v", [(4, 1.0), (1, 1.0), (2, 0.3)])
def test_device_sqrt_and_division_equal_the_host(backend, oracle, scoring, v):
    """One-word key frames (word 7, weight w_k) against a one-word query (weight v): Bhattacharyya is sqrt(v w_k), chi-square 2 (v w_k / (v + w_k)), L2
    1 - sqrt(1 - v w_k) or the clamp.  With v = 1 the product IS w_k.  One scores call over all slots, compared bit for bit with the oracle: no tolerance."""
    w = probe_weights()
    db = orb_slam2_amd.KeyFrameDatabase(100, library=backend)
    db.set_scoring(scoring)
    ids = np.array([7], np.uint32)
    slots = [db.add(ids, np.array([x])) for x in w]
    got = db.scores(ids, np.array([v]), slots)
    want = np.array([oracle.voc_score(scoring, ids, np.array([v]), ids, np.array([x])) for x in w])
    if scoring == 4:
        assert np.array_equal(dbits(want), dbits(np.sqrt(v * w)))
    if scoring == 1:
        assert np.sum(want == 1.0) > 100 and np.sum(want < 1.0) > 100
    bad = np.nonzero(dbits(got) != dbits(want))[0]
    assert len(bad) == 0, (len(bad), [(float(w[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:8]])
