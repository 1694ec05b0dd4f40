"""The device key-frame database (orbhip_kfdb_*, orb_slam2_amd.KeyFrameDatabase) against ORB_SLAM2's KeyFrameDatabase.

The chain is reference -> model -> product: tests/golden/kfdb_ref.npz holds what the reference's own member functions returned and left in the key frames for
a recorded script of calls (tests/golden/make_golden_kfdb.py); tests/kfdb_model.py is a literal restatement of KeyFrameDatabase.cc that must reproduce it; the
product must reproduce the golden, and the model on synthetic databases of the sizes at which the two kernels can go wrong.  Everything is compared exactly:
slots, counts, the raw bits of every float.

Sizes the sweep is built around: k_kfdb_scan stages the WHOLE query id list in LDS (at most 8192 ids, copied 256 per round: query sizes 1, 255, 256, 257 and
8192), searches 64 words of a key frame per round (1, 63, 64, 65, 200 and 8192 words; 0, 1, 64, 65 and more than 128 shared ones) and handles four key frames
per workgroup; k_kfdb_select passes over 1024 slots per round and sorts up to 4096 listed key frames in LDS, more in device memory (4097 key frames)."""
import os
import threading

import numpy as np
import pytest

import orb_slam2_amd
from orb_slam2_amd import KFDB_LOOP, KFDB_RELOC
import kfdb_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kfdb_ref.npz")
VOC = os.path.join(ROOT, "tests", "golden", "voc_k6_L3_ref.txt")


def bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.fixture(scope="module")
def l1(oracle):
    return lambda a, b, c, d: oracle.voc_score(0, a, b, c, d)


class Pair:
    """One script through the model and the product side by side; every answer compared as it comes."""

    def __init__(self, backend, nwords, score, check_state=True):
        self.db = orb_slam2_amd.KeyFrameDatabase(nwords, library=backend)
        self.model = M.ModelDatabase(score)
        self.slot, self.kf_of, self.live = {}, {}, []
        self.check_state = check_state

    def add(self, kf):
        self.model.add(kf)
        s = self.db.add(kf.bow_id, kf.bow_val)
        assert s not in self.kf_of
        self.slot[id(kf)], self.kf_of[s] = s, kf
        self.live.append(kf)
        return s

    def erase(self, kf):
        self.model.erase(kf)
        s = self.slot.pop(id(kf))
        self.db.erase(s)
        del self.kf_of[s]
        self.live = [k for k in self.live if k is not kf]

    def clear(self):
        self.model.clear()
        self.db.clear()
        self.slot, self.kf_of, self.live = {}, {}, []

    def states(self):
        assert len(self.db) == len(self.live)
        for kf in self.live:
            for kind in (KFDB_RELOC, KFDB_LOOP):
                q, w, s = self.db.state(kind, self.slot[id(kf)])
                mq, mw, ms = kf.fields(kind)
                assert (q, w, bits(s)) == (mq, mw, bits(ms)), (kf.mnId, kind)

    def query(self, kind, q, min_score=0.0):
        """q: a model KF (the frame, or the querying key frame with its connected list) -> the model's Result, after every comparison"""
        r = self.model.detect_reloc(q) if kind == KFDB_RELOC else self.model.detect_loop(q, min_score)
        excluded = [self.slot[id(k)] for k in q.connected if id(k) in self.slot] if kind == KFDB_LOOP else None
        hits, nsharing, minc = self.db.query(kind, q.mnId, q.bow_id, q.bow_val, excluded=excluded, min_score=min_score)
        assert nsharing == len(r.sharing) and minc == r.min_common
        assert [(int(h["slot"]), bits(h["score"])) for h in hits] == [(self.slot[id(k)], bits(s)) for s, k in r.scored]
        assert [int(h["words"]) for h in hits] == [k.fields(kind)[1] for _, k in r.scored]
        neigh = [[self.slot.get(id(k2), -1) for k2 in self.kf_of[int(h["slot"])].best_covisibles(10)] for h in hits]
        cand = self.db.select(kind, q.mnId, minc, hits, neigh, min_score=min_score)
        assert [int(c) for c in cand] == [self.slot[id(k)] for k in r.candidates]
        if self.check_state:
            self.states()
        return r


# ------------------------------------------------------------------------------------------------ 1, 2: the golden
def test_model_reproduces_reference(l1):
    nkf, bows, ops, res = M.load_golden(GOLDEN)
    kfs = [M.KF(k, *bows[k]) for k in range(nkf)]
    db = M.ModelDatabase(l1)
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


def test_product_reproduces_reference(backend, l1):
    nkf, bows, ops, res = M.load_golden(GOLDEN)
    kfs = [M.KF(k, *bows[k]) for k in range(nkf)]
    P = Pair(backend, 216, l1)
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
            r = P.query(KFDB_LOOP, kfs[op["kf"]], op["min_score"])
            assert [k.mnId for k in r.candidates] == cand, (i, op)
        else:
            r = P.query(KFDB_RELOC, M.KF(op["qid"], *bows[op["bow"]]))
            assert [k.mnId for k in r.candidates] == cand, (i, op)
        for kf in P.live:                                                  # the product's state against the GOLDEN's fields (Pair.query compared it with the model's)
            for kind in (0, 1):
                q, w, s = P.db.state(kind, P.slot[id(kf)])
                assert (q, w, bits(s)) == fields[kf.mnId][kind], (i, op, kf.mnId, kind)


# ------------------------------------------------------------------------------------------------ 3: the shape sweep
def rbow(rng, ids):
    ids = np.unique(np.asarray(ids, np.int64)).astype(np.uint32)
    v = rng.random(len(ids)) + 1e-3
    return ids, v / v.sum()                                                # L1 = 1: the order of the chain's additions shows in the last bits


def covis(rng, kfs, n=3):
    for k in kfs:
        k.ordered = [kfs[int(j)] for j in rng.integers(0, len(kfs), min(n, len(kfs)))]
        k.connected = list(k.ordered)


@pytest.mark.parametrize("nkf,nwords", [(1, 10**6), (63, 10**6), (65, 216), (257, 10**6), (1025, 10**6)])
def test_sweep_key_frame_counts(backend, l1, nkf, nwords):
    """Key-frame counts around a workgroup of the scan (4), a pass of the select (1024), with varied words per key frame; RELOC and LOOP, repeated id, erase
    + add (the arena's freed ranges and the freed slots are reused), clear."""
    rng = np.random.default_rng(nkf)
    pool = rng.choice(nwords, min(150, nwords), replace=False)
    sizes = [1, 63, 64, 65, 200]
    kfs = [M.KF(k + 1, *rbow(rng, np.concatenate([rng.choice(pool, min(sizes[k % 5], len(pool)), replace=False), [0] if k % 7 == 0 else [], [nwords - 1] if k % 11 == 0 else []])))
           for k in range(nkf)]
    covis(rng, kfs)
    P = Pair(backend, nwords, l1, check_state=nkf <= 65)
    for k in kfs:
        P.add(k)
    frame = M.KF(7, *rbow(rng, np.concatenate([rng.choice(pool, 120, replace=False), [0, nwords - 1]])))
    r = P.query(KFDB_RELOC, frame)
    assert nkf < 60 or len(r.scored) >= 2
    assert not P.query(KFDB_RELOC, frame).sharing                         # the same id again
    q = M.KF(9, *rbow(rng, rng.choice(pool, 100, replace=False)))
    q.connected = [kfs[int(j)] for j in rng.integers(0, nkf, 5)]
    r0 = P.query(KFDB_LOOP, q, 0.0)
    q.mnId = 10
    if len(r0.scored) >= 2:
        sc = sorted(float(s) for s, _ in r0.scored)
        P.query(KFDB_LOOP, q, float(np.float32(sc[len(sc) // 2])))
    for k in kfs[::3]:
        P.erase(k)
    fresh = [M.KF(5000 + i, *rbow(rng, rng.choice(pool, sizes[(i + 2) % 5] if sizes[(i + 2) % 5] <= len(pool) else len(pool), replace=False))) for i in range(len(kfs[::3]) + 2)]
    for k in fresh:
        P.add(k)
    covis(rng, P.live)
    frame.mnId = 11
    P.query(KFDB_RELOC, frame)
    P.states()
    P.clear()
    frame.mnId = 12
    assert not P.query(KFDB_RELOC, frame).sharing and len(P.db) == 0
    P.add(M.KF(9000, kfs[0].bow_id, kfs[0].bow_val))                     # (a new key frame: the fields of the cleared ones went with their slots)
    frame.mnId = 13
    P.query(KFDB_RELOC, frame)
    P.states()


def test_sweep_more_listed_than_the_lds_sort_holds(backend, l1):
    """4097 key frames that all share a word with the query, one more than k_kfdb_select sorts in LDS: with every count equal to 1 all of them are scored and
    ordered by (first shared word, add order) in device memory.  A second query with fewer than 4096 listed takes the LDS path on the same database."""
    rng = np.random.default_rng(4097)
    nwords, n = 10**6, 4097
    anchors = [0, 77, nwords - 1]
    kfs = [M.KF(k + 1, *rbow(rng, [anchors[int(rng.integers(0, 3))], 1000 + 2 * k, 1001 + 2 * k])) for k in range(n)]
    covis(rng, kfs, 2)
    P = Pair(backend, nwords, l1, check_state=False)
    for k in kfs:
        P.add(k)
    r = P.query(KFDB_RELOC, M.KF(3, *rbow(rng, anchors)))
    assert len(r.scored) == n
    r = P.query(KFDB_LOOP, M.KF(4, *rbow(rng, [77, 1000, 1001])), 0.0)
    assert 1000 < len(r.sharing) < 4096
    P.states()


def shared_bows(rng, nwords, nq, kf_words, shared):
    """a query of nq words and a key frame of kf_words words that share exactly `shared` of them, spread over the key frame's 64-word rounds"""
    ids = rng.choice(nwords - 2, nq + kf_words - shared, replace=False) + 1
    common, q_only, k_only = ids[:shared], ids[shared:nq], ids[nq:]
    if shared >= 2:
        common[0], common[1] = 0, nwords - 1                                # ids 0 and nwords - 1, shared: at the ends of both
    return rbow(rng, np.concatenate([common, q_only])), rbow(rng, np.concatenate([common, k_only]))


# ------------------------------------------------------------------------------------------------ 5: scores (and the scan's shapes)
def test_scores_double_for_double(backend, oracle):
    rng = np.random.default_rng(5)
    nwords = 10**6
    db = orb_slam2_amd.KeyFrameDatabase(nwords, library=backend)
    for nq, cases in [(300, [(1, 0), (1, 1), (63, 1), (64, 64), (65, 65), (200, 64), (200, 65), (200, 130), (8192, 0), (8192, 300), (200, 0)]),
                      (1, [(1, 1), (200, 1), (65, 0)]), (255, [(200, 129)]), (256, [(200, 129)]), (257, [(8192, 257)]), (8192, [(8192, 8192), (8192, 4000), (1, 1), (65, 64)])]:
        for kw, sh in cases:
            (qi, qv), (ki, kv) = shared_bows(rng, nwords, nq, kw, sh)
            assert len(qi) == nq and len(ki) == kw and len(np.intersect1d(qi, ki)) == sh
            s0, s1 = db.add(ki, kv), db.add(qi, qv)
            got = db.scores(qi, qv, [s0, s1, s0])
            want = np.array([oracle.voc_score(0, qi, qv, ki, kv), oracle.voc_score(0, qi, qv, qi, qv), oracle.voc_score(0, qi, qv, ki, kv)])
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (nq, kw, sh, got, want)
            # the same pairs through a query: the key frame that IS the query shares every word and is always scored, with the float of the same double
            s2 = db.add(ki, kv)
            hits, nsharing, minc = db.query(KFDB_RELOC, 1, qi, qv)
            assert nsharing == 1 + 2 * (sh > 0) and minc == int(np.float32(nq) * np.float32(0.8))
            by_slot = {int(h["slot"]): h for h in hits}
            assert int(by_slot[s1]["words"]) == nq and bits(by_slot[s1]["score"]) == bits(np.float32(want[1]))
            assert (s0 in by_slot) == (s2 in by_slot) == (sh > minc)
            if sh > minc:
                assert int(by_slot[s0]["words"]) == sh and bits(by_slot[s2]["score"]) == bits(np.float32(want[0])) and [int(h["slot"]) for h in hits] == [s0, s1, s2]
            db.clear()
    assert len(db.scores([3], [1.0], [])) == 0


# ------------------------------------------------------------------------------------------------ 4: a resident frame
def test_query_frame_reads_the_resident_bow(backend):
    from orb_slam2_amd import synth
    w, h, n = 320, 240, 300
    ex = orb_slam2_amd.ORBextractor(n, 1.2, 8, 20, 7, w, h, max_batch=2, library=backend)
    voc = orb_slam2_amd.ORBVocabulary(VOC, library=backend)
    ex.extract_batch([synth.frame(w, h, seed=21), synth.frame(w, h, seed=22)])
    voc.compute_bow(ex, 2, levelsup=4)
    bows = [voc.fetch_bow(ex, f)[:2] for f in range(2)]
    assert len(bows[0][0]) > 10 and len(bows[1][0]) > 10
    rng = np.random.default_rng(3)
    a, b = orb_slam2_amd.KeyFrameDatabase(voc.size(), library=backend), orb_slam2_amd.KeyFrameDatabase(voc.size(), library=backend)
    for k in range(40):
        bow = rbow(rng, rng.choice(voc.size(), int(rng.integers(5, 120)), replace=False))
        assert a.add(*bow) == b.add(*bow)
    for f in range(2):
        for kind in (KFDB_RELOC, KFDB_LOOP):
            ha, na, ma = a.query_frame(kind, 5 + f, ex, voc, frame=f, excluded=[1, 2], min_score=0.01)
            hb, nb, mb = b.query(kind, 5 + f, bows[f][0], bows[f][1], excluded=[1, 2], min_score=0.01)
            assert na == nb > 0 and ma == mb and ha.tobytes() == hb.tobytes()
    for s in range(40):
        for kind in (KFDB_RELOC, KFDB_LOOP):
            assert a.state(kind, s) == b.state(kind, s)
    with pytest.raises(orb_slam2_amd.OrbHipError):
        a.query_frame(KFDB_RELOC, 9, ex, voc, frame=2)
    other = orb_slam2_amd.KeyFrameDatabase(voc.size() + 1, library=backend)
    with pytest.raises(orb_slam2_amd.OrbHipError):
        other.query_frame(KFDB_RELOC, 9, ex, voc, frame=0)


# ------------------------------------------------------------------------------------------------ 6: errors
def test_errors_return_a_status_and_leave_the_database_usable(backend, l1):
    import ctypes as C
    L = orb_slam2_amd.lib(backend)
    h = C.c_void_p()
    for scoring in (1, 2, 3, 4, 5):
        assert L.orbhip_kfdb_create(C.byref(h), 0, 100, scoring) == orb_slam2_amd.orbhip.ERR_UNSUPPORTED and not h.value
        assert b"scoring" in L.orbhip_last_error()
    rng = np.random.default_rng(6)
    P = Pair(backend, 20000, l1)
    kfs = [M.KF(k + 1, *rbow(rng, rng.choice(400, 100, replace=False))) for k in range(12)]
    covis(rng, kfs)
    for k in kfs:
        P.add(k)
    db = P.db
    big = rbow(rng, rng.choice(20000, 8193, replace=False))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    slot, n, ns, mc = C.c_int(-5), C.c_int(0), C.c_int(0), C.c_int(0)
    hits = np.zeros(16, orb_slam2_amd.KFDB_HIT)
    assert L.orbhip_kfdb_add(db.h, p(big[0]), p(big[1]), 8193, C.byref(slot)) == orb_slam2_amd.orbhip.ERR_UNSUPPORTED and slot.value == -1
    assert L.orbhip_kfdb_query(db.h, 0, 3, p(big[0]), p(big[1]), 8193, None, 0, 0.0, p(hits), 16, C.byref(n), C.byref(ns), C.byref(mc)) == orb_slam2_amd.orbhip.ERR_UNSUPPORTED
    unsorted = (np.array([5, 4], np.uint32), np.array([0.5, 0.5]))
    assert L.orbhip_kfdb_add(db.h, p(unsorted[0]), p(unsorted[1]), 2, C.byref(slot)) == orb_slam2_amd.orbhip.ERR_INVALID
    beyond = (np.array([5, 20000], np.uint32), np.array([0.5, 0.5]))
    assert L.orbhip_kfdb_add(db.h, p(beyond[0]), p(beyond[1]), 2, C.byref(slot)) == orb_slam2_amd.orbhip.ERR_INVALID
    for bad in (-1, 12, 10**6):
        assert L.orbhip_kfdb_erase(db.h, bad) == orb_slam2_amd.orbhip.ERR_INVALID
        assert L.orbhip_kfdb_state(db.h, 0, bad, None, None, None) == orb_slam2_amd.orbhip.ERR_INVALID
        s = np.array([0, bad], np.int32); out = np.zeros(2)
        assert L.orbhip_kfdb_scores(db.h, p(kfs[0].bow_id), p(kfs[0].bow_val), 100, p(s), 2, p(out)) == orb_slam2_amd.orbhip.ERR_INVALID
    assert L.orbhip_kfdb_query(db.h, 2, 3, p(kfs[0].bow_id), p(kfs[0].bow_val), 100, None, 0, 0.0, p(hits), 16, C.byref(n), C.byref(ns), C.byref(mc)) == orb_slam2_amd.orbhip.ERR_INVALID
    P.states()                                                             # nothing above touched a key frame
    # a hit list that is too small: the status says so, *nhits the size needed, the first `cap` hits are delivered and the state is the completed query's
    frame = M.KF(21, *rbow(rng, rng.choice(400, 150, replace=False)))
    r = P.model.detect_reloc(frame)
    assert len(r.scored) >= 3
    st = L.orbhip_kfdb_query(db.h, 0, 21, p(frame.bow_id), p(frame.bow_val), len(frame.bow_id), None, 0, 0.0, p(hits), 2, C.byref(n), C.byref(ns), C.byref(mc))
    assert st == orb_slam2_amd.orbhip.ERR_CAPACITY and n.value == len(r.scored) and ns.value == len(r.sharing)
    assert [int(s) for s in hits["slot"][:2]] == [P.slot[id(k)] for _, k in r.scored[:2]] and hits["slot"][2] == 0
    P.states()
    frame.mnId = 22
    P.query(KFDB_RELOC, frame)                                             # later calls are exact
    assert len(db.query(KFDB_RELOC, 22, frame.bow_id, frame.bow_val)[0]) == 0
    # a candidate list that is too small
    frame.mnId = 23
    r = P.model.detect_reloc(frame)
    hits3, _, minc = db.query(KFDB_RELOC, 23, frame.bow_id, frame.bow_val)
    neigh = [[P.slot[id(k2)] for k2 in k.best_covisibles(10)] for _, k in r.scored]
    assert [int(c) for c in db.select(KFDB_RELOC, 23, minc, hits3, neigh)] == [P.slot[id(k)] for k in r.candidates]
    assert len(r.candidates) >= 1
    off, out = np.zeros(len(hits3) + 1, np.int32), np.zeros(1, np.int32)
    assert L.orbhip_kfdb_select(db.h, 0, 23, minc, 0.0, p(hits3), len(hits3), p(off), None, p(out), 0, C.byref(n)) == orb_slam2_amd.orbhip.ERR_CAPACITY and n.value >= 1
    bad_hit = hits3.copy(); bad_hit["slot"][0] = 99
    assert L.orbhip_kfdb_select(db.h, 0, 23, minc, 0.0, p(bad_hit), len(bad_hit), p(off), None, p(out), 1, C.byref(n)) == orb_slam2_amd.orbhip.ERR_INVALID
    P.states()


# ------------------------------------------------------------------------------------------------ 7: three threads
def test_two_threads_query_while_a_third_adds(backend, l1):
    """Tracking (RELOC) and LoopClosing (LOOP) query while LocalMapping adds.  Every answer must equal the serial model for SOME serial order of the adds; the
    script makes that order unique: the key frames added during a phase share no word with that phase's queries (whenever they land, they change no answer -
    but they grow the arenas and the slot arrays under the running queries), and the next phase's queries, which start after the adder has finished, meet them."""
    rng = np.random.default_rng(7)
    nwords, nphase, per_phase = 10**6, 3, 45
    P = Pair(backend, nwords, l1, check_state=False)
    band = lambda p: 1000 * p + rng.choice(200, 60, replace=False)         # phase p's words: [1000 p, 1000 p + 200)
    base = [M.KF(k + 1, *rbow(rng, band(0))) for k in range(30)]
    for k in base:
        P.add(k)
    next_id = [100]
    for p in range(nphase):
        new = [M.KF(next_id[0] + i, *rbow(rng, band(p + 1))) for i in range(per_phase)]
        next_id[0] += per_phase
        frames = [M.KF(1000 + 10 * p + i, *rbow(rng, np.concatenate([band(q) for q in range(p + 1)]))) for i in range(4)]
        loops = [M.KF(2000 + 10 * p + i, *rbow(rng, np.concatenate([band(q) for q in range(p + 1)]))) for i in range(4)]
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
        for k in new:                                                      # the model catches up: the adds are before the next phase's queries
            P.model.add(k)
            P.live.append(k)
        P.states()
    assert len(P.db) == 30 + nphase * per_phase
