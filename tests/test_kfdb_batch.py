"""Batched key-frame database queries (orbhip_kfdb_query_batch / _query_frames / _batch_hits / _select_batch) against ORB_SLAM2's KeyFrameDatabase.

The chain is reference -> model -> product, as in tests/test_kfdb.py: the expected result of a batch is tests/kfdb_model.py's single members applied in
order (tests/kfdb_batch_model.py), which tests/golden/kfdb_ref.npz pins to the reference.  Everything is exact: slots, counts, raw float bits.

Sizes the sweep is built around: k_kfdb_scan_batch stages a tile of at most 16 queries and 8192 ids in LDS (batches of 1, 2, 16 and 17 one-word queries;
5 queries of 8192 words = 5 tiles; query sizes 0, 1, 255, 256, 257, 8192 in one batch), searches 64 words of a key frame per round and handles four key
frames per workgroup pass (1, 4, 5 slots); the walks and the per-query sort pass over 256 / 1024 slots (1025 slots) and the sort leaves the LDS above
4096 hits (4097 slots all hit by each of 3 queries)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import orb_slam2_amd
from orb_slam2_amd import KFDB_LOOP, KFDB_RELOC
import kfdb_model as M
import kfdb_batch_model as BM
from test_kfdb import Pair, bits, covis, rbow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kfdb_ref.npz")
VOC = os.path.join(ROOT, "tests", "golden", "voc_k6_L3_ref.txt")
TILE_Q = 16                                                                # KB_TQ


@pytest.fixture(scope="module")
def l1(oracle):
    return lambda a, b, c, d: oracle.voc_score(0, a, b, c, d)


class BatchPair(Pair):
    """One script through the model and the product side by side, the queries sent as batches."""

    def batch(self, kind, queries, min_scores=None):
        nq = len(queries)
        min_scores = [0.0] * nq if min_scores is None else [float(np.float32(m)) for m in min_scores]
        want = BM.run_batch(self.model, kind, queries, min_scores, self.live)
        excluded = [[self.slot[id(k)] for k in q.connected if id(k) in self.slot] for q in queries] if kind == KFDB_LOOP else None
        b = self.db.query_batch(kind, [q.mnId for q in queries], [(q.bow_id, q.bow_val) for q in queries], excluded=excluded, min_score=min_scores if kind == KFDB_LOOP else None)
        assert len(b) == nq and b.hit_off[0] == 0
        for i, r in enumerate(want.results):
            hits = b.query_hits(i)
            assert b.nsharing[i] == len(r.sharing) and b.min_common[i] == r.min_common, i
            assert [(int(h["slot"]), bits(h["score"])) for h in hits] == [(self.slot[id(k)], bits(s)) for s, k in r.scored], i
            assert [int(h["words"]) for h in hits] == [want.fields[i][id(k)][1] for _, k in r.scored], i      # the words right after query i
        neigh = [[self.slot.get(id(k2), -1) for k2 in self.kf_of[int(h["slot"])].best_covisibles(10)] for h in b.hits]
        cand = self.db.select_batch(b, neigh)
        for i, r in enumerate(want.results):
            assert [int(c) for c in cand[i]] == [self.slot[id(k)] for k in r.candidates], i
        if self.check_state:
            self.states()
        return want, b


def replay_golden(P, send):
    """the golden's script with every run of consecutive same-kind queries handed to send(kind, [(op index, op)]) at its end"""
    nkf, bows, ops, res = M.load_golden(GOLDEN)
    kfs = [M.KF(k, *bows[k]) for k in range(nkf)]
    run, sizes = [], []

    def flush():
        if run:
            sizes.append(("loop" if run[0][1]["op"] == "loop" else "reloc", len(run)))
            send(kfs, bows, res, list(run))
            del run[:]

    for i, op in enumerate(ops):
        if op["op"] in ("loop", "reloc") and (not run or run[0][1]["op"] == op["op"]):
            run.append((i, op))
            continue
        flush()
        if op["op"] in ("loop", "reloc"):
            run.append((i, op))
        elif op["op"] == "add":
            P.add(kfs[op["kf"]])
        elif op["op"] == "erase":
            P.erase(kfs[op["kf"]])
        elif op["op"] == "clear":
            P.clear()
        elif op["op"] == "connect":
            kfs[op["kf"]].connected.append(kfs[op["other"]])
            if op["w"] > 0:
                kfs[op["kf"]].ordered.append(kfs[op["other"]])
    flush()
    return sizes


# ------------------------------------------------------------------------------------------------ 1: the golden
def test_golden_replayed_in_batches(backend, l1):
    P = BatchPair(backend, 216, l1)

    def send(kfs, bows, res, run):
        kind = KFDB_LOOP if run[0][1]["op"] == "loop" else KFDB_RELOC
        qs = [kfs[op["kf"]] if kind == KFDB_LOOP else M.KF(op["qid"], *bows[op["bow"]]) for _, op in run]
        want, _ = P.batch(kind, qs, [op["min_score"] for _, op in run] if kind == KFDB_LOOP else None)
        for (i, op), r, fields in zip(run, want.results, want.fields):
            assert [k.mnId for k in r.candidates] == res[i][0], (i, op)
            for kf in P.live:                                              # the model's fields after every query of the batch against the golden's
                q, w, s = fields[id(kf)]
                assert (q, w, bits(s)) == res[i][1][kf.mnId][kind], (i, op, kf.mnId)
        for kf in P.live:                                                  # the product's state after the batch against the golden's, both kinds
            for k2 in (0, 1):
                q, w, s = P.db.state(k2, P.slot[id(kf)])
                assert (q, w, bits(s)) == res[run[-1][0]][1][kf.mnId][k2], (run[-1], kf.mnId, k2)

    sizes = replay_golden(P, send)
    assert any(n >= 3 for _, n in sizes) and ("loop", 2) in sizes, sizes


# ------------------------------------------------------------------------------------------------ 2: shapes
def small_db(rng, P, nkf, pool, sizes=(1, 63, 64, 65, 200), erase_every=0):
    kfs = [M.KF(k + 1, *rbow(rng, rng.choice(pool, min(sizes[k % len(sizes)], len(pool)), replace=False))) for k in range(nkf)]
    covis(rng, kfs)
    for k in kfs:
        P.add(k)
    if erase_every:
        for k in kfs[1::erase_every]:
            P.erase(k)
    return kfs


@pytest.mark.parametrize("nq", [1, 2, TILE_Q, TILE_Q + 1])
def test_batch_sizes_around_a_tile_of_one_word_queries(backend, l1, nq):
    rng = np.random.default_rng(nq)
    nwords = 10**6
    pool = rng.choice(nwords, 40, replace=False)
    P = BatchPair(backend, nwords, l1)
    small_db(rng, P, 9, pool, sizes=(1, 5, 20))
    qs = [M.KF(100 + i % 3, *rbow(rng, [pool[i % len(pool)]])) for i in range(nq)]      # query ids repeat inside the batch
    want, _ = P.batch(KFDB_RELOC, qs)
    assert sum(len(r.sharing) for r in want.results) > 0
    assert nq < 4 or want.count["repeated_qid"] > 0
    for q in qs:
        q.connected = [P.live[int(j)] for j in rng.integers(0, len(P.live), 2)]
        q.mnId += 50
    P.batch(KFDB_LOOP, qs, [0.0] * nq)


def test_five_queries_of_8192_words_take_five_tiles(backend, l1):
    rng = np.random.default_rng(5)
    nwords = 10**6
    big = [rng.choice(nwords, 8192, replace=False) for _ in range(5)]
    P = BatchPair(backend, nwords, l1)
    kfs = [M.KF(1, *rbow(rng, big[0])), M.KF(2, *rbow(rng, np.concatenate([big[1][:4000], big[2][:4000]]))), M.KF(3, *rbow(rng, big[4][:200])),
           M.KF(4, *rbow(rng, np.concatenate([big[3][:7000], big[4][:65]]))), M.KF(5, *rbow(rng, []))]
    covis(rng, kfs)
    for k in kfs:
        P.add(k)
    want, _ = P.batch(KFDB_RELOC, [M.KF(20 + i, *rbow(rng, big[i])) for i in range(5)])
    assert all(len(q) == 8192 for q in big) and all(r.scored for r in want.results)


def test_mixed_query_and_key_frame_sizes_in_one_batch(backend, l1):
    """queries of 0, 1, 255, 256, 257 and 8192 words; key frames of 0, 1, 63, 64, 65, 200 and 8192 words sharing 0, 1, 64, 65 and more than 128 words"""
    rng = np.random.default_rng(6)
    nwords = 10**6
    ids = rng.permutation(nwords)[:30000]
    q8192 = ids[:8192]
    private = ids[8192:]
    shapes = [(0, 0), (1, 0), (1, 1), (63, 1), (64, 64), (65, 65), (200, 64), (200, 65), (200, 130), (8192, 0), (8192, 300), (8192, 8192)]      # (words, shared with the large query)
    kfs, o = [], 0
    for k, (n, sh) in enumerate(shapes):
        kfs.append(M.KF(k + 1, *rbow(rng, np.concatenate([q8192[np.linspace(0, 8191, sh).astype(int)] if sh else [], private[o:o + n - sh]]))))
        o += n - sh
        assert len(kfs[-1].bow_id) == n and len(np.intersect1d(kfs[-1].bow_id, q8192)) == sh
    covis(rng, kfs)
    P = BatchPair(backend, nwords, l1)
    for k in kfs:
        P.add(k)
    sizes = [0, 1, 255, 256, 257, 8192]
    qs = [M.KF(40 + i, *rbow(rng, q8192[:n] if n < 8192 else q8192)) for i, n in enumerate(sizes)]
    assert [len(q.bow_id) for q in qs] == sizes
    want, _ = P.batch(KFDB_RELOC, qs)
    assert not want.results[0].sharing and len(want.results[5].sharing) == 9
    for q in qs:
        q.mnId += 10
        q.connected = [kfs[4], kfs[11]]
    P.batch(KFDB_LOOP, qs[::-1], [0.0, 0.01, 0.0, 0.02, 0.0, 0.0])


@pytest.mark.parametrize("nkf", [1, 4, 5, 1025])
def test_slot_counts_with_erased_slots(backend, l1, nkf):
    rng = np.random.default_rng(nkf)
    nwords = 10**6
    pool = rng.choice(nwords, 150, replace=False)
    P = BatchPair(backend, nwords, l1, check_state=nkf <= 5)
    small_db(rng, P, nkf, pool, erase_every=3 if nkf > 4 else 0)
    covis(rng, P.live)
    qs = [M.KF(7 + i % 2, *rbow(rng, rng.choice(pool, 100, replace=False))) for i in range(3)]
    want, _ = P.batch(KFDB_RELOC, qs)
    assert nkf < 5 or all(r.scored for r in want.results[:2])
    for i, q in enumerate(qs):
        q.mnId = 20 + i
        q.connected = [P.live[int(j)] for j in rng.integers(0, len(P.live), 3)]
    P.batch(KFDB_LOOP, qs, [0.0, 0.05, 0.0])
    P.states()


def test_more_hits_than_the_lds_sort_holds(backend, l1):
    """4097 key frames all hit by each of 3 queries: every query's hits are ordered in device memory, each at its own place of the workspace"""
    rng = np.random.default_rng(4097)
    nwords, n = 10**6, 4097
    anchors = [0, 77, nwords - 1]
    kfs = [M.KF(k + 1, *rbow(rng, [anchors[int(rng.integers(0, 3))], 1000 + 2 * k, 1001 + 2 * k])) for k in range(n)]
    covis(rng, kfs, 2)
    P = BatchPair(backend, nwords, l1, check_state=False)
    for k in kfs:
        P.add(k)
    want, _ = P.batch(KFDB_RELOC, [M.KF(3 + i, *rbow(rng, anchors)) for i in range(3)])
    assert all(len(r.scored) == n for r in want.results)
    P.states()


# ------------------------------------------------------------------------------------------------ 2: where the order of the queries shows
def test_order_coupling_reloc_pins_the_snapshot(backend, l1):
    """A (20 words) is scored by query 0; query 1 shares 5 words with A and 20 with B, so A is listed below minCommonWords and keeps query 0's score;
    B is a hit of query 1 and A its covisible, so the second half of query 1 adds A's STALE score.  Query 2 repeats query 1's id; the first query's id is
    the one an earlier single call left in C."""
    rng = np.random.default_rng(11)
    nwords = 10**5
    wa, wb, wc = np.arange(100, 120), np.arange(200, 220), np.arange(300, 320)
    A, B, Cc = M.KF(1, *rbow(rng, wa)), M.KF(2, *rbow(rng, wb)), M.KF(3, *rbow(rng, wc))
    A.ordered, B.ordered, Cc.ordered = [B], [A, Cc], [A]
    P = BatchPair(backend, nwords, l1)
    for k in (A, B, Cc):
        P.add(k)
    P.query(KFDB_RELOC, M.KF(50, *rbow(rng, wc[:3])))                      # leaves query id 50 in C
    qs = [M.KF(50, *rbow(rng, np.concatenate([wa, wc[:10]]))), M.KF(51, *rbow(rng, np.concatenate([wa[:5], wb]))), M.KF(51, *rbow(rng, np.concatenate([wa[:2], wb[:3], wc])))]
    want, b = P.batch(KFDB_RELOC, qs)
    assert want.count["stale_score_added"] >= 1 and want.count["repeated_qid"] == 1 and want.count["qid_left_by_earlier_call"] == 1, want.count
    assert [k.mnId for _, k in want.results[1].scored] == [2] and bits(want.fields[1][id(A)][2]) == bits(want.fields[0][id(A)][2]) != 0
    # after the batch A's state differs from what query 1 saw: a select over the final state would not reproduce the candidates
    assert want.fields[2][id(A)] != want.fields[1][id(A)]


def test_order_coupling_loop_excluded_and_listed_in_both_orders(backend, l1):
    rng = np.random.default_rng(12)
    nwords = 10**5
    pool = np.arange(1000, 1060)
    P = BatchPair(backend, nwords, l1)
    kfs = small_db(rng, P, 12, pool, sizes=(20, 30, 40))
    qs = [M.KF(70 + i, *rbow(rng, rng.choice(pool, 35, replace=False))) for i in range(4)]
    qs[0].connected, qs[1].connected, qs[2].connected, qs[3].connected = [kfs[0], kfs[1]], [kfs[2]], [kfs[0], kfs[2], kfs[3]], []
    want, _ = P.batch(KFDB_LOOP, qs, [0.0, 0.02, 0.0, 0.03])
    assert want.count["excluded_then_listed"] >= 1 and want.count["listed_then_excluded"] >= 1, want.count
    qs2 = [M.KF(73, q.bow_id, q.bow_val) for q in qs[:2]]                  # the id the last call left, twice
    want, _ = P.batch(KFDB_LOOP, qs2, [0.0, 0.0])
    assert want.count["qid_left_by_earlier_call"] == 1 and want.count["repeated_qid"] == 1, want.count


@pytest.mark.parametrize("scoring", [0, 1, 2, 4, 5])
def test_every_scoring_in_a_batch(backend, oracle, scoring):
    rng = np.random.default_rng(20 + scoring)
    nwords = 10**6
    pool = rng.choice(nwords, 150, replace=False)
    P = BatchPair(backend, nwords, lambda a, b, c, d: oracle.voc_score(scoring, a, b, c, d))
    P.db.set_scoring(scoring)
    small_db(rng, P, 9, pool)
    want, _ = P.batch(KFDB_RELOC, [M.KF(7 + i, *rbow(rng, rng.choice(pool, 100, replace=False))) for i in range(3)])
    assert all(r.scored for r in want.results)
    with pytest.raises(orb_slam2_amd.OrbHipError):
        P.db.set_scoring(3)
    assert P.db.scoring == scoring


# ------------------------------------------------------------------------------------------------ 3: batch == sequence
def test_a_batch_equals_the_sequence_of_single_calls(backend):
    rng = np.random.default_rng(30)
    nwords = 10**6
    pool = rng.choice(nwords, 150, replace=False)
    a, b = orb_slam2_amd.KeyFrameDatabase(nwords, library=backend), orb_slam2_amd.KeyFrameDatabase(nwords, library=backend)
    nkf = 70
    for k in range(nkf):
        bow = rbow(rng, rng.choice(pool, int(rng.integers(1, 120)), replace=False))
        assert a.add(*bow) == b.add(*bow)
    neigh_of = [[int(j) for j in rng.integers(0, nkf, 4)] for _ in range(nkf)]
    for kind in (KFDB_RELOC, KFDB_LOOP):
        qids = [5, 6, 5, 7, 7, 8]
        bows = [rbow(rng, rng.choice(pool, int(n), replace=False)) for n in (100, 60, 90, 0, 120, 30)]
        excl = [[int(j) for j in rng.integers(0, nkf, 6)] for _ in qids]
        ms = [0.0, 0.02, 0.0, 0.0, 0.05, 0.0]
        bt = a.query_batch(kind, qids, bows, excluded=excl, min_score=ms)
        ca = a.select_batch(bt, [neigh_of[int(h["slot"])] for h in bt.hits])
        for i, qid in enumerate(qids):
            hits, ns, mc = b.query(kind, qid, *bows[i], excluded=excl[i], min_score=ms[i])
            cb = b.select(kind, qid, mc, hits, [neigh_of[int(h["slot"])] for h in hits], min_score=ms[i])
            assert bt.query_hits(i).tobytes() == hits.tobytes() and (bt.nsharing[i], bt.min_common[i]) == (ns, mc), (kind, i)
            assert ca[i].tolist() == cb.tolist(), (kind, i)
        assert len(bt.hits) > 10
        for s in range(nkf):
            assert a.state(kind, s) == b.state(kind, s)


# ------------------------------------------------------------------------------------------------ 4: resident frames
def test_query_frames_reads_the_resident_bows(backend):
    from orb_slam2_amd import synth
    w, h, n = 320, 240, 300
    ex = orb_slam2_amd.ORBextractor(n, 1.2, 8, 20, 7, w, h, max_batch=5, library=backend)
    voc = orb_slam2_amd.ORBVocabulary(VOC, library=backend)
    frames = [synth.frame(w, h, seed=31 + f) for f in range(5)]
    frames[3] = np.full((h, w), 128, np.uint8)                            # a frame with no key points: an empty BowVector
    ex.extract_batch(frames)
    voc.compute_bow(ex, 5, levelsup=4)
    bows = [voc.fetch_bow(ex, f)[:2] for f in range(5)]
    assert len(bows[3][0]) == 0 and all(len(bows[f][0]) > 10 for f in (0, 1, 2, 4))
    rng = np.random.default_rng(3)
    a, b = orb_slam2_amd.KeyFrameDatabase(voc.size(), library=backend), orb_slam2_amd.KeyFrameDatabase(voc.size(), library=backend)
    for k in range(40):
        bow = rbow(rng, rng.choice(voc.size(), int(rng.integers(5, 120)), replace=False))
        assert a.add(*bow) == b.add(*bow)
    for case, (kind, first, nq) in enumerate([(KFDB_RELOC, 0, 5), (KFDB_LOOP, 2, 3), (KFDB_RELOC, 4, 1)]):
        qids = [60 + 10 * case + i % 2 for i in range(nq)]
        excl = [[1, 2, 30 + i] for i in range(nq)]
        ra = a.query_frames(kind, qids, ex, voc, first_frame=first, excluded=excl, min_score=0.01)
        rb = b.query_batch(kind, qids, bows[first:first + nq], excluded=excl, min_score=0.01)
        assert ra.hit_off.tolist() == rb.hit_off.tolist() and ra.hits.tobytes() == rb.hits.tobytes() and len(ra.hits) > 0
        assert ra.nsharing.tolist() == rb.nsharing.tolist() and ra.min_common.tolist() == rb.min_common.tolist()
        for s in range(40):
            assert a.state(kind, s) == b.state(kind, s)
    with pytest.raises(orb_slam2_amd.OrbHipError):
        a.query_frames(KFDB_RELOC, [1, 2], ex, voc, first_frame=4)


# ------------------------------------------------------------------------------------------------ 5: the contract
def test_contract_of_the_batch_entries(backend, l1):
    L = orb_slam2_amd.lib(backend)
    E = orb_slam2_amd.orbhip
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rng = np.random.default_rng(40)
    P = BatchPair(backend, 20000, l1)
    kfs = [M.KF(k + 1, *rbow(rng, rng.choice(400, 100, replace=False))) for k in range(12)]
    covis(rng, kfs)
    for k in kfs:
        P.add(k)
    db = P.db
    qs = [M.KF(21 + i, *rbow(rng, rng.choice(400, 150, replace=False))) for i in range(3)]
    want = BM.run_batch(P.model, KFDB_RELOC, qs, [0.0] * 3, P.live)
    true_off = np.concatenate([[0], np.cumsum([len(r.scored) for r in want.results])]).astype(np.int32)
    assert true_off[3] >= 6
    qids = np.array([q.mnId for q in qs], np.uint64)
    boff = np.concatenate([[0], np.cumsum([len(q.bow_id) for q in qs])]).astype(np.int32)
    bid, bval = np.concatenate([q.bow_id for q in qs]), np.concatenate([q.bow_val for q in qs])
    hit_off, ns, mc, tok = np.zeros(4, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32), C.c_uint64(0)
    hits = np.zeros(64, orb_slam2_amd.KFDB_HIT)
    # too small a cap: the status says so, hit_off is true, the state is the completed batch's, the hits are fetched afterwards
    st = L.orbhip_kfdb_query_batch(db.h, 0, 3, p(qids), p(boff), p(bid), p(bval), None, None, None, p(hit_off), p(ns), p(mc), p(hits), 2, C.byref(tok))
    assert st == E.ERR_CAPACITY and hit_off.tolist() == true_off.tolist() and tok.value != 0
    assert ns.tolist() == [len(r.sharing) for r in want.results] and mc.tolist() == [r.min_common for r in want.results]
    P.states()
    assert L.orbhip_kfdb_batch_hits(db.h, tok.value, 0, 3, p(hits), 3) == E.ERR_CAPACITY
    assert L.orbhip_kfdb_batch_hits(db.h, tok.value, 1, 2, p(hits), 64) == E.OK
    assert [int(s) for s in hits["slot"][:true_off[3] - true_off[1]]] == [P.slot[id(k)] for r in want.results[1:] for _, k in r.scored]
    assert L.orbhip_kfdb_batch_hits(db.h, tok.value, 2, 2, p(hits), 64) == E.ERR_INVALID
    # add / erase between query and select: liveness is read at select time, a key frame added since is a new key frame
    assert L.orbhip_kfdb_batch_hits(db.h, tok.value, 0, 3, p(hits), 64) == E.OK
    victim = next(k2 for r in want.results for _, k in r.scored for k2 in k.best_covisibles(10) if all(k2 is not k3 for r2 in want.results for _, k3 in r2.scored))
    vslot = P.slot[id(victim)]
    P.erase(victim)
    fresh = M.KF(900, *rbow(rng, rng.choice(400, 100, replace=False)))
    assert P.add(fresh) == vslot                                           # the freed slot is reused: its snapshot cells belong to the erased key frame
    neigh = [[P.slot.get(id(k2), -1) if k2 is not victim else vslot for k2 in k.best_covisibles(10)] for r in want.results for _, k in r.scored]
    noff = np.concatenate([[0], np.cumsum([len(v) for v in neigh])]).astype(np.int32)
    nflat = np.ascontiguousarray(np.concatenate(neigh), np.int32)
    out, out_off = np.zeros(64, np.int32), np.zeros(4, np.int32)
    assert L.orbhip_kfdb_select_batch(db.h, tok.value, 0, p(hits), p(hit_off), p(noff), p(nflat), p(out), p(out_off), 64) == E.OK
    for k in P.live:                                                       # the model's second halves again, as the reference runs them with the victim erased
        k.ordered = [k2 for k2 in k.ordered if k2 is not victim]
    for i, (q, r) in enumerate(zip(qs, want.results)):
        acc_list, best_acc = [], np.float32(0)
        for si, k in r.scored:
            best_score, acc, best_kf = si, si, k
            for k2 in k.best_covisibles(10):
                fq, _, fs = want.fields[i][id(k2)]
                if fq != q.mnId:
                    continue
                acc = np.float32(acc + fs)
                if fs > best_score:
                    best_kf, best_score = k2, fs
            acc_list.append((acc, best_kf))
            best_acc = max(best_acc, acc)
        assert out[out_off[i]:out_off[i + 1]].tolist() == [P.slot[id(k)] for k in M.ModelDatabase._retain(acc_list, best_acc)], i
    assert L.orbhip_kfdb_select_batch(db.h, tok.value, 0, p(hits), p(hit_off), p(noff), p(nflat), p(out), p(out_off), 0) == E.ERR_CAPACITY and out_off[3] >= 1
    assert L.orbhip_kfdb_select_batch(db.h, tok.value, 1, p(hits), p(hit_off), p(noff), p(nflat), p(out), p(out_off), 64) == E.ERR_INVALID
    # superseded by a query of any form, and by clear
    P.query(KFDB_LOOP, M.KF(5, [3], [1.0]), 0.0)
    assert L.orbhip_kfdb_select_batch(db.h, tok.value, 0, p(hits), p(hit_off), p(noff), p(nflat), p(out), p(out_off), 64) == E.ERR_INVALID
    assert L.orbhip_kfdb_batch_hits(db.h, tok.value, 0, 1, p(hits), 64) == E.ERR_INVALID
    P.states()
    # a non-ascending BowVector in the LAST query: nothing changes
    bad = bid.copy(); bad[-1] = bad[-2]
    tok2 = C.c_uint64(7)
    assert L.orbhip_kfdb_query_batch(db.h, 0, 3, p(qids + 100), p(boff), p(bad), p(bval), None, None, None, p(hit_off), p(ns), p(mc), None, 0, C.byref(tok2)) == E.ERR_INVALID
    beyond = bid.copy(); beyond[-1] = 20000
    assert L.orbhip_kfdb_query_batch(db.h, 0, 3, p(qids + 100), p(boff), p(beyond), p(bval), None, None, None, p(hit_off), p(ns), p(mc), None, 0, C.byref(tok2)) == E.ERR_INVALID
    assert L.orbhip_kfdb_query_batch(db.h, 1, 3, p(qids + 100), p(boff), p(bid), p(bval), None, None, None, p(hit_off), p(ns), p(mc), None, 0, C.byref(tok2)) == E.ERR_INVALID      # LOOP without lists
    assert L.orbhip_kfdb_query_batch(db.h, 2, 3, p(qids + 100), p(boff), p(bid), p(bval), None, None, None, p(hit_off), p(ns), p(mc), None, 0, C.byref(tok2)) == E.ERR_INVALID
    P.states()
    # an empty batch does nothing; an oversize one is refused with nothing changed
    assert L.orbhip_kfdb_query_batch(db.h, 0, 0, None, None, None, None, None, None, None, p(hit_off), None, None, None, 0, C.byref(tok2)) == E.OK and hit_off[0] == 0
    nbig = (1 << 27) // 64 + 1                                             # 12 key frames: a slot capacity of 64
    zeros = np.zeros(nbig + 1, np.int32)
    assert L.orbhip_kfdb_query_batch(db.h, 0, nbig, p(np.zeros(nbig, np.uint64)), p(zeros), None, None, None, None, None, p(zeros.copy()), None, None, None, 0, C.byref(tok2)) == E.ERR_UNSUPPORTED
    assert b"split" in L.orbhip_last_error()
    P.states()
    b = db.query_batch(KFDB_RELOC, [31], [(qs[0].bow_id, qs[0].bow_val)])   # a token outlives an empty batch and dies with clear
    assert L.orbhip_kfdb_query_batch(db.h, 0, 0, None, None, None, None, None, None, None, p(hit_off), None, None, None, 0, C.byref(tok2)) == E.OK
    assert L.orbhip_kfdb_batch_hits(db.h, b.token, 0, 1, p(hits), 64) == E.OK
    db.clear()
    assert L.orbhip_kfdb_batch_hits(db.h, b.token, 0, 1, p(hits), 64) == E.ERR_INVALID
    b = db.query_batch(KFDB_RELOC, [1, 2], [(qs[0].bow_id, qs[0].bow_val)] * 2)      # an empty database
    assert b.hit_off.tolist() == [0, 0, 0] and all(len(c) == 0 for c in db.select_batch(b, []))


# ------------------------------------------------------------------------------------------------ 5: threads
def test_two_threads_batch_while_a_third_adds(backend, l1):
    """As tests/test_kfdb.py's threading test, the queries in batches: the key frames added during a phase share no word with that phase's queries."""
    rng = np.random.default_rng(7)
    nwords, nphase, per_phase = 10**6, 3, 45
    P = BatchPair(backend, nwords, l1, check_state=False)
    band = lambda ph: 1000 * ph + rng.choice(200, 60, replace=False)
    for k in [M.KF(k + 1, *rbow(rng, band(0))) for k in range(30)]:
        P.add(k)
    next_id = 100
    for ph in range(nphase):
        new = [M.KF(next_id + i, *rbow(rng, band(ph + 1))) for i in range(per_phase)]
        next_id += per_phase
        frames = [M.KF(1000 + 10 * ph + i, *rbow(rng, np.concatenate([band(q) for q in range(ph + 1)]))) for i in range(4)]
        loops = [M.KF(2000 + 10 * ph + i, *rbow(rng, np.concatenate([band(q) for q in range(ph + 1)]))) for i in range(4)]
        for q in loops:
            q.connected = [P.live[int(j)] for j in rng.integers(0, len(P.live), 4)]
        want = {}
        for kind, qs in ((KFDB_RELOC, frames), (KFDB_LOOP, loops)):
            w = BM.run_batch(P.model, kind, qs, [0.05] * 4, P.live)
            for q, r, f in zip(qs, w.results, w.fields):
                want[q.mnId] = (len(r.sharing), r.min_common, [(P.slot[id(k)], bits(s), f[id(k)][1]) for s, k in r.scored])
        got, errors = {}, []

        def run_queries(kind, qs):
            try:
                for half in (qs[:2], qs[2:]):
                    ex = [[P.slot[id(k)] for k in q.connected] for q in half] if kind == KFDB_LOOP else None
                    b = P.db.query_batch(kind, [q.mnId for q in half], [(q.bow_id, q.bow_val) for q in half], excluded=ex, min_score=0.05 if kind == KFDB_LOOP else None)
                    for i, q in enumerate(half):
                        got[q.mnId] = (int(b.nsharing[i]), int(b.min_common[i]), [(int(h["slot"]), bits(h["score"]), int(h["words"])) for h in b.query_hits(i)])
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
        assert got == want, ph
        for k in new:
            P.model.add(k)
            P.live.append(k)
        P.states()
    assert len(P.db) == 30 + nphase * per_phase
