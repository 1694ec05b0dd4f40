"""The vector overload of DetectRelocalizationCandidates of orb_slam2_amd/cpp/KeyFrameDatabase.cc (one batched device query, one batched selection) on the
emulation build: over the golden's script, with every run of consecutive relocalisation queries sent as one batch, it must return per frame the
vector<KeyFrame*> the reference's own class returned (tests/golden/kfdb_ref.npz); over a synthetic batch in which the order of the queries matters, the
model's (tests/kfdb_model.py).  The key frames are the stand-ins of tests/kfdb/ (kf_stub.cpp, stub/), the driver tests/kfdb/kf_batch_stub.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kfdb_model as M
import kfdb_batch_model as BM
from test_kfdb import rbow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kfdb_ref.npz")
VOC = os.path.join(ROOT, "tests", "golden", "voc_k6_L3_ref.txt")
vp = C.c_void_p
p = lambda a: a.ctypes.data_as(vp)


@pytest.fixture(scope="module")
def dropin(emu_lib, tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("kfdb_batch") / "libkfdb_batch_dropin.so")
    srcs = [os.path.join(ROOT, f) for f in ("orb_slam2_amd/cpp/KeyFrameDatabase.cc", "tests/kfdb/kf_stub.cpp", "tests/kfdb/kf_batch_stub.cpp", "orb_slam2_amd/cpp/ORBVocabulary.cc",
                                            "orb_slam2_amd/cpp/ORBextractor.cc")]
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-fPIC", "-shared", "-pthread", "-Wall", "-ffp-contract=off", "-DKFDB_STUB_OWN_TYPES", "-I" + os.path.join(ROOT, "tests/kfdb/stub"),
                        "-I" + os.path.join(ROOT, "include")] + srcs + ["-o", lib, "-L" + os.path.dirname(emu_lib), "-lorbhip_emu", "-Wl,-rpath," + os.path.dirname(emu_lib)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(lib)
    L.kfs_voc.restype = vp; L.kfs_voc.argtypes = [C.c_char_p]
    L.kfs_db.restype = vp; L.kfs_db.argtypes = [vp]
    L.kfs_db_free.argtypes = [vp]
    L.kfs_kf.restype = vp; L.kfs_kf.argtypes = [C.c_uint64, vp, vp, C.c_int]
    L.kfs_connect.argtypes = [vp, vp, C.c_int]
    L.kfs_add.argtypes = [vp, vp]; L.kfs_erase.argtypes = [vp, vp]; L.kfs_clear.argtypes = [vp]
    L.kfs_loop.argtypes = [vp, vp, C.c_float, vp, C.c_int]
    L.kfs_reloc.argtypes = [vp, C.c_uint64, vp, vp, C.c_int, vp, C.c_int]
    L.kfs_reloc_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int]
    return L


def reloc_batch(L, db, index, queries):
    """queries: [(qid, ids, vals)] -> per query the key frames' indices"""
    qid = np.array([q[0] for q in queries], np.uint64)
    off = np.concatenate([[0], np.cumsum([len(q[1]) for q in queries])]).astype(np.int32)
    bid = np.ascontiguousarray(np.concatenate([q[1] for q in queries]), np.uint32)
    bval = np.ascontiguousarray(np.concatenate([q[2] for q in queries]), np.float64)
    buf, out_off = (vp * 256)(), np.zeros(len(queries) + 1, np.int32)
    assert L.kfs_reloc_batch(db, len(queries), p(qid), p(off), p(bid), p(bval), buf, p(out_off), 256) == len(queries)
    assert out_off[-1] <= 256
    return [[index[buf[j]] for j in range(out_off[i], out_off[i + 1])] for i in range(len(queries))]


def test_vector_overload_replays_the_golden(dropin):
    L = dropin
    nkf, bows, ops, res = M.load_golden(GOLDEN)
    voc = L.kfs_voc(VOC.encode())
    assert voc
    db = L.kfs_db(voc)
    kfs = [L.kfs_kf(k, p(bows[k][0]), p(bows[k][1]), len(bows[k][0])) for k in range(nkf)]
    index = {h: k for k, h in enumerate(kfs)}
    buf = (vp * 64)()
    run, sizes = [], []

    def flush():
        if run:
            got = reloc_batch(L, db, index, [(op["qid"],) + tuple(bows[op["bow"]]) for _, op in run])
            for (i, op), g in zip(run, got):
                assert g == res[i][0], (i, op)
            sizes.append(len(run))
            del run[:]

    for i, (op, (cand, _)) in enumerate(zip(ops, res)):
        if op["op"] == "reloc":
            run.append((i, op))
            continue
        flush()
        if op["op"] == "add":
            L.kfs_add(db, kfs[op["kf"]])
        elif op["op"] == "erase":
            L.kfs_erase(db, kfs[op["kf"]])
        elif op["op"] == "clear":
            L.kfs_clear(db)
        elif op["op"] == "connect":
            L.kfs_connect(kfs[op["kf"]], kfs[op["other"]], op["w"])
        else:
            n = L.kfs_loop(db, kfs[op["kf"]], op["min_score"], buf, 64)
            assert [index[buf[j]] for j in range(n)] == cand, (i, op)
    flush()
    assert 3 in sizes and 2 in sizes and 1 in sizes, sizes                # the golden's RRR and RR runs and lone queries
    L.kfs_db_free(db)


def test_vector_overload_on_a_batch_whose_order_matters(dropin, oracle):
    """the fixture of tests/test_kfdb_batch.py's snapshot test: the second frame's candidates need the state right after the second query"""
    L = dropin
    rng = np.random.default_rng(11)
    wa, wb, wc = np.arange(100, 120), np.arange(180, 200), np.arange(40, 60)      # the golden's vocabulary has 216 words
    mk = [M.KF(1, *rbow(rng, wa)), M.KF(2, *rbow(rng, wb)), M.KF(3, *rbow(rng, wc))]
    mk[0].ordered, mk[1].ordered, mk[2].ordered = [mk[1]], [mk[0], mk[2]], [mk[0]]
    model = M.ModelDatabase(lambda a, b, c, d: oracle.voc_score(0, a, b, c, d))
    voc = L.kfs_voc(VOC.encode())
    db = L.kfs_db(voc)
    hk = [L.kfs_kf(k.mnId, p(k.bow_id), p(k.bow_val), len(k.bow_id)) for k in mk]
    index = {h: i for i, h in enumerate(hk)}
    for k, h in zip(mk, hk):
        model.add(k)
        L.kfs_add(db, h)
        for o in k.ordered:
            L.kfs_connect(h, hk[mk.index(o)], 1)
    qs = [M.KF(50, *rbow(rng, np.concatenate([wa, wc[:10]]))), M.KF(51, *rbow(rng, np.concatenate([wa[:5], wb]))), M.KF(51, *rbow(rng, np.concatenate([wa[:2], wb[:3], wc]))),
          M.KF(52, *rbow(rng, []))]
    want = BM.run_batch(model, 0, qs, [0.0] * 4, mk)
    assert want.count["stale_score_added"] >= 1 and want.count["repeated_qid"] == 1
    got = reloc_batch(L, db, index, [(q.mnId, q.bow_id, q.bow_val) for q in qs])
    assert got == [[mk.index(k) for k in r.candidates] for r in want.results] and any(got) and got[3] == []
    L.kfs_db_free(db)
