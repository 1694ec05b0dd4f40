"""Freezes what ORB_SLAM2's own KeyFrameDatabase does with a recorded script of calls -> tests/golden/kfdb_ref.npz (data only).

Runs only where the reference checkout is mounted (/root/reference, or $ORBSLAM_REF).  The reference's src/KeyFrameDatabase.cc is compiled where it lies,
into a temporary directory (never into this repository), with the include flags of tests/test_apply_dropin.py::_flags, beside the test-owned stub
tests/kfdb/kf_stub.cpp (the few KeyFrame / Frame members that file needs) and this repository's ORBVocabulary on the emulation build, whose score is pinned
against the reference's DBoW2 elsewhere.  The script is played through the reference's add / erase / DetectLoopCandidates /
DetectRelocalizationCandidates; after every call the returned candidates and every key frame's six query fields are recorded.  The same script runs through
tests/kfdb_model.py beside it: the generator refuses to write a golden whose script lacks one of the situations the tests are about.

    python tests/golden/make_golden_kfdb.py
"""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("ORBSLAM_REF", "/root/reference")
VOC = os.path.join(ROOT, "tests", "golden", "voc_k6_L3_ref.txt")
OUT = os.path.join(ROOT, "tests", "golden", "kfdb_ref.npz")
NWORDS = 216


def make_script(seed=20240):
    """-> (bows: list of (ids, vals); ops: list of dicts).  Key frame k has mnId k; bows[k] is its BowVector; bows past the key frames are frames' (RELOC queries)."""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(NWORDS, 50, replace=False))

    def bow(ids):
        ids = np.unique(np.asarray(ids)).astype(np.uint32)
        v = rng.random(len(ids)) + 0.05
        return ids, v / v.sum()

    nkf = 14
    bows = [bow(rng.choice(pool, 40, replace=False)) for _ in range(nkf)]
    bows[12] = bow(rng.choice(NWORDS, 8, replace=False))                      # a key frame off the pool
    bows[13] = bow(np.arange(NWORDS))                                         # every word, ids 0 and nwords - 1
    frames = {
        "A": bow(bows[3][0]),                                                 # key frame 3's words: it is scored alone or nearly so
        "C": bow(np.concatenate([bows[2][0], bows[3][0][:2]])),               # key frame 2's words and two of key frame 3's: 3 shares few words and keeps its stale score
        "D": bow(rng.choice(pool, 45, replace=False)),
        "E": bow(rng.choice(NWORDS, 30, replace=False)),
        "Z": bow([int(pool[0])]),
    }
    names = list(frames)
    for n in names:
        bows.append(frames[n])
    fr = {n: nkf + i for i, n in enumerate(names)}
    ops = []
    for k in range(1, 9):
        ops.append({"op": "add", "kf": k})
    for k in range(1, 9):                                                     # covisibility: ordered neighbours (weight > 0) and connected-only ones (weight 0)
        ops.append({"op": "connect", "kf": k, "other": k % 8 + 1, "w": 5})
        ops.append({"op": "connect", "kf": k, "other": (k + 2) % 8 + 1, "w": 3})
    ops.append({"op": "connect", "kf": 2, "other": 3, "w": 9})
    ops += [
        {"op": "reloc", "qid": 0, "bow": fr["D"]},                            # query id 0 against fresh key frames: nothing
        {"op": "loop", "kf": 0, "min_score": 0.0},                            # ... and the loop form of it (key frame 0 has mnId 0)
        {"op": "reloc", "qid": 5, "bow": fr["A"]},
        {"op": "reloc", "qid": 5, "bow": fr["A"]},                            # a repeated query id: nothing, the counts go on
        {"op": "reloc", "qid": 6, "bow": fr["C"]},                            # depends on key frame 3's stale score
        {"op": "erase", "kf": 5},
        {"op": "reloc", "qid": 7, "bow": fr["D"]},
        {"op": "add", "kf": 9}, {"op": "add", "kf": 10}, {"op": "add", "kf": 12}, {"op": "add", "kf": 13},
        {"op": "connect", "kf": 11, "other": 2, "w": 0}, {"op": "connect", "kf": 11, "other": 4, "w": 4}, {"op": "connect", "kf": 11, "other": 5, "w": 2},
        {"op": "loop", "kf": 11, "min_score": None},                          # connected key frames, a minScore that removes some hits (filled in below)
        {"op": "loop", "kf": 11, "min_score": 0.0},                           # the same id again
        {"op": "reloc", "qid": 8, "bow": fr["E"]},
        {"op": "reloc", "qid": 9, "bow": fr["Z"]},                            # one word
        {"op": "erase", "kf": 2}, {"op": "add", "kf": 11},
        {"op": "loop", "kf": 10, "min_score": 0.0},
        {"op": "reloc", "qid": 10, "bow": fr["D"]},
        {"op": "clear"},
        {"op": "reloc", "qid": 11, "bow": fr["D"]},                           # an empty database
    ]
    return nkf, bows, ops


def play_model(nkf, bows, ops, score):
    """The script through tests/kfdb_model.py -> per op (candidates as key-frame indices or None, fields [nkf][2 kinds] of (query, words, score), the Result)."""
    import kfdb_model as M
    kfs = [M.KF(k, *bows[k]) for k in range(nkf)]
    db = M.ModelDatabase(score)
    out = []
    for op in ops:
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
        elif op["op"] == "reloc":
            r = db.detect_reloc(M.KF(op["qid"], *bows[op["bow"]]))
        cand = None if r is None else [k.mnId for k in r.candidates]
        out.append((cand, [[kfs[k].fields(kind) for kind in (0, 1)] for k in range(nkf)], r))
    return out


def build_reference(tmp):
    from conftest import EMU_LIB                                          # tests/conftest.py
    from oracle.orbslam_ref import _locked_make
    _locked_make(["-C", os.path.join(ROOT, "orb_slam2_amd", "csrc"), "-s", "emu"])
    co = os.path.join(tmp, "include")
    shutil.copytree(os.path.join(REF, "include"), co)
    os.remove(os.path.join(co, "Converter.h"))                             # needs Eigen / g2o: oracle/ref_shim's stand-in is found instead (as in tests/test_apply_dropin.py)
    ora = os.path.join(ROOT, "oracle")
    flags = ["-std=c++14", "-w", "-O1", "-fPIC", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-DCVLITE_ALGEBRA", "-DORBHIP_USE_OPENCV", "-DORBSLAM_DROPIN_BUILD", "-DORBHIP_USE_DBOW2_TYPES",
             "-include", os.path.join(ora, "ref_shim/dropin/ORBVocabulary.h"),
             "-I" + co, "-I" + os.path.join(ora, "ref_shim"), "-I" + REF, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(REF, "Thirdparty/DBoW2")]
    lib = os.path.join(tmp, "libkfdb_reference.so")
    objs = []
    # the reference's translation unit and the stub see the reference's headers first; this repository's vocabulary class (and the extractor it names) its own
    for src, first in ((os.path.join(REF, "src/KeyFrameDatabase.cc"), co), (os.path.join(ROOT, "tests/kfdb/kf_stub.cpp"), co),
                       (os.path.join(REF, "Thirdparty/DBoW2/DBoW2/BowVector.cpp"), co), (os.path.join(REF, "Thirdparty/DBoW2/DBoW2/FeatureVector.cpp"), co),
                       (os.path.join(ROOT, "orb_slam2_amd/cpp/ORBVocabulary.cc"), os.path.join(ROOT, "include")), (os.path.join(ROOT, "orb_slam2_amd/cpp/ORBextractor.cc"), os.path.join(ROOT, "include"))):
        objs.append(os.path.join(tmp, os.path.basename(src) + ".o"))
        subprocess.run(["g++", "-c", "-I" + first] + flags + [src, "-o", objs[-1]], check=True)
    subprocess.run(["g++", "-shared", "-pthread"] + objs + ["-o", lib, "-L" + os.path.dirname(EMU_LIB), "-lorbhip_emu", "-Wl,-rpath," + os.path.dirname(EMU_LIB)], check=True)
    return lib


def play_reference(lib, nkf, bows, ops):
    L = C.CDLL(lib)
    vp = C.c_void_p
    L.kfs_voc.restype = vp; L.kfs_voc.argtypes = [C.c_char_p]
    L.kfs_db.restype = vp; L.kfs_db.argtypes = [vp]
    L.kfs_kf.restype = vp; L.kfs_kf.argtypes = [C.c_uint64, vp, vp, C.c_int]
    L.kfs_connect.argtypes = [vp, vp, C.c_int]
    for f in (L.kfs_add, L.kfs_erase):
        f.argtypes = [vp, vp]
    L.kfs_clear.argtypes = [vp]
    L.kfs_loop.argtypes = [vp, vp, C.c_float, vp, C.c_int]
    L.kfs_reloc.argtypes = [vp, C.c_uint64, vp, vp, C.c_int, vp, C.c_int]
    L.kfs_fields.argtypes = [vp, vp, vp, vp]
    p = lambda a: a.ctypes.data_as(vp)
    voc = L.kfs_voc(VOC.encode())
    assert voc
    db = L.kfs_db(voc)
    kfs = [L.kfs_kf(k, p(bows[k][0]), p(bows[k][1]), len(bows[k][0])) for k in range(nkf)]
    index = {h: k for k, h in enumerate(kfs)}
    out = []
    buf = (vp * 64)()
    for op in ops:
        cand = None
        if op["op"] == "add":
            L.kfs_add(db, kfs[op["kf"]])
        elif op["op"] == "erase":
            L.kfs_erase(db, kfs[op["kf"]])
        elif op["op"] == "clear":
            L.kfs_clear(db)
        elif op["op"] == "connect":
            L.kfs_connect(kfs[op["kf"]], kfs[op["other"]], op["w"])
        elif op["op"] == "loop":
            n = L.kfs_loop(db, kfs[op["kf"]], op["min_score"], buf, 64)
            cand = [index[buf[i]] for i in range(n)]
        elif op["op"] == "reloc":
            b = bows[op["bow"]]
            n = L.kfs_reloc(db, op["qid"], p(b[0]), p(b[1]), len(b[0]), buf, 64)
            cand = [index[buf[i]] for i in range(n)]
        fields = []
        for k in range(nkf):
            q = np.zeros(2, np.uint64); w = np.zeros(2, np.int32); s = np.zeros(2, np.float32)
            L.kfs_fields(kfs[k], p(q), p(w), p(s))
            fields.append([(int(q[i]), int(w[i]), np.float32(s[i])) for i in (0, 1)])
        out.append((cand, fields, None))
    return out


def check_script(ops, bows, model):
    """the situations the tests are about are in the script"""
    seen = {"query id 0": False, "repeated query id": False, "stale score": False, "minScore removes hits": False, "connected key frames": False,
            "erase between queries": False, "same first shared word": False}
    connected_of = {}
    for op in ops:
        if op["op"] == "connect":
            connected_of.setdefault(op["kf"], []).append(op["other"])
    scored_ever, prev, erased, nqueries = set(), None, False, 0
    for op, (cand, fields, r) in zip(ops, model):
        if op["op"] == "erase" and nqueries:
            erased = True
        if r is None:
            continue
        qid = op["qid"] if op["op"] == "reloc" else op["kf"]
        if qid == 0 and not r.sharing:
            seen["query id 0"] = True
        if prev == (op["op"], qid) and not r.sharing:
            seen["repeated query id"] = True
        prev = (op["op"], qid)
        seen["erase between queries"] |= erased
        nqueries += 1
        now = set(k.mnId for _, k in r.scored)
        if op["op"] == "reloc":
            for _, k in r.scored:
                for k2 in k.best_covisibles(10):
                    if k2.mnRelocQuery == qid and k2.mnId not in now and k2.mnId in scored_ever and k2.mRelocScore != 0:
                        seen["stale score"] = True
            scored_ever |= now
        else:
            nscored = sum(1 for k in r.sharing if k.mnLoopWords > r.min_common)
            if op["min_score"] > 0 and 0 < len(r.scored) < nscored:
                seen["minScore removes hits"] = True
            if any(fields[c][1][1] == 1 and fields[c][1][0] != qid for c in connected_of.get(op["kf"], [])):
                seen["connected key frames"] = True
        if len(r.scored) >= 2:
            qb = bows[op["bow"]][0] if op["op"] == "reloc" else bows[op["kf"]][0]
            first = [int(np.intersect1d(qb, k.bow_id)[0]) for _, k in r.scored]
            seen["same first shared word"] |= len(set(first)) < len(first)
    missing = [k for k, v in seen.items() if not v]
    assert not missing, f"the script lacks: {missing}"


def main():
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit(f"{REF} is not mounted: the golden is made where the reference is")
    from oracle import orb_oracle as O
    O.build()
    score = lambda a, b, c, d: O.voc_score(0, a, b, c, d)
    nkf, bows, ops = make_script()
    # minScore of the LOOP query that must remove some hits: the median score of what it scores with minScore 0
    for op in ops:
        if op["op"] == "loop" and op["min_score"] is None:
            trial = [dict(o) for o in ops]
            for o in trial:
                if o["op"] == "loop" and o["min_score"] is None:
                    o["min_score"] = 0.0
            res = play_model(nkf, bows, trial, score)[ops.index(op)][2]
            sc = sorted(float(s) for s, _ in res.scored)
            assert len(sc) >= 3, "the LOOP query of the script scores fewer than three key frames"
            op["min_score"] = float(np.float32((sc[len(sc) // 2 - 1] + sc[len(sc) // 2]) / 2))
    model = play_model(nkf, bows, ops, score)
    check_script(ops, bows, model)
    with tempfile.TemporaryDirectory() as tmp:
        ref = play_reference(build_reference(tmp), nkf, bows, ops)
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
    np.savez_compressed(OUT, ops=np.frombuffer(json.dumps(ops).encode(), np.uint8), nkf=np.int32(nkf), nwords=np.int32(NWORDS),
                        bow_off=np.cumsum([0] + [len(b[0]) for b in bows]).astype(np.int32), bow_id=np.concatenate([b[0] for b in bows]).astype(np.uint32),
                        bow_val=np.concatenate([b[1] for b in bows]).astype(np.float64),
                        is_query=np.array([c is not None for c, _, _ in ref], np.uint8), cand_off=np.array(cand_off, np.int32), cand=np.array(cand, np.int32),
                        field_query=q, field_words=w, field_score_bits=s)
    agree = all(rc == mc for (rc, _, _), (mc, _, _) in zip(ref, model))
    print(f"{OUT}: {nops} calls, {int(sum(c is not None for c, _, _ in ref))} queries, {len(cand)} candidates; the model's candidates agree: {agree}")


if __name__ == "__main__":
    main()
