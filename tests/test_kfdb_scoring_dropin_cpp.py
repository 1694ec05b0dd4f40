"""orb_slam2_amd/cpp/KeyFrameDatabase.cc under a vocabulary whose scoring object is not L1_NORM, on the emulation build: the drop-in class must score with
what the vocabulary declares (ORBVocabulary::getScoringType, read at the constructor and at every Detect), so the scripts of tests/golden/kfdb_scoring_ref.npz
replayed through DetectLoopCandidates / DetectRelocalizationCandidates must return the vector<KeyFrame*> the reference's own class returned.  The key frames
are the stand-ins of tests/kfdb/; everything is compiled into the test's temporary directory."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kfdb_scoring_golden as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dropin(emu_lib, tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("kfdb_scoring") / "libkfdb_scoring_dropin.so")
    srcs = [os.path.join(ROOT, "orb_slam2_amd/cpp/KeyFrameDatabase.cc"), os.path.join(ROOT, "tests/kfdb/kf_stub.cpp"), os.path.join(ROOT, "tests/kfdb/voc_scoring_shim.cpp"),
            os.path.join(ROOT, "orb_slam2_amd/cpp/ORBVocabulary.cc"), os.path.join(ROOT, "orb_slam2_amd/cpp/ORBextractor.cc")]
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-fPIC", "-shared", "-pthread", "-Wall", "-ffp-contract=off", "-DKFDB_STUB_OWN_TYPES", "-I" + os.path.join(ROOT, "tests/kfdb/stub"),
                        "-I" + os.path.join(ROOT, "include")] + srcs + ["-o", lib, "-L" + os.path.dirname(emu_lib), "-lorbhip_emu", "-Wl,-rpath," + os.path.dirname(emu_lib)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(lib)
    vp = C.c_void_p
    L.kfs_voc.restype = vp; L.kfs_voc.argtypes = [C.c_char_p]
    L.kfs_voc_free.argtypes = [vp]
    L.kfs_voc_set_scoring.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
    L.kfs_voc_get.argtypes = [vp, vp]
    L.kfs_voc_save.argtypes = [vp, C.c_char_p]
    L.kfs_db_try.restype = vp; L.kfs_db_try.argtypes = [vp, C.c_char_p, C.c_int]
    L.kfs_db_free.argtypes = [vp]
    L.kfs_kf.restype = vp; L.kfs_kf.argtypes = [C.c_uint64, vp, vp, C.c_int]
    L.kfs_connect.argtypes = [vp, vp, C.c_int]
    L.kfs_add.argtypes = [vp, vp]; L.kfs_erase.argtypes = [vp, vp]; L.kfs_clear.argtypes = [vp]
    L.kfs_loop.argtypes = [vp, vp, C.c_float, vp, C.c_int]
    L.kfs_reloc.argtypes = [vp, C.c_uint64, vp, vp, C.c_int, vp, C.c_int]
    return L


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def info(L, voc):
    out = np.zeros(4, np.int32)
    L.kfs_voc_get(voc, p(out))
    return [int(x) for x in out]


def replay(L, voc, scoring, switch=False):
    """the golden's script under `scoring` through a new database on `voc`: every query's candidates must be the reference's.  switch: the vocabulary is
    given that scoring only after the database has been built on it"""
    nkf, bows, ops, res, _, _ = SG.load(scoring)
    msg = C.create_string_buffer(1024)
    db = L.kfs_db_try(voc, msg, 1024)
    assert db, msg.value
    if switch:
        assert info(L, voc)[0] != scoring and L.kfs_voc_set_scoring(voc, scoring, msg, 1024) == 0
    kfs = [L.kfs_kf(k, p(bows[k][0]), p(bows[k][1]), len(bows[k][0])) for k in range(nkf)]
    index = {h: k for k, h in enumerate(kfs)}
    buf = (C.c_void_p * 64)()
    nq = ncand = 0
    for i, (op, (cand, _)) in enumerate(zip(ops, res)):
        if op["op"] == "add":
            L.kfs_add(db, kfs[op["kf"]])
        elif op["op"] == "erase":
            L.kfs_erase(db, kfs[op["kf"]])
        elif op["op"] == "clear":
            L.kfs_clear(db)
        elif op["op"] == "connect":
            L.kfs_connect(kfs[op["kf"]], kfs[op["other"]], op["w"])
        else:
            if op["op"] == "loop":
                n = L.kfs_loop(db, kfs[op["kf"]], op["min_score"], buf, 64)
            else:
                b = bows[op["bow"]]
                n = L.kfs_reloc(db, op["qid"], p(b[0]), p(b[1]), len(b[0]), buf, 64)
            assert [index[buf[j]] for j in range(n)] == cand, (scoring, i, op)
            nq += 1; ncand += n
    assert nq >= 10 and ncand >= 5
    L.kfs_db_free(db)


@pytest.mark.parametrize("scoring", SG.SCORINGS)
def test_dropin_class_scores_as_the_vocabulary_file_declares(dropin, tmp_path, scoring):
    L = dropin
    voc = L.kfs_voc(SG.write_vocabulary(scoring, tmp_path / "voc.txt").encode())
    assert voc and info(L, voc) == [scoring, 0, 6, 3]
    replay(L, voc, scoring)
    L.kfs_voc_free(voc)


def test_set_scoring_type_before_and_after_the_database_is_built(dropin, tmp_path):
    L = dropin
    msg = C.create_string_buffer(1024)
    voc = L.kfs_voc(SG.VOC.encode())
    assert voc and info(L, voc) == [0, 0, 6, 3]
    assert L.kfs_voc_set_scoring(voc, 1, msg, 1024) == 0                   # DBoW2::L2_NORM
    assert info(L, voc) == [1, 0, 6, 3]
    replay(L, voc, 1)
    out = tmp_path / "saved.txt"
    L.kfs_voc_save(voc, str(out).encode())
    lines = open(out).read().split("\n")
    assert lines[0] == "6 3  1 0" and lines[1:] == open(SG.VOC).read().split("\n")[1:]
    replay(L, voc, 4, switch=True)                                         # a database built under L2 follows the vocabulary to Bhattacharyya at its next Detect
    assert L.kfs_voc_set_scoring(voc, 6, msg, 1024) == 1 and b"scoring" in msg.value and info(L, voc)[0] == 4
    L.kfs_voc_free(voc)


def test_a_kl_vocabulary_is_refused_by_the_constructor(dropin, tmp_path):
    L = dropin
    voc = L.kfs_voc(SG.write_vocabulary(3, tmp_path / "voc_kl.txt").encode())
    assert voc and info(L, voc)[0] == 3
    msg = C.create_string_buffer(1024)
    assert not L.kfs_db_try(voc, msg, 1024)
    assert b"KL" in msg.value and b"KeyFrameDatabase" in msg.value
    L.kfs_voc_free(voc)
