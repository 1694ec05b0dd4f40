"""Builds and drives tests/voc_train/ref_train.cpp: the reference's own TemplatedVocabulary::create, its k-means++ stream reseeded per node by a subclass
(DESIGN.md H14), compiled together with the reference's DBoW2 sources where they lie, into a directory the caller names (a temporary one: never into this
repository).  Two users: tests/golden/make_golden_voc_train.py and tools/voc_train_rate.py (the reference timed on one thread of the host)."""
import ctypes as C
import multiprocessing
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_sources(reference):
    """the REF_SRCS list of oracle/Makefile (read, not changed)"""
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    m = re.search(r"^REF_SRCS\s*:=\s*((?:.*\\\n)*.*)$", mk, re.M)
    dbow2 = os.path.join(reference, "Thirdparty", "DBoW2")
    return [s.replace("$(DBOW2)", dbow2) for s in m.group(1).replace("\\\n", " ").split()], dbow2


def build(tmp, reference, name="libvoc_train_ref.so", opt="-O2"):
    srcs, dbow2 = ref_sources(reference)
    lib = os.path.join(str(tmp), name)
    cmd = ["g++", "-std=c++14", "-fPIC", "-shared", opt, "-w", "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(ROOT, "include"), "-I" + dbow2,
           os.path.join(ROOT, "tests", "voc_train", "ref_train.cpp")] + srcs + ["-o", lib]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def train(lib, images, k, L, weighting=0, scoring=0, seed=0, text_path=None):
    """-> the same dict as voc_train_model.train (without stats), plus seconds: the time of create() alone"""
    R = C.CDLL(lib)
    vp = C.c_void_p
    R.vt_ref_create.restype = vp; R.vt_ref_create.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32]
    R.vt_ref_seconds.restype = C.c_double
    for f in ("vt_ref_free", "vt_ref_seconds", "vt_ref_nodes", "vt_ref_words"):
        getattr(R, f).argtypes = [vp]
    R.vt_ref_tree.argtypes = [vp] * 5; R.vt_ref_after.argtypes = [vp, vp]; R.vt_ref_word_docs.argtypes = [vp, vp]; R.vt_ref_save.argtypes = [vp, C.c_char_p]
    counts = np.array([len(f) for f in images], np.int32)
    desc = np.ascontiguousarray(np.concatenate([np.asarray(f, np.uint8).reshape(-1, 32) for f in images])) if counts.sum() else np.zeros((0, 32), np.uint8)
    h = R.vt_ref_create(_p(desc), _p(counts), len(counts), k, L, weighting, scoring, seed)
    try:
        nn, nw = R.vt_ref_nodes(h), R.vt_ref_words(h)
        out = dict(parent=np.zeros(nn, np.int32), leaf=np.zeros(nn, np.uint8), desc=np.zeros((nn, 32), np.uint8), weight=np.zeros(nn, np.float64),
                   ni=np.zeros(nw, np.int32), after=np.zeros_like(desc), seconds=R.vt_ref_seconds(h))
        R.vt_ref_tree(h, _p(out["parent"]), _p(out["leaf"]), _p(out["desc"]), _p(out["weight"]))
        R.vt_ref_after(h, _p(out["after"])); R.vt_ref_word_docs(h, _p(out["ni"]))
        if text_path:
            R.vt_ref_save(h, str(text_path).encode())
            out["text"] = open(text_path, "rb").read()
    finally:
        R.vt_ref_free(h)
    return out


def _child(conn, args, kw):
    try:
        conn.send(train(*args, **kw))
    except BaseException as e:                                                # noqa: BLE001
        conn.send(e)


def train_isolated(*args, **kw):
    """train() in a child process: the reference faults on some training sets (a cluster that loses all its features).  None when the child died."""
    ctx = multiprocessing.get_context("fork")
    a, b = ctx.Pipe(duplex=False)
    p = ctx.Process(target=_child, args=(b, args, kw))
    p.start(); b.close()
    try:
        out = a.recv()
    except EOFError:
        out = None
    p.join()
    if isinstance(out, BaseException):
        raise out
    return out
