"""orbhip_voc_create / orbhip_voc_save_text (orb_slam2_amd.ORBVocabulary.create / saveToTextFile) against DBoW2's TemplatedVocabulary::create and saveToTextFile.

The chain is reference -> model -> product.  tests/golden/voc_train_ref.npz (voc_train_model.CASES) and voc_train_shapes_ref.npz (voc_train_model.SHAPES)
hold what the reference's own create() made of the seeded training sets of tests/voc_train_model.py, its k-means++ stream reseeded per node (DESIGN.md H14;
tests/golden/make_golden_voc_train.py, which refuses to write unless the model reproduces the reference everywhere).  The product must reproduce the golden exactly: parents, leaf flags, node descriptors, word order, Ni per word,
the training features as create() leaves them, and the saved file byte for byte.  Weights are compared with math.log(ndocs / ni) evaluated here - the libm the
library itself calls - so that Ni is pinned exactly and a libm that differs from the golden's machine in the last bit cannot fail the test.

Sizes (orb_slam2_amd/csrc/orbhip_voc_train.hip): a node's features are cut into chunks of VT_CHUNK = 1024, a workgroup has 256 threads, a wavefront 64; the
root_M cases are one node of exactly M features around each of them, M = 5 and 10 the trivial case (one cluster per feature), 4097 a node of five chunks.

The SHAPES cases are made for what the first set never executes, and the golden keeps the model's counters of each (name/stats) so that
test_shapes_reach_their_situations fails when a case stops reaching what it was made for:
  big_few_values   a root of two chunks whose k-means++ stops at 3 of 5 centres (ncl != round in the seeding kernels, nc < k in k_vt_count / k_vt_mean_big /
                   k_vt_scatter), with a cluster of exactly one feature finished from the device-memory counters (vt_finalize's n < 2 by way of k_vt_mean_big),
                   and below it nodes of 1300 and 700 equal features: every Lloyd kernel with nc == 1;
  zero_cut_first, zero_cut_later   root keys whose rand() stream holds a 0 at draw 1 and at draw 3: the redraw of the cut while it is 0.0
                   (TemplatedVocabulary.h:887-891); of all 2^31 keys, 33 draw a 0 among draws 1 .. 31.  Both base seeds lie above 2^31;
  root_key_zero    a node key of 0: srand(0) is srand(1);
  wide_level       606 k-means nodes on level 7: three workgroups of the per-node kernels (k_vt_seed_first, k_vt_pass_end), and the level's Lloyd passes
                   end with a node of the third: it takes more passes than every one of the first 512;
  root_2048, root_2049   a node of exactly two chunks, and of two and one feature more;
  one_image        every reached word has log(1 / 1) = 0, printed as 0;  empty_runs: runs of two and three empty images and images of one feature in k_vt_docs.

Still not reached by any test: the bound of VT_MAX_PASSES = 512 Lloyd passes on a level (the reference has none).  A search of 193 300 small sets of tight blobs
with the model, at a bound of 60 passes, found 6384 that empty a cluster and none that cycled; no test is built on it."""
import ctypes as C
import hashlib
import math
import os
import threading

import numpy as np
import pytest

import orb_slam2_amd
import voc_train_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "voc_train_ref.npz")
GOLDEN_SHAPES = os.path.join(ROOT, "tests", "golden", "voc_train_shapes_ref.npz")
REF_VOC = os.path.join(ROOT, "tests", "golden", "voc_k6_L3_ref.txt")             # written by the reference's own saveToTextFile
INVALID, UNSUPPORTED = 1, 4           # orbhip_status


@pytest.fixture(scope="module")
def golden():
    out = {}
    for path in (GOLDEN, GOLDEN_SHAPES):
        g = np.load(path)
        assert not set(g.files) & set(out)
        out.update({k: g[k] for k in g.files})
    return out


_inputs = {}


def inputs(name):
    """the case's training set: made once, shared, never changed"""
    if name not in _inputs:
        imgs = M.case_images(name)
        for f in imgs:
            f.setflags(write=False)
        _inputs[name] = imgs
    return _inputs[name]


def parse(text):
    """a saved vocabulary -> k, L, scoring, weighting, parent, leaf, desc, the printed weights"""
    lines = text.decode().split("\n")
    assert lines[-1] == ""
    head = lines[0].split(" ")
    assert len(head) == 5 and head[2] == "", lines[0]                         # two spaces before the scoring field
    rows = [l.split(" ") for l in lines[1:-1]]
    for r in rows:
        assert len(r) == 36 and r[34] == "", r                                # FORB::toString's trailing space, then one more
    nn = len(rows) + 1
    parent = np.zeros(nn, np.int32); leaf = np.zeros(nn, np.uint8); desc = np.zeros((nn, 32), np.uint8); weight = np.zeros(nn)
    for i, r in enumerate(rows, 1):
        parent[i], leaf[i], desc[i], weight[i] = int(r[0]), int(r[1]), [int(b) for b in r[2:34]], float(r[35])
    return int(head[0]), int(head[1]), int(head[3]), int(head[4]), parent, leaf, desc, weight


def features_words(voc, feats):
    """word and full-precision weight of every feature, 8192 (the per-call limit of the transform) at a time"""
    w = [voc.transform_features(feats[i:i + 8192], 0)[:2] for i in range(0, len(feats), 8192)]
    return (np.concatenate([x[0] for x in w]), np.concatenate([x[1] for x in w])) if w else (np.zeros(0, np.uint32), np.zeros(0))


def create(name, backend, tmp_path, **kw):
    k, L, weighting, scoring, seed, _ = M.ALL[name]
    v, after = orb_slam2_amd.ORBVocabulary.create(inputs(name), k, L, weighting, scoring, kw.get("seed", seed), return_features=True, library=backend)
    path = str(tmp_path / (name + ".txt"))
    v.saveToTextFile(path)
    return v, (np.concatenate(after) if len(after) else np.zeros((0, 32), np.uint8)), open(path, "rb").read(), path


@pytest.mark.parametrize("name", list(M.ALL))
def test_product_reproduces_reference(backend, golden, tmp_path, name):
    k, L, weighting, scoring, seed, _ = M.ALL[name]
    g = {key: golden[f"{name}/{key}"] for key in ("parent", "leaf", "desc", "weight", "ni", "after_rows", "after_vals", "params")}
    imgs = inputs(name)
    assert list(g["params"]) == [k, L, weighting, scoring, seed] and M.input_hash(imgs) == str(golden[f"{name}/input_hash"]), "the golden was made from another training set"
    v, after, text, _ = create(name, backend, tmp_path)
    want_after = np.concatenate(imgs).copy() if len(after) else after
    want_after[g["after_rows"]] = g["after_vals"]
    pk, pL, psc, pwt, parent, leaf, desc, printed = parse(text)
    mine = dict(parent=parent, leaf=leaf, desc=desc, ni=v.word_docs, after=after)
    why = M.explain(mine, dict(g, after=want_after))
    if why:                                                                   # say whether the golden or the product left the model
        m = M.train(imgs, k, L, weighting, scoring, seed)
        pytest.fail(f"product / golden: {why}; product / model: {M.explain(mine, m)}")
    assert (pk, pL, psc, pwt) == (k, L, scoring, weighting) == (v.k, v.L, v.scoring, v.weighting)
    assert (v.nnodes, v.nwords) == (len(parent), int(leaf.sum()))
    # the saved file, byte for byte
    assert hashlib.sha256(text).hexdigest() == str(golden[f"{name}/text_sha256"])
    if f"{name}/text" in golden:
        assert text == golden[f"{name}/text"].tobytes()
    # weights: full doubles through the per-feature transform of the features a word is made of; word ids are the leaves in node-id order
    ndocs = len(imgs)
    words = np.flatnonzero(leaf)
    word, weight = features_words(v, after)
    image = np.repeat(np.arange(ndocs), [len(f) for f in imgs])
    seen = np.zeros((max(len(words), 1), ndocs), bool)
    seen[word, image] = True
    assert np.array_equal(seen.sum(axis=1)[:len(words)], g["ni"])
    for w in np.unique(word):
        want = 1.0 if weighting in (1, 3) else math.log(ndocs / int(g["ni"][w]))
        assert np.all(weight[word == w] == want), (int(w), want)
        assert printed[words[w]] == float("%g" % want)
    unreached = words[g["ni"] == 0]
    assert np.all(printed[unreached] == (1.0 if weighting in (1, 3) else 0.0))
    assert np.all(printed[leaf == 0] == 0.0)


@pytest.mark.parametrize("name", ["k10_L3", "k3_L6"])
def test_created_and_reloaded_transform_alike(backend, tmp_path, name):
    """the file keeps six digits of a weight w: w' = w (1 + e), |e| <= 5e-6, and a normalised value w_i / sum(w) moves by at most (1 + 5e-6) / (1 - 5e-6) - 1 < 1.1e-5"""
    v, _, _, path = create(name, backend, tmp_path)
    again = orb_slam2_amd.ORBVocabulary(path, library=backend)
    assert (again.k, again.L, again.nnodes, again.nwords) == (v.k, v.L, v.nnodes, v.nwords)
    frame = M.make_set(999, [500], 300, 0.2)[0]
    a, b = v.transform(frame, 1), again.transform(frame, 1)
    for i in (0, 2, 3, 4):
        assert np.array_equal(a[i], b[i]), i
    assert len(a[0]) > 50 and np.allclose(a[1], b[1], rtol=1.1e-5, atol=0)
    resaved = str(tmp_path / "again.txt")
    again.saveToTextFile(resaved)                                             # a loaded vocabulary saves too, and to the same bytes
    assert open(resaved, "rb").read() == open(path, "rb").read()


def test_shapes_reach_their_situations(golden):
    """the counters the generator stored are the model's on today's training sets, and every case still reaches what it was made for"""
    assert tuple(golden["stat_keys"]) == M.STAT_KEYS and set(M.REACHES) <= set(M.SHAPES)
    for name, (k, L, weighting, scoring, seed, _) in M.SHAPES.items():
        stored = dict(zip(M.STAT_KEYS, (int(x) for x in golden[f"{name}/stats"])))
        assert M.train(inputs(name), k, L, weighting, scoring, seed)["stats"] == stored, name
        for key, need in M.REACHES.get(name, {}).items():
            assert stored[key] >= need, (name, key, stored[key], need)
    imgs = {name: [len(f) for f in inputs(name)] for name in ("root_2048", "root_2049", "one_image", "empty_runs")}
    assert sum(imgs["root_2048"]) == 2 * 1024 and sum(imgs["root_2049"]) == 2 * 1024 + 1 and len(imgs["one_image"]) == 1
    assert imgs["empty_runs"][:3] == [0, 0, 1] and imgs["empty_runs"][4:8] == [0, 0, 0, 1] and imgs["empty_runs"][-2:] == [0, 0]
    assert M.ALL["zero_cut_first"][4] >= 2**31 and M.ALL["zero_cut_later"][4] >= 2**31 and M.seed_of(M.ALL["root_key_zero"][4], 0, 300) == 0
    assert np.all(parse(golden["one_image/text"].tobytes())[7] == 0.0)         # one image: every printed weight is 0


@pytest.mark.parametrize("name", ["k3_L6", "wide_level"])
def test_created_vocabulary_against_oracle(backend, oracle, tmp_path, name):
    """the saved file of a created vocabulary (leaves above L, nodes of fewer than k children) loaded by the oracle: an unseen frame must get the same words,
    nodes and feature lists, and values within the six digits the file keeps (the bound of test_created_and_reloaded_transform_alike)"""
    L = M.ALL[name][1]
    v, _, _, path = create(name, backend, tmp_path)
    o = oracle.OracleVocabulary(path)
    assert (o.k, o.L, o.scoring, o.weighting, o.nnodes, o.nwords) == (v.k, v.L, v.scoring, v.weighting, v.nnodes, v.nwords)
    frame = M.make_set(999, [500], 300, 0.2)[0]
    for levelsup in (0, 1, L):
        a, b = v.transform(frame, levelsup), o.transform(frame, levelsup)
        for i in (0, 2, 3, 4):
            assert np.array_equal(a[i], b[i]), (levelsup, i)
        assert len(a[0]) > 50 and np.allclose(a[1], b[1], rtol=1.1e-5, atol=0), levelsup
    o.close()


def test_reference_written_file_round_trip(backend, tmp_path):
    """a file the reference's own saveToTextFile wrote, loaded and saved back: the same bytes"""
    v = orb_slam2_amd.ORBVocabulary(REF_VOC, library=backend)
    out = str(tmp_path / "back.txt")
    v.saveToTextFile(out)
    want = open(REF_VOC, "rb").read()
    assert len(want) > 10000 and open(out, "rb").read() == want


def test_three_threads(backend, golden, tmp_path):
    """three callers at once: a node of several chunks, a deep tree, a trivial one.  Each gets its own tree, and the level times of its own call (thread-local):
    one per level that ran k-means, none for root_5 (5 features, k = 10)"""
    names = ["big_few_values", "wide_level", "root_5"]
    levels = {n: int(golden[f"{n}/stats"][M.STAT_KEYS.index("kmeans_levels")]) for n in names[:2]}
    levels["root_5"] = 0
    assert sorted(levels.values()) == [0, 3, 7]
    L = orb_slam2_amd.lib(backend)
    out, errs = {}, []

    def work(name):
        try:
            for _ in range(2):
                v, _, text, _ = create(name, backend, tmp_path)
                out[name] = (hashlib.sha256(text).hexdigest(), len(v.level_ms), v.nnodes)
                v.close()
            L.orbhip_thread_release()
        except Exception as e:                                                # noqa: BLE001
            errs.append(e)

    for n in names:
        inputs(n)
    th = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for n in names:
        assert out[n] == (str(golden[f"{n}/text_sha256"]), levels[n], len(golden[f"{n}/parent"])), n


def test_seed_decides_the_tree(backend, tmp_path):
    _, after0, text0, _ = create("k3_L6", backend, tmp_path)
    _, after1, text1, _ = create("k3_L6", backend, tmp_path)
    other = M.CASES["k3_L6"][4] + 2                                           # (+ 1 empties a cluster at level 4: the model and the product both say so)
    _, after2, text2, _ = create("k3_L6", backend, tmp_path, seed=other)
    assert text0 == text1 and np.array_equal(after0, after1)
    assert text0 != text2
    m = M.train(inputs("k3_L6"), 3, 6, 0, 0, other)                           # a case made at test time: the other seed, against the model
    assert text2 == m["text"] and np.array_equal(after2, m["after"])


def _create_raw(L, desc, counts, k, depth, weighting=0, scoring=0, out=True):
    h = C.c_void_p()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    st = L.orbhip_voc_create(C.byref(h) if out else None, 0, p(desc), p(counts), 0 if counts is None else len(counts), k, depth, weighting, scoring, 0, None, None)
    assert (st == 0) == bool(h.value)
    if h.value:
        L.orbhip_voc_destroy(h)
    return st


def test_envelope(backend):
    L = orb_slam2_amd.lib(backend)
    desc = np.ascontiguousarray(np.concatenate(inputs("root_64"))); counts = np.array([len(f) for f in inputs("root_64")], np.int32)
    assert _create_raw(L, desc, counts, 10, 1) == 0
    assert _create_raw(L, desc, counts, 2, 10) == 0 and _create_raw(L, desc, counts, 32, 1) == 0
    for k, depth in ((1, 3), (33, 3), (0, 3), (10, 0), (10, 11)):
        assert _create_raw(L, desc, counts, k, depth) == UNSUPPORTED and L.orbhip_last_error() != b"", (k, depth)
    assert _create_raw(L, desc, counts, 10, 3, weighting=4) == INVALID and _create_raw(L, desc, counts, 10, 3, scoring=6) == INVALID
    bad = counts.copy(); bad[1] = -1
    assert _create_raw(L, desc, bad, 10, 3) == INVALID and b"image 1" in L.orbhip_last_error()
    assert _create_raw(L, None, counts, 10, 3) == INVALID and _create_raw(L, desc, counts, 10, 3, out=False) == INVALID
    assert L.orbhip_voc_save_text(None, b"/nonexistent") == INVALID
    assert _create_raw(L, desc, counts, 10, 1) == 0                           # and the library goes on working


def test_empty_cluster_is_refused(backend, golden, tmp_path):
    """tight blobs on which a cluster loses all its features: the reference dereferences a null pointer (the golden's generator saw it fault); here the call
    says which node and returns nothing"""
    d = golden["empty_cluster/desc"]; k, depth, weighting, scoring, seed = (int(x) for x in golden["empty_cluster/params"])
    with pytest.raises(M.EmptyCluster):
        M.train([d], k, depth, weighting, scoring, seed)
    with pytest.raises(orb_slam2_amd.OrbHipError, match="lost all its features") as e:
        orb_slam2_amd.ORBVocabulary.create([d], k, depth, weighting, scoring, seed, library=backend)
    assert e.value.status == UNSUPPORTED and "starts at feature 0 (%d features)" % len(d) in str(e.value)
    _, _, text, _ = create("root_65", backend, tmp_path)                      # the process goes on working
    assert hashlib.sha256(text).hexdigest() == str(golden["root_65/text_sha256"])


def test_model_rand_is_glibc():
    libc = C.CDLL(None)
    for s in (0, 1, 12345, 0x7fffffff):
        libc.srand(s)
        r = M.Rand(s)
        assert [libc.rand() for _ in range(400)] == [r() for _ in range(400)], s
