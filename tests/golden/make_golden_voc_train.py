"""Writes tests/golden/voc_train_ref.npz (voc_train_model.CASES) and tests/golden/voc_train_shapes_ref.npz (voc_train_model.SHAPES, with the model's counters
per case as name/stats, in the order of stat_keys): what the reference's own TemplatedVocabulary::create (tests/voc_train_harness.py: its k-means++ stream reseeded per
node) makes of the seeded training sets of tests/voc_train_model.py.  Data only: per case the tree (parents, leaf flags, node descriptors,
full-double weights), Ni per word, the training features create() overwrote (rows and new values), the saved text file (its SHA-256, and the file itself
where it is small), and a hash of the inputs - the inputs themselves come from the seeded generator again.

    python tests/golden/make_golden_voc_train.py /path/to/ORB_SLAM2

Nothing is written when the reference faults on a case, when the model (tests/voc_train_model.py) disagrees with the reference anywhere, or when one of the
situations the tests rely on does not occur in the set."""
import hashlib
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voc_train_harness as H      # noqa: E402
import voc_train_model as M        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "voc_train_ref.npz")
OUT_SHAPES = os.path.join(ROOT, "tests", "golden", "voc_train_shapes_ref.npz")
TEXT_MAX = 40000                      # saved files up to this many bytes are kept whole
# the least the shapes cases (voc_train_model.SHAPES) must reach somewhere, beside what every one of them was made for (voc_train_model.REACHES):
# 513 k-means nodes on a level are three workgroups of 256 (and on one such level a node of the third must be the last to settle), a run of 3 empty images is longer than one step of k_vt_docs' bisection
SHAPES_NEED = dict(big_early_stop=1, big_singleton=1, big_one_centre=1, zero_cut=1, key_zero=1, max_level_nodes=513, settles_past_512=1, empty_run=3)


def blobs(seed, n, nb, flip):
    rng = np.random.default_rng(seed)
    protos = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    return np.packbits(np.unpackbits(protos[rng.integers(0, nb, n)], axis=1) ^ (rng.random((n, 256)) < flip), axis=1)


def find_empty_cluster(budget=2.0):
    """a small set of tight blobs on which a cluster loses all its features (model), within `budget` seconds"""
    t0 = time.time()
    seed = 0
    while time.time() - t0 < budget:
        rng = np.random.default_rng(seed + 10**6)
        n, k, nb, flip = int(rng.integers(8, 40)), int(rng.integers(3, 7)), int(rng.integers(2, 4)), float(rng.choice([0.004, 0.01, 0.02]))
        d = blobs(seed, n, nb, flip)
        try:
            M.train([d], k, 1, 0, 0, seed)
        except M.EmptyCluster as e:
            return d, k, seed, str(e)
        seed += 1
    return None


def run_cases(lib, tmp, cases, with_stats):
    """the reference and the model on every case -> (the golden's arrays, the model's counters per case); exits when they disagree"""
    out, stats = {}, {}
    for name, (k, L, weighting, scoring, seed, make) in cases.items():
        images = make()
        r = H.train_isolated(lib, images, k, L, weighting, scoring, seed, text_path=os.path.join(tmp, "voc.txt"))
        if r is None:
            sys.exit(f"{name}: the reference faulted; nothing written")
        m = M.train(images, k, L, weighting, scoring, seed)
        why = M.explain(r, m)
        if why or r["text"] != m["text"] or not np.array_equal(r["weight"], m["weight"]):
            sys.exit(f"{name}: the model leaves the reference ({why or 'weights / saved file'}); nothing written")
        stats[name] = m["stats"]
        before = np.concatenate(images) if len(r["after"]) else r["after"]
        rows = np.flatnonzero((before != r["after"]).any(axis=1)).astype(np.int32)
        for key in ("parent", "leaf", "desc", "weight", "ni"):
            out[f"{name}/{key}"] = r[key]
        out[f"{name}/after_rows"] = rows; out[f"{name}/after_vals"] = r["after"][rows]
        out[f"{name}/params"] = np.array([k, L, weighting, scoring, seed], np.int64)
        out[f"{name}/input_hash"] = np.array(M.input_hash(images)); out[f"{name}/text_sha256"] = np.array(hashlib.sha256(r["text"]).hexdigest())
        if len(r["text"]) <= TEXT_MAX:
            out[f"{name}/text"] = np.frombuffer(r["text"], np.uint8)
        if with_stats:
            out[f"{name}/stats"] = np.array([m["stats"][key] for key in M.STAT_KEYS], np.int64)
        print(f"{name}: {len(r['parent'])} nodes, {len(r['ni'])} words, {len(rows)} features overwritten, reference {r['seconds']:.3f} s; model agrees")
    return out, stats


def main(reference):
    tmp = tempfile.mkdtemp(prefix="voc_train_ref_")
    lib = H.build(tmp, reference)
    out, stats = run_cases(lib, tmp, M.CASES, False)
    seen = {key: sum(s[key] for s in stats.values()) for key in ("early_stop", "singleton", "alias_write", "leaf_above_L", "zero_docs", "empty_images")}
    missing = [k for k, v in seen.items() if v == 0]
    if missing:
        sys.exit(f"situations that never occur in the set: {missing}; nothing written")
    shapes, sstats = run_cases(lib, tmp, M.SHAPES, True)
    shapes["stat_keys"] = np.array(M.STAT_KEYS)
    sseen = {key: max(s[key] for s in sstats.values()) for key in SHAPES_NEED}
    missing = [f"{key} {sseen[key]} < {need}" for key, need in SHAPES_NEED.items() if sseen[key] < need]
    missing += [f"{name}: {key} {sstats[name][key]} < {need}" for name, needs in M.REACHES.items() for key, need in needs.items() if sstats[name][key] < need]
    if missing:
        sys.exit(f"situations that never occur in the set: {missing}; nothing written")
    found = find_empty_cluster()
    if found:
        d, k, seed, what = found
        if H.train_isolated(lib, [d], k, 1, 0, 0, seed) is not None:
            sys.exit("empty-cluster set: the model sees an empty cluster, the reference survives; nothing written")
        out["empty_cluster/desc"] = d; out["empty_cluster/params"] = np.array([k, 1, 0, 0, seed], np.int64)
        print(f"empty cluster: {what}; the reference faults on it")
    else:
        print("no empty-cluster set found within the budget: the golden goes without one")
    np.savez_compressed(OUT, **out)
    print(f"situations: {seen}\nwrote {OUT}: {os.path.getsize(OUT)} bytes; the model reproduces the reference on all {len(M.CASES)} cases")
    np.savez_compressed(OUT_SHAPES, **shapes)
    print(f"situations: {sseen}\nwrote {OUT_SHAPES}: {os.path.getsize(OUT_SHAPES)} bytes; the model reproduces the reference on all {len(M.SHAPES)} cases")


if __name__ == "__main__":
    main(sys.argv[1])
