"""A plain restatement of DBoW2's TemplatedVocabulary::create (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:558-616, :642-996) with FORB (FORB.cpp:28-101), walked
level by level, and the seeded training sets the vocabulary-training tests share.

tests/golden/make_golden_voc_train.py checks the model against the reference's own code (tests/voc_train_harness.py) before it writes a golden; the tests use
it to say WHERE a product tree leaves the reference's, and for cases made at test time.  What the restatement has to get right:
  - every node that runs k-means reseeds glibc's rand() (Rand below) from seed_of(base, first feature, feature count);
  - centres alias training features: a mean of >= 2 features is written INTO the feature that seeded the cluster, a group of exactly one replaces the centre
    by a copy (the alias ends), and a node's descriptor is what its feature holds when everything is over;
  - inside a node the means are computed cluster after cluster, each seeing the features as the previous ones left them (which, as _kmeans asserts, never
    shows: an aliased feature sits in its own cluster or an earlier one);
  - weights come from walking the MODIFIED features down the finished tree; a word no walk reaches keeps weight 0.
"""
import hashlib
import math

import numpy as np

POP = np.array([bin(i).count("1") for i in range(256)], np.int64)
MAX_PASSES = 512                       # the product's bound on the Lloyd passes of a level
CHUNK = 1024                           # the product's VT_CHUNK: a node of more features is cut into several chunks and takes the device-memory counter path


# train()'s counters.  Per k-means node: early_stop (k-means++ ran out of distance before k centres), singleton (a cluster of exactly one feature ends its
# centre's alias), one_centre (the node keeps a single centre), each also counted as big_* when the node has more than CHUNK features; zero_cut (a cut of 0.0
# drawn again, TemplatedVocabulary.h:887-891); key_zero (the node's srand key is 0).  Per call: alias_write, passes (the most Lloyd passes of a node),
# leaf_above_L, zero_docs (words no walk reaches), empty_images, empty_run (the longest run of consecutive empty images), max_level_nodes (the most k-means
# nodes on one level), kmeans_levels (levels with at least one k-means node: what orbhip_voc_create_level_ms counts), settles_past_512 (levels on which a
# k-means node past the first 512 takes more Lloyd passes than every one of the first 512: the level's passes end with a node of the third workgroup).
STAT_KEYS = ("early_stop", "singleton", "alias_write", "passes", "leaf_above_L", "zero_docs", "empty_images", "big_early_stop", "big_singleton", "one_centre",
             "big_one_centre", "zero_cut", "key_zero", "max_level_nodes", "empty_run", "kmeans_levels", "settles_past_512")


class EmptyCluster(Exception):
    """a cluster lost all its features: the reference releases the centre and reads through a null pointer at the next distance"""


class Rand:
    """glibc's srand / rand: TYPE_3 additive feedback, r[i] = r[i-31] + r[i-3] over 31 words of the 16807 Lehmer sequence, 310 values discarded, 31 bits out"""

    def __init__(self, seed):
        w = seed if seed else 1
        r = [w]
        for _ in range(30):
            hi, lo = divmod(w, 127773)
            w = 16807 * lo - 2836 * hi
            if w < 0:
                w += 2147483647
            r.append(w)
        r += r[0:3]
        for i in range(34, 344):
            r.append((r[i - 31] + r[i - 3]) & 0xffffffff)
        self.r = r

    def __call__(self):
        r = self.r
        r.append((r[-31] + r[-3]) & 0xffffffff)
        return r[-1] >> 1


def seed_of(base, first, n):
    return (base ^ (first * 0x9E3779B1) ^ (n * 0x85EBCA6B)) & 0x7fffffff


def ham(a, b):
    """distances of the rows of a (n x 32) to b (32)"""
    return POP[a ^ b].sum(axis=1)


def mean_value(rows):
    n = len(rows)
    return np.packbits(np.unpackbits(rows, axis=1).sum(axis=0) >= n // 2 + n % 2)


def _kmeans(feats, idx, k, base, stats):
    """HKmeansStep's k-means on the node whose features are idx (:671-783) -> (centres: feature slot or -1, own buffers, association, Lloyd passes)"""
    n = len(idx)
    big = n > CHUNK
    key = seed_of(base, int(idx[0]), n)
    stats["key_zero"] += key == 0
    rng = Rand(key)
    slots = [int(idx[int((rng() / 2147483648.0) * n)])]
    d = feats[idx]
    mind = ham(d, feats[slots[0]])
    while len(slots) < k:
        nd = ham(d, feats[slots[-1]])
        m = (mind > 0) & (nd < mind)
        mind[m] = nd[m]
        s = int(mind.sum())
        if s == 0:
            stats["early_stop"] += 1; stats["big_early_stop"] += big
            break
        while True:
            cut = (rng() / 2147483647.0) * s
            if cut != 0.0:
                break
            stats["zero_cut"] += 1
        j = int(np.searchsorted(np.cumsum(mind), cut, side="left"))
        slots.append(int(idx[min(j, n - 1)]))
    nc = len(slots)
    stats["one_centre"] += nc == 1; stats["big_one_centre"] += big and nc == 1
    own = [None] * nc
    assoc = last = None
    for npass in range(MAX_PASSES + 1):
        if assoc is not None:
            for c in range(nc):
                members = idx[assoc == c]
                if len(members) == 0:
                    raise EmptyCluster(f"node of {n} features from feature {int(idx[0])}: cluster {c} is empty in pass {npass}")
                if len(members) == 1:
                    if slots[c] >= 0:
                        stats["singleton"] += 1; stats["big_singleton"] += big
                    own[c] = feats[members[0]].copy(); slots[c] = -1
                else:
                    mean = mean_value(feats[members])
                    if slots[c] >= 0:
                        # the feature holds centre c's own bytes, so it was assigned to the first centre at distance 0: c or an earlier one,
                        # whose mean is already taken.  No later cluster of this pass reads what is written here.
                        assert assoc[np.flatnonzero(idx == slots[c])[0]] <= c
                        stats["alias_write"] += 1
                        feats[slots[c]] = mean
                    else:
                        own[c] = mean
        cur = feats[idx]
        dist = np.stack([ham(cur, feats[slots[c]] if slots[c] >= 0 else own[c]) for c in range(nc)])
        last, assoc = assoc, np.argmin(dist, axis=0)                          # the first of equal minima
        if last is not None and np.array_equal(last, assoc):
            stats["passes"] = max(stats["passes"], npass)
            return slots, own, assoc, npass
    raise RuntimeError("k-means did not settle")


def train(images, k, L, weighting=0, scoring=0, seed=0):
    """images: one (n_i x 32) uint8 array per image -> dict(parent, leaf, desc, weight, ni, after, text, stats); node ids are the reference's"""
    counts = [len(f) for f in images]
    feats = np.concatenate([np.asarray(f, np.uint8).reshape(-1, 32) for f in images]).copy() if sum(counts) else np.zeros((0, 32), np.uint8)
    M = len(feats)
    stats = dict.fromkeys(STAT_KEYS, 0)
    stats["empty_images"] = sum(c == 0 for c in counts)
    stats["empty_run"] = max((len(r) for r in "".join("e" if c == 0 else " " for c in counts).split()), default=0)
    hparent, hslot, hown, hkids, hlevel = [0], [-1], [None], [[]], [0]

    def add(p, slot, own, level):
        hparent.append(p); hslot.append(slot); hown.append(own); hkids.append([]); hlevel.append(level)
        hkids[p].append(len(hparent) - 1)
        return len(hparent) - 1

    work = [(0, np.arange(M))] if M else []
    for level in range(1, L + 1):
        nxt = []
        width = sum(len(idx) > k for _, idx in work)
        stats["max_level_nodes"] = max(stats["max_level_nodes"], width); stats["kmeans_levels"] += width > 0
        passes = []                                                           # of this level's k-means nodes, in the product's node order
        for h, idx in work:
            if len(idx) <= k:                                                 # :660-670
                for f in idx:
                    add(h, int(f), None, level)
                continue
            slots, own, assoc, npass = _kmeans(feats, idx, k, seed, stats)
            passes.append(npass)
            for c in range(len(slots)):
                child = add(h, slots[c], own[c], level)
                g = idx[assoc == c]
                if len(g) > 1 and level < L:
                    nxt.append((child, g))
        stats["settles_past_512"] += len(passes) > 512 and max(passes[512:]) > max(passes[:512])
        work = nxt
    # ids: a node's children take the next ids when it is visited, then the children are visited in order (:786-817)
    nn = len(hparent)
    ident = [0] * nn
    nxt_id = [1]

    def visit(h):
        stack = [h]
        while stack:
            x = stack.pop()
            for c in hkids[x]:
                ident[c] = nxt_id[0]; nxt_id[0] += 1
            stack.extend(c for c in reversed(hkids[x]) if hkids[c])
    visit(0)
    parent = np.zeros(nn, np.int32); leaf = np.zeros(nn, np.uint8); desc = np.zeros((nn, 32), np.uint8)
    kids = [[] for _ in range(nn)]
    for h in range(1, nn):
        i = ident[h]
        parent[i] = ident[hparent[h]]; leaf[i] = not hkids[h]
        desc[i] = feats[hslot[h]] if hslot[h] >= 0 else hown[h]
        stats["leaf_above_L"] += int(not hkids[h] and hlevel[h] < L)
    for i in range(1, nn):
        kids[parent[i]].append(i)
    words = np.flatnonzero(leaf[1:]) + 1
    word_of = {int(n): w for w, n in enumerate(words)}
    # setNodeWeights (:943-996): the walk of every (modified) feature
    image = np.repeat(np.arange(len(counts)), counts)
    docs = [set() for _ in words]
    walk = [(0, np.arange(M))] if len(words) and M else []
    while walk:
        node, fi = walk.pop()
        if not kids[node]:
            docs[word_of[node]].update(image[fi].tolist())
            continue
        best = np.argmin(np.stack([ham(feats[fi], desc[c]) for c in kids[node]]), axis=0)
        for j, c in enumerate(kids[node]):
            if np.any(best == j):
                walk.append((c, fi[best == j]))
    ni = np.array([len(s) for s in docs], np.int32)
    weight = np.zeros(nn, np.float64)
    for w, n in enumerate(words):
        if weighting in (1, 3):
            weight[n] = 1.0
        elif ni[w] > 0:
            weight[n] = math.log(len(counts) / int(ni[w]))
    stats["zero_docs"] = int((ni == 0).sum())
    return dict(parent=parent, leaf=leaf, desc=desc, weight=weight, ni=ni, after=feats, text=text_of(k, L, scoring, weighting, parent, leaf, desc, weight), stats=stats)


def text_of(k, L, scoring, weighting, parent, leaf, desc, weight):
    """saveToTextFile (:1429-1449)"""
    lines = ["%d %d  %d %d\n" % (k, L, scoring, weighting)]
    for i in range(1, len(parent)):
        lines.append("%d %d %s  %s\n" % (parent[i], 1 if leaf[i] else 0, " ".join(str(int(b)) for b in desc[i]), "%g" % weight[i]))
    return "".join(lines).encode()


def explain(a, b):
    """the first place where two trees (dicts like train's) part"""
    for key in ("parent", "leaf", "desc", "ni", "after"):
        x, y = np.asarray(a[key]), np.asarray(b[key])
        if x.shape != y.shape:
            return f"{key}: shapes {x.shape} and {y.shape}"
        if not np.array_equal(x, y):
            bad = np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))
            return f"{key}: {len(bad)} rows differ, first at {int(bad[0])}: {x[bad[0]]} / {y[bad[0]]}"
    return None


# ------------------------------------------------------------------------------------------------ training sets
def make_set(seed, counts, nproto=0, flip=0.2):
    """one array per image: independent random bits (nproto = 0), or `nproto` random prototypes with every bit flipped with probability `flip`"""
    rng = np.random.default_rng(seed)
    total = int(sum(counts))
    if nproto:
        protos = rng.integers(0, 256, (nproto, 32), dtype=np.uint8)
        bits = np.unpackbits(protos[rng.integers(0, nproto, total)], axis=1) ^ (rng.random((total, 256)) < flip)
        desc = np.packbits(bits, axis=1)
    else:
        desc = rng.integers(0, 256, (total, 32), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(counts)])
    return [desc[off[i]:off[i + 1]] for i in range(len(counts))]


def few_values(seed, counts, nvalues):
    """features that take only `nvalues` distinct values: k-means++ runs out of distance before it has k centres"""
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 256, (nvalues, 32), dtype=np.uint8)
    total = int(sum(counts))
    desc = vals[rng.integers(0, nvalues, total)]
    off = np.concatenate([[0], np.cumsum(counts)])
    return [desc[off[i]:off[i + 1]] for i in range(len(counts))]


def counted_values(seed, counts_per_value, image_counts):
    """one random value per entry of `counts_per_value`, each taken by exactly that many features, in shuffled order"""
    rng = np.random.default_rng(seed)
    vals = rng.integers(0, 256, (len(counts_per_value), 32), dtype=np.uint8)
    assert len(np.unique(vals, axis=0)) == len(vals) and sum(counts_per_value) == sum(image_counts)
    desc = vals[rng.permutation(np.repeat(np.arange(len(vals)), counts_per_value))]
    off = np.concatenate([[0], np.cumsum(image_counts)])
    return [desc[off[i]:off[i + 1]] for i in range(len(image_counts))]


def split(total, nimages, seed, empty=()):
    """`total` features over `nimages` images, those listed in `empty` without any"""
    rng = np.random.default_rng(seed)
    full = [i for i in range(nimages) if i not in empty]
    cuts = np.sort(rng.integers(0, total + 1, len(full) - 1))
    sizes = np.diff(np.concatenate([[0], cuts, [total]]))
    counts = [0] * nimages
    for i, s in zip(full, sizes):
        counts[i] = int(s)
    return counts


ROOT_SIZES = (5, 10, 11, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)      # the root of k = 10, L = 1 is one node of exactly M features

# name -> (k, L, weighting, scoring, seed, training set)
CASES = {
    "k10_L3": (10, 3, 0, 0, 11, lambda: make_set(101, split(10000, 40, 1), 300, 0.2)),
    "k3_L6": (3, 6, 0, 0, 12, lambda: make_set(102, split(900, 12, 2), 40, 0.18)),
    "k5_L5": (5, 5, 0, 0, 13, lambda: make_set(103, split(3400, 20, 3))),
    "k8_L2_empty_images": (8, 2, 0, 0, 14, lambda: make_set(104, split(200, 10, 4, empty=(0, 4, 9)), 12, 0.15)),
    "k2_L8": (2, 8, 0, 0, 15, lambda: make_set(105, split(260, 6, 5), 20, 0.2)),
    "k32_L2": (32, 2, 0, 0, 16, lambda: make_set(106, split(3400, 16, 6), 200, 0.25)),
    "three_values": (5, 3, 0, 0, 17, lambda: few_values(107, split(90, 5, 7), 3)),
    "no_features": (10, 3, 0, 0, 18, lambda: [np.zeros((0, 32), np.uint8)] * 3),
    "weighting_tf": (8, 2, 1, 0, 14, lambda: make_set(104, split(200, 10, 4, empty=(0, 4, 9)), 12, 0.15)),
    "weighting_idf": (8, 2, 2, 1, 14, lambda: make_set(104, split(200, 10, 4, empty=(0, 4, 9)), 12, 0.15)),
    "weighting_binary": (8, 2, 3, 5, 14, lambda: make_set(104, split(200, 10, 4, empty=(0, 4, 9)), 12, 0.15)),
}
for _m in ROOT_SIZES:
    CASES["root_%d" % _m] = (10, 1, 0, 0, 20 + _m, (lambda m: lambda: make_set(200 + m, split(m, 3, m)))(_m))


# Node shapes and draws the cases above do not reach (tests/golden/voc_train_shapes_ref.npz).  The root of a set of n features starts at feature 0, so its
# srand key is (base ^ n * 0x85EBCA6B) & 0x7fffffff: root_key(n, s) is the base seed that makes it s.  srand(1866778841) returns 0 at draw 1 and
# srand(1974820829) at draw 3 (draw 0 picks the first centre); both bases come out above 2^31.
def root_key(n, s):
    return (s ^ (n * 0x85EBCA6B)) & 0xffffffff


SHAPES = {
    "big_few_values": (5, 3, 0, 0, 31, lambda: counted_values(301, (1300, 700, 1), split(2001, 6, 31))),
    "zero_cut_first": (10, 1, 0, 0, root_key(300, 1866778841), lambda: make_set(303, split(300, 4, 33), 25, 0.2)),
    "zero_cut_later": (10, 1, 0, 0, root_key(300, 1974820829), lambda: make_set(303, split(300, 4, 33), 25, 0.2)),
    "root_key_zero": (10, 2, 0, 0, root_key(300, 0), lambda: make_set(304, split(300, 4, 34), 25, 0.2)),
    "wide_level": (3, 7, 0, 0, 47, lambda: make_set(302, split(6000, 9, 32))),
    "one_image": (6, 3, 0, 0, 35, lambda: make_set(305, [400], 30, 0.2)),
    "empty_runs": (6, 2, 0, 0, 36, lambda: make_set(306, [0, 0, 1, 150, 0, 0, 0, 1, 148, 0, 0], 12, 0.15)),
}
for _m in (2048, 2049):
    SHAPES["root_%d" % _m] = (10, 1, 0, 0, 20 + _m, (lambda m: lambda: make_set(200 + m, split(m, 3, m)))(_m))
# what each case was made for: the least its counter must say (train()["stats"], stored beside the golden)
REACHES = {
    "big_few_values": dict(big_early_stop=3, big_singleton=1, big_one_centre=2, one_centre=4),
    "zero_cut_first": dict(zero_cut=1),
    "zero_cut_later": dict(zero_cut=1),
    "root_key_zero": dict(key_zero=1),
    "wide_level": dict(max_level_nodes=513, settles_past_512=1),
    "empty_runs": dict(empty_run=3, empty_images=7),
}
ALL = dict(CASES, **SHAPES)


def case_images(name):
    return ALL[name][5]()


def input_hash(images):
    h = hashlib.sha256()
    h.update(np.array([len(f) for f in images], np.int64).tobytes())
    for f in images:
        h.update(np.ascontiguousarray(f, np.uint8).tobytes())
    return h.hexdigest()
