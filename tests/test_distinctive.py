"""orbhip_distinctive_descriptors (orb_slam2_amd.distinctive_descriptors) against MapPoint::ComputeDistinctiveDescriptors of ORB_SLAM2.

The chain is reference -> model -> product: tests/golden/distinct_ref.npz holds every point's mDescriptor before and after the reference's own member ran
(tests/golden/make_golden_distinct.py); tests/distinct_model.py is a literal restatement of MapPoint.cc:272-301 that must reproduce it; the product must
reproduce the golden, and the model at the sizes where the two kernels can go wrong.  Everything is compared exactly.

Sizes the sweep is built around (orb_slam2_amd/csrc/orbhip_distinct.hip): a group of up to DS_SMALL_MAX = 64 descriptors is one wavefront's (k_distinct_small,
DS_T / 64 = 4 groups per workgroup, the row handled eight columns at a time: 1, 2, 3, 63, 64), a larger one is one workgroup's (k_distinct_large: 65, 127, 128,
129), which stages the descriptors in LDS up to DL_STAGE_MAX = 1024 of them and reads them from device memory beyond (1023, 1024, 1025)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import orb_slam2_amd
import distinct_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "distinct_ref.npz")
DS_SMALL_MAX, GROUPS_PER_WORKGROUP, DL_STAGE_MAX = 64, 4, 1024


def near(rng, n, p=0.12):
    """n descriptors around one: distances small enough for medians to tie now and then"""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    return np.packbits(np.unpackbits(np.repeat(base[None], n, 0), axis=1) ^ (rng.random((n, 256)) < p), axis=1)


def pack(groups):
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    desc = np.concatenate([np.asarray(g, np.uint8).reshape(-1, 32) for g in groups]) if off[-1] else np.zeros((0, 32), np.uint8)
    return desc, off


def star(rng, n, w):
    """n - 1 descriptors that differ from a centre in w bits each, no bit twice, then the centre LAST: its median is w, every other row's 2w"""
    c = np.unpackbits(rng.integers(0, 256, 32, dtype=np.uint8))
    rows = []
    for j in range(n - 1):
        x = c.copy(); x[j * w:(j + 1) * w] ^= 1
        rows.append(np.packbits(x))
    return np.array(rows + [np.packbits(c)], np.uint8)


def make_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "sizes":
        return [near(rng, n) for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, DL_STAGE_MAX - 1, DL_STAGE_MAX, DL_STAGE_MAX + 1)]
    if name.startswith("alone_"):
        return [near(rng, int(name[6:]))]
    if name.startswith("workgroup_"):
        return [near(rng, int(rng.integers(1, 20))) for _ in range(int(name[10:]))]
    if name == "mixed_3000":
        sizes = np.where(rng.random(3000) < 0.7, rng.integers(2, 11, 3000), np.where(rng.random(3000) < 0.8, rng.integers(11, 41, 3000), rng.integers(41, 65, 3000)))
        sizes[rng.choice(3000, 150, replace=False)] = 0
        sizes[rng.choice(3000, 12, replace=False)] = rng.integers(65, 150, 12)
        sizes[0] = sizes[-1] = 0
        return [near(rng, int(n)) for n in sizes]
    if name == "all_ties":
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        return [np.repeat(d[None], 64, 0), np.repeat(d[None], 65, 0)]
    if name == "winner_last":
        return [star(rng, 40, 6), star(rng, 100, 2), star(rng, 64, 4), star(rng, 65, 3)]
    if name == "three_descriptors":
        three = rng.integers(0, 256, (3, 32), dtype=np.uint8)
        return [three[rng.integers(0, 3, int(n))] for n in rng.integers(1, 81, 200)]
    raise KeyError(name)


CASES = ["sizes", "alone_1", "alone_7", "alone_64", "alone_65", "workgroup_%d" % (GROUPS_PER_WORKGROUP - 1), "workgroup_%d" % GROUPS_PER_WORKGROUP,
         "workgroup_%d" % (GROUPS_PER_WORKGROUP + 1), "mixed_3000", "all_ties", "winner_last", "three_descriptors"]
_cache = {}


def case(name):
    """(desc, offsets, the model's index and median per group): computed once, shared by both backends, never changed"""
    if name not in _cache:
        desc, off = pack(make_case(name))
        bi, bm = M.best_all(desc, off)
        for a in (desc, off, bi, bm):
            a.setflags(write=False)
        _cache[name] = (desc, off, bi, bm)
    return _cache[name]


@pytest.fixture(scope="module")
def golden():
    g = M.load_golden(GOLDEN)
    return g, M.golden_groups(g)


# ------------------------------------------------------------------------------------------------ 1, 2: the golden
def test_model_reproduces_reference(golden):
    g, groups = golden
    assert np.array_equal(g["before"], g["initial"])
    touched = 0
    for p, (d, untouched) in enumerate(groups):
        want = g["before"][p] if untouched else d[M.best(d)[0]]
        assert np.array_equal(g["after"][p], want), p
        touched += not untouched
    assert touched >= 20 and touched < len(groups) - 2


def test_product_reproduces_reference(backend, golden):
    g, groups = golden
    desc, off = pack([d for d, _ in groups])
    bi, bm = orb_slam2_amd.distinctive_descriptors(desc, off, library=backend)
    for p, (d, untouched) in enumerate(groups):
        if len(d) == 0:
            assert bi[p] == -1, p
            continue
        assert 0 <= bi[p] < len(d), p
        if not untouched:                                                     # (a bad point's group is computed all the same: its answer is nobody's)
            assert np.array_equal(d[bi[p]], g["after"][p]), p
        mi, mm = M.best(d)
        assert bm[p] == mm, p
        if len(np.unique(d, axis=0)) == len(d):
            assert bi[p] == mi, p


# ------------------------------------------------------------------------------------------------ 3: product against model
@pytest.mark.parametrize("name", CASES)
def test_product_equals_model(backend, name):
    desc, off, mi, mm = case(name)
    bi, bm = orb_slam2_amd.distinctive_descriptors(desc, off, library=backend)
    bad = np.flatnonzero((bi != mi) | (bm != mm))
    assert len(bad) == 0, [(int(g), int(off[g + 1] - off[g]), int(bi[g]), int(mi[g]), int(bm[g]), int(mm[g])) for g in bad[:8]]
    n = np.diff(off)
    assert np.all(bi[n == 0] == -1)
    if name == "all_ties":
        assert list(bi) == [0, 0] and list(bm) == [0, 0]
    if name == "winner_last":
        assert list(bi) == [39, 99, 63, 64]
    if name == "mixed_3000":
        assert n[0] == 0 and n[-1] == 0 and (n == 0).sum() > 100 and (n > DS_SMALL_MAX).sum() >= 10
    if name == "three_descriptors":
        assert (n >= 4).mean() > 0.9                                          # four rows of three descriptors: two rows are equal, and so are their medians


# ------------------------------------------------------------------------------------------------ 4: the C ABI
def _call(L, desc, off, bi, bm, n=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return L.orbhip_distinctive_descriptors(0, p(desc), p(off), len(off) - 1 if n is None else n, p(bi), p(bm))


def test_abi_edges(backend):
    L = orb_slam2_amd.lib(backend)
    desc, off, mi, mm = case("workgroup_5")
    bi = np.full(5, 77, np.int32); bm = np.full(5, 77, np.int32)
    assert _call(L, desc, off, bi, bm, n=0) == 0 and np.all(bi == 77) and np.all(bm == 77)      # npoints = 0 touches nothing ...
    assert _call(L, None, None, None, None, n=0) == 0                                           # ... not even its pointers
    assert _call(L, desc, off, bi, None) == 0 and np.array_equal(bi, mi) and np.all(bm == 77)   # best_median may be NULL
    assert _call(L, desc, off, bi, bm) == 0 and np.array_equal(bm, mm)
    down = np.array(off); down[2] = down[3] + 1
    with pytest.raises(orb_slam2_amd.OrbHipError, match="offsets decrease at group 2"):
        orb_slam2_amd.distinctive_descriptors(desc, down, library=backend)
    start = np.array(off); start[0] = 1
    assert _call(L, desc, start, bi, bm) == 1 and b"offsets[0]" in L.orbhip_last_error()
    for args in ((None, off, bi, bm), (desc, None, bi, bm), (desc, off, None, bm)):
        assert _call(L, *args, n=5) == 1 and L.orbhip_last_error() != b""
    assert _call(L, desc, off, bi, bm, n=-1) == 1
    e0, e1 = orb_slam2_amd.distinctive_descriptors(np.zeros((0, 32), np.uint8), np.zeros(4, np.int32), library=backend)      # empty groups only, no descriptor at all
    assert list(e0) == [-1, -1, -1]


def test_arena_regrows_between_calls(backend):
    for name in ("alone_7", "sizes", "workgroup_4", "three_descriptors", "alone_1"):           # small, large, small ... on one thread
        desc, off, mi, mm = case(name)
        bi, bm = orb_slam2_amd.distinctive_descriptors(desc, off, library=backend)
        assert np.array_equal(bi, mi) and np.array_equal(bm, mm), name


def test_three_threads(backend):
    names = ["three_descriptors", "winner_last", "workgroup_5"]
    L = orb_slam2_amd.lib(backend)
    L.orbhip_thread_api_ms(1)
    out, errs = {}, []

    def work(name):
        try:
            desc, off, _, _ = case(name)
            for _ in range(3):
                out[name] = orb_slam2_amd.distinctive_descriptors(desc, off, library=backend)
            out[name + "_ms"] = L.orbhip_thread_api_ms(0)
            L.orbhip_thread_release()
        except Exception as e:                                                # noqa: BLE001
            errs.append(e)

    for n in names:
        case(n)
    th = [threading.Thread(target=work, args=(n,)) for n in names]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for n in names:
        assert np.array_equal(out[n][0], case(n)[2]) and np.array_equal(out[n][1], case(n)[3]), n
        assert out[n + "_ms"] > 0                                             # the entry counts into orbhip_thread_api_ms
