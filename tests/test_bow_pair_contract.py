"""What the four BoW matcher entry points of the C ABI promise about each other and about their arguments (include/orbhip.h):
orbhip_search_by_bow / orbhip_search_by_bow_batch and orbhip_search_for_triangulation / orbhip_search_for_triangulation_batch.

  test_invalid_arguments      negative counts, null outputs, a mode that does not exist, no pyramid levels, mode 1 without side 2's flags, a pair without a side,
                              no fundamental matrix: ORBHIP_ERR_INVALID
  test_nothing_to_match       an empty side or FeatureVector, the other array pointers null: ORBHIP_OK, nmatches 0, match12 (handed in full of garbage) all -1;
                              a batch of no pairs: ORBHIP_OK
  test_single_is_one_pair_*   a call and a batch of that one pair answer alike, exactly, where side 2's node is walked on registers (64), by ballots (257) and with
                              the upper `taken` mask (4097); both modes; triangulation in the canonical and in the fused arithmetic
  test_interleaved_*          batch of three, single, the batch, the single on one thread: every answer equals its first one (the thread's arena is reused)
  test_record_of_one_pair     emulation only: the ORBHIP_TEST_RECORD bytes of a triangulation call and of the batch of that one pair are the same"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_shapes as B  # noqa: E402
import orb_slam2_amd  # noqa: E402
from orb_slam2_amd import orbhip as H  # noqa: E402

F_X = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32) * np.float32(1.0 / 300)      # a translation along x
GARBAGE = 0x5a5a5a5
BOW_SIDE = ("desc", "angle", "valid", "n", "fv_node", "fv_off", "fv_feat", "nfv")
TRI_SIDE = ("desc", "kp", "has_mp", "stereo", "n", "fv_node", "fv_off", "fv_feat", "nfv")
TRI_LEVELS = ("scale_factors", "level_sigma2", "nlevels")


@functools.lru_cache(maxsize=None)
def _scene(len2, seed=0):
    """a node of len2 side-2 features among small ones, a node on one side only each way; flags of both matchers mixed.  Read-only: the tests share it."""
    rng = np.random.default_rng(4000 + len2 + seed)
    sc = B.Scene(rng, [(3, 20, 64), (7, 30, len2), (9, 4, 0), (11, 0, 6), (12, 66, 40)])
    sc.fill()
    for flags, p in ((sc.valid1, 0.9), (sc.valid2, 0.9), (sc.has1, 0.1), (sc.has2, 0.1), (sc.st1, 0.5), (sc.st2, 0.5)):
        flags[:] = rng.random(len(flags)) < p
    return sc


def _side(sc, s, tri):
    """one side's arguments by the names of orbhip_bow_side / orbhip_tri_side: contiguous arrays and counts"""
    d, k, fv = (sc.d1, sc.d2)[s], (sc.k1, sc.k2)[s], (sc.fv1, sc.fv2)[s]
    a = dict(desc=np.ascontiguousarray(d, np.uint8), n=len(d), fv_node=np.ascontiguousarray(fv[0], np.uint32), fv_off=np.ascontiguousarray(fv[1], np.int32),
             fv_feat=np.ascontiguousarray(fv[2], np.uint32), nfv=len(fv[0]))
    if tri:
        a.update(kp=np.ascontiguousarray(np.stack([k["x"], k["y"], k["angle"], k["octave"].astype(np.float32)], axis=1), np.float32),
                 has_mp=np.ascontiguousarray((sc.has1, sc.has2)[s], np.uint8), stereo=np.ascontiguousarray((sc.st1, sc.st2)[s], np.uint8),
                 scale_factors=np.ascontiguousarray(sc.scale, np.float32), level_sigma2=np.ascontiguousarray(sc.sigma2, np.float32), nlevels=len(sc.scale))
    else:
        a.update(angle=np.ascontiguousarray(k["angle"], np.float32), valid=np.ascontiguousarray((sc.valid1, sc.valid2)[s], np.uint8))
    return a


def _c(v):
    return H._p(v) if isinstance(v, np.ndarray) else v


def _addr(v):
    return H._p(v).value if isinstance(v, np.ndarray) else v


class Call:
    """The arguments of one pair, every one replaceable by name (`n1=-1`, `valid2=None`, `match12=None`, ...), for the single and the one-pair batch entry."""

    def __init__(self, sc, tri, mode=0, **over):
        self.tri, self.mode = tri, mode
        self.s = [_side(sc, 0, tri), _side(sc, 1, tri)]
        self.out = np.full(max(sc.n1, 4), GARBAGE, np.int32)
        self.a = dict(match12=self.out, nmatches=C.c_int(GARBAGE), F12=np.ascontiguousarray(F_X, np.float32).reshape(9), side1=True, side2=True, npairs=1)
        for key, v in over.items():
            if key[-1] in "12" and key[:-1] in self.s[0]:
                self.s[int(key[-1]) - 1][key[:-1]] = v
            else:
                assert key in self.a, key
                self.a[key] = v

    def single(self, L):
        s1, s2, a = self.s[0], self.s[1], self.a
        nm = None if a["nmatches"] is None else C.byref(a["nmatches"])
        if self.tri:
            return L.orbhip_search_for_triangulation(0, *[_c(s1[k]) for k in TRI_SIDE], *[_c(s2[k]) for k in TRI_SIDE], _c(a["F12"]), -5000.0, -5000.0,
                                                     *[_c(s2[k]) for k in TRI_LEVELS], 0, 1, _c(a["match12"]), nm)
        return L.orbhip_search_by_bow(0, self.mode, *[_c(s1[k]) for k in BOW_SIDE], *[_c(s2[k]) for k in BOW_SIDE], 0.75, 1, _c(a["match12"]), nm)

    def batch(self, L):
        """-> status; self.pair holds the pair afterwards"""
        s1, s2, a = self.s[0], self.s[1], self.a
        if self.tri:
            c1, c2 = (H.TriSide(*[_addr(s[k]) for k in TRI_SIDE + TRI_LEVELS]) for s in (s1, s2))
            self.pair = arr = (H.TriPair * 1)()
            if a["side2"]:
                arr[0].kf2 = C.pointer(c2)
            for i, v in enumerate(F_X.reshape(9)):
                arr[0].F12[i] = float(v)
            arr[0].ex = arr[0].ey = -5000.0
            arr[0].match12, arr[0].nmatches = _addr(a["match12"]), GARBAGE
            return L.orbhip_search_for_triangulation_batch(0, C.byref(c1) if a["side1"] else None, a["npairs"], arr, 0, 1)
        c1, c2 = (H.BowSide(*[_addr(s[k]) for k in BOW_SIDE]) for s in (s1, s2))
        self.pair = arr = (H.BowPair * 1)()
        if a["side1"]:
            arr[0].side1 = C.pointer(c1)
        if a["side2"]:
            arr[0].side2 = C.pointer(c2)
        arr[0].match12, arr[0].nmatches = _addr(a["match12"]), GARBAGE
        return L.orbhip_search_by_bow_batch(0, self.mode, a["npairs"], arr, C.c_float(0.75), 1)


# (arguments replaced, the matchers it applies to, the entry forms it applies to)
INVALID = {
    "n1<0": (dict(n1=-1), "bt", "sb"), "n2<0": (dict(n2=-1), "bt", "sb"), "nfv1<0": (dict(nfv1=-1), "bt", "sb"), "nfv2<0": (dict(nfv2=-1), "bt", "sb"),
    "null match12": (dict(match12=None), "bt", "sb"), "null nmatches": (dict(nmatches=None), "bt", "s"),
    "mode 2": (dict(mode=2), "b", "sb"), "nlevels2=0": (dict(nlevels2=0), "t", "sb"), "mode 1, null valid2": (dict(mode=1, valid2=None), "b", "sb"),
    "null side 1": (dict(side1=None), "bt", "b"), "null side 2": (dict(side2=None), "bt", "b"), "null F12": (dict(F12=None), "t", "s"),
    "npairs<0": (dict(npairs=-1), "bt", "b"),
}
CASES = [(name, m, f) for name, (_, ms, fs) in INVALID.items() for m in ms for f in fs]


@pytest.mark.parametrize("name,matcher,form", CASES, ids=[f"{n}-{m}-{f}" for n, m, f in CASES])
def test_invalid_arguments(backend, name, matcher, form):
    L = H.lib(backend)
    call = Call(_scene(64), matcher == "t", **INVALID[name][0])
    st = call.single(L) if form == "s" else call.batch(L)
    assert st == H.ERR_INVALID and L.orbhip_last_error()


# an empty side or FeatureVector: the arrays of BOTH sides may then be null
_NULL_BOW = {f"{k}{s}": None for s in "12" for k in BOW_SIDE if k not in ("n", "nfv")}
_NULL_TRI = {f"{k}{s}": None for s in "12" for k in TRI_SIDE + TRI_LEVELS[:2] if k not in ("n", "nfv")}


@pytest.mark.parametrize("form", ["single", "batch"])
@pytest.mark.parametrize("matcher", ["bow0", "bow1", "tri"])
@pytest.mark.parametrize("empty", ["n1", "n2", "nfv1", "nfv2"])
def test_nothing_to_match(backend, empty, matcher, form):
    L = H.lib(backend)
    tri = matcher == "tri"
    call = Call(_scene(64), tri, mode=int(matcher == "bow1"), **{**(_NULL_TRI if tri else _NULL_BOW), empty: 0})
    n1 = call.s[0]["n"]
    if form == "single":
        assert call.single(L) == H.OK and call.a["nmatches"].value == 0
    else:
        assert call.batch(L) == H.OK and call.pair[0].nmatches == 0
    assert np.all(call.out[:n1] == -1) and np.all(call.out[n1:] == GARBAGE)


@pytest.mark.parametrize("matcher", ["bow", "tri"])
def test_batch_of_no_pairs(backend, matcher):
    L = H.lib(backend)
    call = Call(_scene(64), matcher == "tri", npairs=0)
    assert call.batch(L) == H.OK and np.all(call.out == GARBAGE)


def _bow_dict(sc, s):
    return dict(desc=(sc.d1, sc.d2)[s], angle=(sc.k1, sc.k2)[s]["angle"], valid=(sc.valid1, sc.valid2)[s], fv=(sc.fv1, sc.fv2)[s])


def _tri_dict(sc, s):
    return dict(desc=(sc.d1, sc.d2)[s], kps=(sc.k1, sc.k2)[s], has_mp=(sc.has1, sc.has2)[s], stereo=(sc.st1, sc.st2)[s], fv=(sc.fv1, sc.fv2)[s], scale_factors=sc.scale, level_sigma2=sc.sigma2)


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("len2", [64, 257, 4097])
def test_single_is_one_pair_search_by_bow(backend, len2, mode, check_ori):
    sc = _scene(len2)
    one = orb_slam2_amd.search_by_bow(mode, *sc.bow_args(mode), nnratio=0.75, check_ori=check_ori, library=backend)
    s2 = _bow_dict(sc, 1)
    if mode == 0:
        s2["valid"] = None                                       # what the single call above hands in
    (pair,) = H.search_by_bow_batch(mode, [(_bow_dict(sc, 0), s2)], nnratio=0.75, check_ori=check_ori, library=backend)
    assert one[0] > 20 and _same(one, pair), (one[0], pair[0], np.nonzero(one[1] != pair[1])[0][:10])


@pytest.mark.parametrize("only_stereo", [False, True])
@pytest.mark.parametrize("fp_contract", [0, 1])
@pytest.mark.parametrize("len2", [64, 257, 4097])
def test_single_is_one_pair_triangulation(backend, len2, fp_contract, only_stereo):
    sc = _scene(len2)
    ex, ey = float(sc.k2["x"][0]) + 1.5, float(sc.k2["y"][0])
    one = orb_slam2_amd.search_for_triangulation(*sc.tri_args(F_X, ex, ey), only_stereo=only_stereo, check_ori=True, library=backend, fp_contract=fp_contract)
    (pair,) = H.search_for_triangulation_batch(_tri_dict(sc, 0), [dict(kf=_tri_dict(sc, 1), F12=F_X, ex=ex, ey=ey)], only_stereo=only_stereo, check_ori=True, library=backend,
                                               fp_contract=fp_contract)
    assert one[0] > 5 and _same(one, pair), (one[0], pair[0], np.nonzero(one[1] != pair[1])[0][:10])


def test_interleaved_search_by_bow(backend):
    a, b, c = _scene(64), _scene(257), _scene(64, seed=1)
    a1, a2, b1, b2 = _bow_dict(a, 0), _bow_dict(a, 1), _bow_dict(b, 0), _bow_dict(b, 1)
    batch = lambda: H.search_by_bow_batch(1, [(a1, a2), (b1, b2), (a1, a2)], nnratio=0.75, library=backend)      # a1 and a2 named twice: uploaded once
    single = lambda: orb_slam2_amd.search_by_bow(1, *c.bow_args(1), nnratio=0.75, library=backend)
    first = (batch(), single())
    again = (batch(), single())
    assert all(n > 0 for n, _ in first[0]) and first[1][0] > 0
    assert all(_same(x, y) for x, y in zip(first[0], again[0])) and _same(first[1], again[1])
    for sc, got in ((a, first[0][0]), (b, first[0][1]), (c, first[1])):      # ... and the first answers are the calls' own
        assert _same(got, orb_slam2_amd.search_by_bow(1, *sc.bow_args(1), nnratio=0.75, library=backend))


def test_interleaved_triangulation(backend):
    a, b, c = _scene(64), _scene(257), _scene(64, seed=1)
    k1 = _tri_dict(a, 0)
    nbs = [dict(kf=_tri_dict(a, 1), F12=F_X, ex=-5000.0, ey=-5000.0), dict(kf=_tri_dict(c, 1), F12=F_X, ex=300.0, ey=200.0), dict(kf=_tri_dict(a, 1), F12=F_X, ex=300.0, ey=200.0)]
    batch = lambda: H.search_for_triangulation_batch(k1, nbs, check_ori=True, library=backend)
    single = lambda: orb_slam2_amd.search_for_triangulation(*b.tri_args(F_X, -5000.0, -5000.0), check_ori=True, library=backend)
    first = (batch(), single())
    again = (batch(), single())
    assert first[0][0][0] > 0 and first[0][2][0] > 0 and first[1][0] > 0
    assert all(_same(x, y) for x, y in zip(first[0], again[0])) and _same(first[1], again[1])
    assert _same(first[0][0], orb_slam2_amd.search_for_triangulation(*a.tri_args(F_X, -5000.0, -5000.0), check_ori=True, library=backend))


@pytest.mark.parametrize("fp_contract", [0, 1])
def test_record_of_one_pair(emu_lib, tmp_path, monkeypatch, fp_contract):
    sc = _scene(257)
    rec = [tmp_path / "single.bin", tmp_path / "batch.bin"]
    monkeypatch.setenv("ORBHIP_TEST_RECORD", str(rec[0]))
    one = orb_slam2_amd.search_for_triangulation(*sc.tri_args(F_X, 300.0, 200.0), check_ori=True, library=emu_lib, fp_contract=fp_contract)
    monkeypatch.setenv("ORBHIP_TEST_RECORD", str(rec[1]))
    (pair,) = H.search_for_triangulation_batch(_tri_dict(sc, 0), [dict(kf=_tri_dict(sc, 1), F12=F_X, ex=300.0, ey=200.0)], check_ori=True, library=emu_lib, fp_contract=fp_contract)
    monkeypatch.delenv("ORBHIP_TEST_RECORD")
    got = [r.read_bytes() for r in rec]
    assert _same(one, pair) and got[0][:4] == np.int32(3).tobytes() and len(got[0]) > sc.n1 * 32 + sc.n2 * 32 and got[0] == got[1]
