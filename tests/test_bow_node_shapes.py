"""k_bow_match / k_bow_triangulate (orbhip_bow.hip) at node shapes, ties and lane positions that frames through a vocabulary never produce.

A wavefront per vocabulary node: up to 256 side-2 features it walks on registers (four chunks, DPP wave minimum), above that the general walk (ballots over
chunks of 64, "taken" flags in two 64-bit masks split at chunk 64), above 8192 SearchByBoW refuses; side 2's node is found by a four-chunk ballot up to 256 nodes
and by bisection above.  tests/bow_shapes.py builds FeatureVectors of exactly those shapes and descriptors whose distances are known by construction, and holds a
numpy model of the two reference loops.  Every case: model == oracle (CPU), then product == oracle, all by exact equality of nmatches and match12.

Case -> branch:
  test_node_size_edges[len2]                 register walk (<= 256) with a contested feature in every register chunk; general walk (>= 257), chunks >= 11 (>= 705),
                                             taken_hi (>= 4097: the contested feature of the last place sits in a chunk >= 64), the last supported size 8192
  test_overflow_*                            len2 = 8193: overflow flag, ORBHIP_ERR_UNSUPPORTED, every live pair of a batch reset to -1, the arena clean afterwards
  test_side1_block_shapes                    the `blk` loop: one block, a full one, a short last one, three; `taken` carried from block to block
  test_ties_and_gate_edges_*                 first / last of equal minima across lanes and chunks, second == best, TH_LOW at 50 and 49, the ratio at float equality
  test_winner_lane_sweep_*                   bm_wave_min: best and runner-up at every lane (row shifts, row_bcast:15 / :31), every register chunk
  test_node_lookup                           bm_find_node: ballot (nf2 <= 256) and bisection (257, 600); nodes absent / below / above / first / last; idle waves
  test_triangulation_node_shapes             k_bow_triangulate's two walks up to an 8193-feature node (no limit there), selective epipolar gate, the epipole's
                                             radius deciding planted pairs in both walks (the register walk's precomputed near-epipole flags too)
  test_fused_forms_at_the_line_gate          the fp_contract kernel against the model's fused statements where they and the unfused ones part
  test_batch_forms                           several pairs in one launch (the prefix table from block to pair): mixed shapes, an empty side, a shared side
  test_seeded_sweep_*                        random shapes, 1 .. 300 nodes: few large ones; over 256 on both sides (bisection by every workgroup of a full grid)
Single-pair and batched entry points run the same kernels and the same host routine (a single-pair call is a batch of one), so every case here is on the code
the back end's loops use; tests/test_bow_pair_contract.py pins the two forms to each other.
For taken_hi and the cross-block `taken` the evidence is the "first claimant removed -> the second one's answer changes" assertion."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_shapes as B  # noqa: E402
import orb_slam2_amd  # noqa: E402
from orb_slam2_amd import orbhip as H  # noqa: E402

NODE_EDGES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192]
F_X = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32) * np.float32(1.0 / 300)      # a translation along x: the line gate bounds |y2 - y1| per octave


def _bow(backend, oracle, sc, mode, nnratio=0.75, check_ori=True, model=True):
    args = sc.bow_args(mode)
    n_o, m_o = oracle.search_by_bow(mode, *args, nnratio=nnratio, check_ori=check_ori)
    if model:
        n_m, m_m = B.search_by_bow(mode, *args, nnratio=nnratio, check_ori=check_ori)
        assert n_m == n_o and np.array_equal(m_m, m_o), "model != oracle"
    n_g, m_g = orb_slam2_amd.search_by_bow(mode, *args, nnratio=nnratio, check_ori=check_ori, library=backend)
    assert n_g == n_o and np.array_equal(m_g, m_o), (n_g, n_o, np.nonzero(m_g != m_o)[0][:10])
    return n_o, m_o


def _tri(backend, oracle, sc, F=F_X, ex=-5000.0, ey=-5000.0, only_stereo=False, check_ori=True, model=True, stats=None, fused=False):
    args = sc.tri_args(F, ex, ey)
    n_o, m_o = oracle.search_for_triangulation(*args, only_stereo=only_stereo, check_ori=check_ori)
    if model:
        n_m, m_m = B.search_for_triangulation(*args, only_stereo=only_stereo, check_ori=check_ori, stats=stats)
        assert n_m == n_o and np.array_equal(m_m, m_o), "model != oracle"
    n_g, m_g = orb_slam2_amd.search_for_triangulation(*args, only_stereo=only_stereo, check_ori=check_ori, library=backend)
    assert n_g == n_o and np.array_equal(m_g, m_o), (n_g, n_o, np.nonzero(m_g != m_o)[0][:10])
    if fused:                                                   # gcc's contracted forms: the model's fused statements are the reference.  On these
        # scenes the two forms agree (the fp_contract kernel walks the same shapes); test_fused_forms_at_the_line_gate is where they differ
        n_f, m_f = B.search_for_triangulation(*args, only_stereo=only_stereo, check_ori=check_ori, fused=True)
        n_g, m_g = orb_slam2_amd.search_for_triangulation(*args, only_stereo=only_stereo, check_ori=check_ori, library=backend, fp_contract=1)
        assert n_g == n_f and np.array_equal(m_g, m_f), ("fused", n_g, n_f)
    return n_o, m_o


def _contests(sc, node, pairs, spots):
    """per j one family: side-1 places pairs[j] = (first claimant, second or None), side-2 places spots[j] = (target, runner-up or None).  The target is 20 from
    the first claimant and 23 from the second, the runner-up 30 and 33: the first takes the target, the second is left the runner-up (or nothing) - and takes
    the target (23 < 0.75 * 33) once the first is gone."""
    out = []
    for (pa, pb), (pt, pr) in zip(pairs, spots):
        i1, i2 = sc.plant(node, [(pa, 0)] + ([(pb, 3)] if pb is not None else []), [(pt, 20)] + ([(pr, 30)] if pr is not None else []))
        out.append(dict(first=int(i1[0]), second=int(i1[1]) if pb is not None else None, target=int(i2[0]), runner=int(i2[1]) if pr is not None else None))
    return out


def _assert_losers(oracle, sc, mode, groups, m_with, **kw):
    """the second claimants lose a side-2 feature they would have taken: with the first ones removed the oracle hands them the targets"""
    groups = [g for g in groups if g["second"] is not None]
    assert groups
    keep = sc.valid1.copy()
    sc.valid1[[g["first"] for g in groups]] = 0
    _, m_without = oracle.search_by_bow(mode, *sc.bow_args(mode), **kw)
    sc.valid1[:] = keep
    for g in groups:
        assert m_with[g["first"]] == g["target"] and m_with[g["second"]] == (g["runner"] if g["runner"] is not None else -1) and m_without[g["second"]] == g["target"], g


def _edge_scene(len2, seed=0):
    """one node of len2 side-2 features with a contested feature at the last place, in every register chunk and on both sides of chunk 64, as far as they exist"""
    rng = np.random.default_rng(1000 + len2 + seed)
    spots = [(p, p - 1 if p else None) for p in sorted({p for p in (3, 67, 131, 195, 259, 720, 4090, 4099, 8000, len2 - 1) if p < len2})]
    g = len(spots)
    sc = B.Scene(rng, [(3, 2, 40), (7, 2 * g + 3, len2), (9, 4, 0), (11, 0, 6)])
    groups = _contests(sc, 7, [(j, g + 1 + j) for j in range(g)], spots)
    groups += _contests(sc, 3, [(0, None)], [(17, 30)])
    sc.valid2[rng.random(sc.n2) < 0.1] = 0                      # mode 1: side-2 features without a map point ...
    sc.valid2[[x for grp in groups for x in (grp["target"], grp["runner"]) if x is not None]] = 1      # ... none of them planted
    return sc, groups


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("len2", NODE_EDGES)
def test_node_size_edges(backend, oracle, len2, mode, check_ori):
    sc, groups = _edge_scene(len2)
    n_o, m_o = _bow(backend, oracle, sc, mode, check_ori=check_ori)
    assert n_o > 0
    if len2 >= 4097:
        at = {int(np.nonzero(B.members(sc.fv2, 7) == g["target"])[0][0]) >> 6 for g in groups[:-1]}
        assert min(at) < 64 <= max(at) and any(c >= 64 for c in at)          # contested features on both sides of chunk 64
    _assert_losers(oracle, sc, mode, groups, m_o, nnratio=0.75, check_ori=check_ori)


def _c_sides(scs):
    """ctypes sides of Scenes (both sides each) -> (keep-alive list, [(BowSide 1, BowSide 2)])"""
    keep, out = [], []
    for sc in scs:
        pair = []
        for d, a, v, fv in ((sc.d1, sc.k1["angle"], sc.valid1, sc.fv1), (sc.d2, sc.k2["angle"], sc.valid2, sc.fv2)):
            arrs = [np.ascontiguousarray(d), np.ascontiguousarray(a, np.float32), np.ascontiguousarray(v), np.ascontiguousarray(fv[0], np.uint32), np.ascontiguousarray(fv[1], np.int32),
                    np.ascontiguousarray(fv[2], np.uint32)]
            keep.extend(arrs)
            p = [H._p(x).value for x in arrs]
            pair.append(H.BowSide(p[0], p[1], p[2], len(d), p[3], p[4], p[5], len(fv[0])))
        out.append(pair)
    return keep, out


def _overflow_scenes():
    rng = np.random.default_rng(77)
    ok1, ok2, big = B.Scene(rng, [(3, 5, 70), (8, 70, 300)]), B.Scene(rng, [(1, 3, 3), (2, 4, 65)]), B.Scene(rng, [(5, 10, 8193), (9, 4, 30)])
    for sc in (ok1, ok2, big):
        sc.fill()
    return ok1, ok2, big


@pytest.mark.parametrize("mode", [0, 1])
def test_overflow_single_call(backend, oracle, mode):
    """a node of 8193 side-2 features: the wrapper raises naming the limit, and the next call on the thread is right (arena and overflow word clean)"""
    ok1, _, big = _overflow_scenes()
    with pytest.raises(orb_slam2_amd.OrbHipError, match="8192"):
        orb_slam2_amd.search_by_bow(mode, *big.bow_args(mode), library=backend)
    n_o, _ = _bow(backend, oracle, ok1, mode)
    assert n_o > 0


@pytest.mark.parametrize("mode", [0, 1])
def test_overflow_in_a_batch(backend, oracle, mode):
    """three pairs, the middle one overflowing: the batch call fails as a whole, every live pair's match12 is -1 and nmatches 0 (C ABI), the wrapper raises,
    and the same thread's next batch and single calls are right"""
    ok1, ok2, big = _overflow_scenes()
    L = H.lib(backend)
    keep, sides = _c_sides([ok1, big, ok2])
    arr = (H.BowPair * 3)()
    outs = [np.full(sc.n1, 7, np.int32) for sc in (ok1, big, ok2)]
    for k in range(3):
        arr[k].side1 = C.pointer(sides[k][0]); arr[k].side2 = C.pointer(sides[k][1]); arr[k].match12 = H._p(outs[k]).value; arr[k].nmatches = 5
    st = L.orbhip_search_by_bow_batch(0, mode, 3, arr, C.c_float(0.75), 1)
    assert st == H.ERR_UNSUPPORTED and b"8192" in L.orbhip_last_error()
    assert all(np.all(o == -1) for o in outs) and all(arr[k].nmatches == 0 for k in range(3))
    as_pairs = lambda scs: [(dict(desc=s.d1, angle=s.k1["angle"], valid=s.valid1, fv=s.fv1), dict(desc=s.d2, angle=s.k2["angle"], valid=s.valid2, fv=s.fv2)) for s in scs]
    with pytest.raises(orb_slam2_amd.OrbHipError, match="8192"):
        H.search_by_bow_batch(mode, as_pairs([ok1, big, ok2]), nnratio=0.75, library=backend)
    got = H.search_by_bow_batch(mode, as_pairs([ok1, ok2]), nnratio=0.75, library=backend)
    for sc, (n_g, m_g) in zip((ok1, ok2), got):
        n_o, m_o = oracle.search_by_bow(mode, *sc.bow_args(mode), nnratio=0.75)
        assert n_g == n_o and np.array_equal(m_g, m_o) and n_o > 0
    _bow(backend, oracle, ok2, mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("len2", [64, 200])
@pytest.mark.parametrize("c1", [1, 64, 65, 130])
def test_side1_block_shapes(backend, oracle, c1, len2, mode):
    """side 1 of a register-walk node in blocks of 64: contested side-2 features whose claimants lie in different blocks (where there are two), claimants
    without a map point at lane 0, at lane 63, at the last place of a short block and inside a block, and in mode 1 a would-be winner without a map point on
    side 2 (the runner-up is promoted)"""
    rng = np.random.default_rng(c1 * 1000 + len2)
    sc = B.Scene(rng, [(4, c1, len2), (6, 68, len2)])
    lanes = [int(x) for x in rng.permutation(len2)[:18]]
    spots = [(lanes[2 * j], lanes[2 * j + 1]) for j in range(9)]        # places inside a node: the two nodes use the same ones
    # node 6 (68 claimants: a full block and a short one of four): first claimants in block 0, second ones in block 1 and at block 0's end
    groups = _contests(sc, 6, [(1, 64), (62, 65), (30, 61)], spots[:3])
    # first claimants without a map point - lane 0, lane 63, the short block's last place, inside: the second ones take the targets
    dead = _contests(sc, 6, [(0, 60), (63, 59), (67, 66), (31, 58)], spots[3:7])
    pairs4 = {1: [(0, None)], 64: [(1, 62), (31, 32)], 65: [(0, 64), (33, 63)], 130: [(0, 65), (62, 128), (66, 126), (67, 125)]}[c1]
    groups4 = _contests(sc, 4, pairs4, spots[:len(pairs4)])
    ends4 = {1: [], 64: [(0, 61), (63, 60)], 65: [(62, 61)], 130: [(129, 124), (63, 123), (64, 122), (127, 121)]}[c1]      # 130: blocks of 64, 64 and 2
    dead4 = _contests(sc, 4, ends4, spots[4:4 + len(ends4)])
    blind = _contests(sc, 6, [(40, None)], [spots[8]])                # mode 1: the target has no map point -> the runner-up (30 < 0.75 * ~128)
    for g in dead + dead4:
        sc.valid1[g["first"]] = 0
    sc.valid2[blind[0]["target"]] = 0
    n_o, m_o = _bow(backend, oracle, sc, mode)
    assert n_o > 0
    for g in dead + dead4:
        assert m_o[g["first"]] == -1 and m_o[g["second"]] == g["target"]
    assert m_o[blind[0]["first"]] == (blind[0]["runner"] if mode == 1 else blind[0]["target"])
    if mode == 1:                                                  # promoted correctly: with the flag cleared nothing else moves
        sc.valid2[blind[0]["target"]] = 1
        _, m_seen = oracle.search_by_bow(1, *sc.bow_args(1), nnratio=0.75)
        sc.valid2[blind[0]["target"]] = 0
        assert np.nonzero(m_seen != m_o)[0].tolist() == [blind[0]["first"]]
    _assert_losers(oracle, sc, mode, groups + groups4, m_o, nnratio=0.75)


def _tie_scene(len2, seed):
    """one rule per node; every node one claimant at place 0 and len2 side-2 features.  -> scene, {rule: claimant}, {rule: (side-2 features by place)}"""
    rules = {                                                       # targets (place, distance); places 5 / 9: one chunk, 5 / 70: two chunks
        "gate50": [(5, 50)], "gate49": [(5, 49)], "gate51": [(5, 51)],
        "tie_lanes": [(5, 20), (9, 20)], "tie_chunks": [(5, 20), (70, 20)], "tie_late_first": [(70, 20), (5, 20)], "no_tie_lanes": [(5, 20), (9, 28)], "no_tie_chunks": [(70, 20), (5, 28)],
        "r30_40": [(5, 30), (70, 40)], "r29_40": [(70, 29), (5, 40)], "r30_41": [(5, 30), (9, 41)], "r7_10": [(9, 7), (5, 10)], "r6_10": [(5, 6), (70, 10)],
        "tri_first_smaller": [(5, 15), (70, 20)], "tri_three": [(5, 20), (9, 20), (70, 20)], "tri_late_bigger": [(5, 20), (70, 21)],
    }
    rng = np.random.default_rng(seed)
    sc = B.Scene(rng, [(10 + 2 * j, 1, len2) for j in range(len(rules))])
    who, where = {}, {}
    for j, (name, targets) in enumerate(rules.items()):
        i1, i2 = sc.plant(10 + 2 * j, [(0, 0)], targets, dy=0.0)
        who[name], where[name] = int(i1[0]), dict(zip([p for p, _ in targets], i2.tolist()))
    return sc, who, where, rules


@pytest.mark.parametrize("len2", [100, 300])
def test_ties_and_gate_edges_search_by_bow(backend, oracle, len2):
    """both walks (len2 = 100: registers, 300: general).  The first of equal minima would win, but a tie makes second == best and the ratio test fails; TH_LOW is
    `<=` in mode 0 and `<` in mode 1; the ratio test is float32: 30 < 0.75f * 40 and 7 < 0.7f * 10 (= 7.0f after rounding) are false."""
    sc, who, where, rules = _tie_scene(len2, 5)
    res = {(mode, r): _bow(backend, oracle, sc, mode, nnratio=r, check_ori=False)[1] for mode in (0, 1) for r in (0.75, 0.7)}
    for mode in (0, 1):
        _bow(backend, oracle, sc, mode, nnratio=0.75, check_ori=True)
    hit = lambda mode, r, name: int(res[(mode, r)][who[name]])
    first = lambda name: where[name][min(rules[name], key=lambda t: (t[1], t[0]))[0]]      # the nearest target
    assert hit(0, 0.75, "gate50") >= 0 and hit(1, 0.75, "gate50") == -1 and hit(0, 0.75, "gate51") == -1
    assert hit(0, 0.75, "gate49") >= 0 and hit(1, 0.75, "gate49") >= 0
    for mode in (0, 1):
        for name in ("tie_lanes", "tie_chunks", "tie_late_first"):
            assert hit(mode, 0.75, name) == -1                      # second == best
        for name in ("no_tie_lanes", "no_tie_chunks", "r29_40", "r30_41"):
            assert hit(mode, 0.75, name) == first(name), name
        assert hit(mode, 0.75, "r30_40") == -1                      # 30 < 30.0f
        assert hit(mode, 0.7, "r7_10") == -1 and hit(mode, 0.7, "r6_10") == first("r6_10")


@pytest.mark.parametrize("len2", [100, 300])
def test_ties_and_gate_edges_triangulation(backend, oracle, len2):
    """`dist <= bestDist`: the last of equal admissible candidates wins, across lanes and across chunks; a later chunk with a bigger minimum does not; the
    candidate at 50 is admissible, the one at 51 is not"""
    sc, who, where, _ = _tie_scene(len2, 6)
    n_o, m_o = _tri(backend, oracle, sc, check_ori=False)
    _tri(backend, oracle, sc, check_ori=True)
    hit = lambda name: int(m_o[who[name]])
    assert hit("tie_lanes") == where["tie_lanes"][9] and hit("tie_chunks") == where["tie_chunks"][70] and hit("tie_late_first") == where["tie_late_first"][70]
    assert hit("tri_three") == where["tri_three"][70] and hit("tri_first_smaller") == where["tri_first_smaller"][5] and hit("tri_late_bigger") == where["tri_late_bigger"][5]
    assert hit("gate50") >= 0 and hit("gate51") == -1 and hit("r30_40") == where["r30_40"][5]
    drop = where["tie_chunks"][70]                                  # the accepted instance's counterpart: without the later one the earlier one is the answer
    sc.has2[drop] = 1
    _, m_d = oracle.search_for_triangulation(*sc.tri_args(F_X, -5000.0, -5000.0), check_ori=False)
    sc.has2[drop] = 0
    assert m_d[who["tie_chunks"]] == where["tie_chunks"][5]


def _lane_scene(len2, tie):
    """64 nodes of len2 side-2 features: node p has its best at lane p (of chunk p % 4 where there are four) and the runner-up at lane (7 p + 3) % 64 (of the
    next chunk); tie: the two are equally far (SearchForTriangulation's last-wins key)"""
    rng = np.random.default_rng(len2 + tie)
    sc = B.Scene(rng, [(100 + p, 1, len2) for p in range(64)])
    nch = len2 // 64
    best = {}
    for p in range(64):
        pb, pr = (p % nch) * 64 + p, ((p + 1) % nch) * 64 + (p * 7 + 3) % 64
        i1, i2 = sc.plant(100 + p, [(0, 0)], [(pb, 20), (pr, 20 if tie else 30)], dy=0.0)
        best[int(i1[0])] = int(i2[1]) if tie and pr > pb else int(i2[0])
    return sc, best


@pytest.mark.parametrize("len2", [64, 256])
def test_winner_lane_sweep_search_by_bow(backend, oracle, len2):
    sc, best = _lane_scene(len2, False)
    for mode in (0, 1):
        n_o, m_o = _bow(backend, oracle, sc, mode, check_ori=False)
        assert n_o == 64 and all(m_o[i] == b for i, b in best.items())
        _bow(backend, oracle, sc, mode, nnratio=0.6, check_ori=False)      # 20 < 0.6f * 30 fails: the runner-up's distance is read from its lane too


@pytest.mark.parametrize("len2", [64, 256])
def test_winner_lane_sweep_triangulation(backend, oracle, len2):
    for tie in (True, False):
        sc, best = _lane_scene(len2, tie)
        n_o, m_o = _tri(backend, oracle, sc, check_ori=False)
        assert n_o == 64 and all(m_o[i] == b for i, b in best.items())      # tie: the later place of the two


def _lookup_scene(nf2, nfv1):
    ids2 = [10 + 2 * j for j in range(nf2)]
    kinds = {1: ["last"], 2: ["first", "absent"], 3: ["below", "last", "above"], 5: ["below", "first", "absent", "last", "above"]}[nfv1]
    at = {"below": 1, "first": ids2[0], "absent": ids2[nf2 // 2] + 1, "last": ids2[-1], "above": ids2[-1] + 7}
    ids1 = sorted({at[k] for k in kinds})
    while len(ids1) < nfv1:                                          # (one node on side 2: first == last)
        ids1.append(ids1[-1] + 2)
    shape = sorted([(i, 3 if i in ids1 else 0, 2 if i in ids2 else 0) for i in set(ids1) | set(ids2)])
    sc = B.Scene(np.random.default_rng(nf2 * 10 + nfv1), shape)
    assert len(sc.fv1[0]) == nfv1 and len(sc.fv2[0]) == nf2
    sc.fill()
    sc.plant(int(np.intersect1d(sc.fv1[0], sc.fv2[0])[0]), [(0, 0)], [(0, 20)], dy=0.0)      # one match that is there whatever fill() drew
    return sc


@pytest.mark.parametrize("nfv1", [1, 2, 3, 5])
@pytest.mark.parametrize("nf2", [1, 255, 256, 257, 600])
def test_node_lookup(backend, oracle, nf2, nfv1):
    sc = _lookup_scene(nf2, nfv1)
    for mode in (0, 1):
        assert _bow(backend, oracle, sc, mode, nnratio=0.9, check_ori=False)[0] > 0
    assert _tri(backend, oracle, sc, check_ori=False)[0] > 0


@pytest.mark.parametrize("only_stereo", [False, True])
@pytest.mark.parametrize("len2", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_triangulation_node_shapes(backend, oracle, len2, only_stereo):
    """key points jittered about the epipolar line by about its gate, stereo flags and map points mixed; canonical arithmetic against the oracle and the fused
    forms against the model's.  The epipole sits among planted pairs that lie exactly on their lines (y2 == y1): a target inside 10 px * sqrt(scale factor of
    its octave) of it is refused where both key points are monocular, in every register chunk of node 3 and at the last place of node 7 (the general walk
    from 257 on) - against a far epipole the oracle matches every one of them."""
    rng = np.random.default_rng(len2 * 2 + only_stereo)
    sc = B.Scene(rng, [(3, 150, 200), (7, 40, len2)])
    sc.fill(dy=1.6)
    sc.st1[:] = rng.random(sc.n1) < 0.5; sc.st2[:] = rng.random(sc.n2) < 0.5
    sc.has1[:] = rng.random(sc.n1) < 0.1; sc.has2[:] = rng.random(sc.n2) < 0.1
    ex, ey = np.float32(321.5), np.float32(207.25)
    # (node, side-1 place, side-2 place, target's offset from the epipole, its octave, stereo 1, stereo 2, refused)
    plan = [(3, 0, 10, (3, 0), 0, 0, 0, True), (3, 1, 70, (6, -6), 7, 0, 0, True), (3, 2, 130, (12, 0), 0, 0, 0, False), (3, 3, 199, (12, 0), 4, 0, 0, True),
            (3, 4, 40, (0, 25), 7, 0, 0, False), (3, 5, 100, (3, 0), 0, 1, 0, False), (3, 6, 160, (3, 0), 0, 0, 1, False), (7, 0, len2 - 1, (4, 3), 2, 0, 0, True)]
    pairs = []
    for node, p1, p2, (ox, oy), octave, s1, s2, refused in plan:
        c = B.members(sc.fv1, node)[p1]
        sc.k1["y"][c] = ey + np.float32(oy)
        i1, i2 = sc.plant(node, [(p1, 0)], [(p2, 20)], dy=0.0)
        sc.k2["x"][i2] = ex + np.float32(ox); sc.k2["octave"][i2] = octave
        sc.st1[i1], sc.st2[i2], sc.has1[i1], sc.has2[i2] = s1, s2, 0, 0
        pairs.append((int(i1[0]), int(i2[0]), refused))
    stats = {}
    n_o, m_o = _tri(backend, oracle, sc, ex=ex, ey=ey, only_stereo=only_stereo, stats=stats, fused=True)
    assert n_o > 0 and 0.2 <= stats["rejected"] / stats["admissible"] <= 0.8, stats
    _, m_far = oracle.search_for_triangulation(*sc.tri_args(F_X, -5000.0, -5000.0), only_stereo=only_stereo)
    if only_stereo:                                                  # monocular key points of side 1 are not looked at: the gate has nothing to refuse
        assert np.array_equal(m_far, m_o) and all(m_o[c] == -1 for c, _, _ in pairs)
    else:
        assert np.nonzero(m_far != m_o)[0].tolist() == sorted(c for c, _, refused in pairs if refused)
        assert all(m_far[c] == t and m_o[c] == (-1 if refused else t) for c, t, refused in pairs)
    _tri(backend, oracle, sc, ex=ex, ey=ey, only_stereo=only_stereo, check_ori=False)


def test_fused_forms_at_the_line_gate(backend, oracle):
    """Where the two arithmetic forms part: under a general F every side-2 target's y is solved in double so that num * num / den of its pair sits at
    3.84 * sigma2[octave], within the rounding of y - the rounding the fused and the unfused statements differ by.  The model's two forms then give different
    answers, the canonical kernel equals the unfused one (and the oracle), the fp_contract kernel the fused one: this is what checks the model's fma and tells
    a fused kernel from a canonical one.  One register-walk node and one of the general walk."""
    rng = np.random.default_rng(12)
    sc = B.Scene(rng, [(3, 120, 200), (7, 100, 300)])
    sc.fill(contested=0.0)                                           # every side-1 feature has a target of its own
    F = np.array([[0, -1e-4, 0.011], [1e-4, 0, -0.96], [-0.012, 0.97, 0.8]], np.float32)
    G = F.astype(np.float64)
    for node in (3, 7):
        m2 = B.members(sc.fv2, node)
        for c in B.members(sc.fv1, node):
            t = m2[int(np.argmin(B.distances(sc.d1[c], sc.d2[m2])))]
            x1, y1, x2 = float(sc.k1["x"][c]), float(sc.k1["y"][c]), float(sc.k2["x"][t])
            la, lb, lc = x1 * G[0, 0] + y1 * G[1, 0] + G[2, 0], x1 * G[0, 1] + y1 * G[1, 1] + G[2, 1], x1 * G[0, 2] + y1 * G[1, 2] + G[2, 2]
            num = float(rng.choice([-1.0, 1.0])) * np.sqrt(3.84 * float(sc.sigma2[sc.k2["octave"][t]]) * (la * la + lb * lb))
            sc.k2["y"][t] = np.float32((num - la * x2 - lc) / lb)
    n_o, m_o = _tri(backend, oracle, sc, F=F, check_ori=False, fused=True)
    n_f, m_f = B.search_for_triangulation(*sc.tri_args(F, -5000.0, -5000.0), check_ori=False, fused=True)
    assert 0.2 * sc.n1 <= n_o <= 0.8 * sc.n1 and 0.2 * sc.n1 <= n_f <= 0.8 * sc.n1      # pairs on both sides of the gate
    for node in (3, 7):
        c = B.members(sc.fv1, node)
        assert (m_f[c] != m_o[c]).any(), node                        # ... and the form decides some of them, in either walk


def _bow_side(sc, side):
    return dict(desc=(sc.d1, sc.d2)[side], angle=(sc.k1, sc.k2)[side]["angle"], valid=(sc.valid1, sc.valid2)[side], fv=(sc.fv1, sc.fv2)[side])


def _tri_side(sc, side, has=None):
    return dict(desc=(sc.d1, sc.d2)[side], kps=(sc.k1, sc.k2)[side], has_mp=(sc.has1, sc.has2)[side] if has is None else has, stereo=(sc.st1, sc.st2)[side], fv=(sc.fv1, sc.fv2)[side],
                scale_factors=sc.scale, level_sigma2=sc.sigma2)


def test_batch_forms(backend, oracle):
    """six pairs per matcher: shapes of the tests above side by side in one launch, a pair with an empty side, a side object that two pairs name"""
    rng = np.random.default_rng(99)
    A = B.Scene(rng, [(2, 1, 63), (4, 64, 64), (6, 65, 65), (9, 130, 200), (11, 3, 0), (12, 0, 5), (15, 20, 257), (20, 10, 4097)])
    Bs = _lookup_scene(600, 5)
    Cs = B.Scene(rng, [(3, 130, 256), (5, 8, 8192)])
    E = B.Scene(rng, [(3, 5, 0)])                                    # nothing on side 2
    for sc in (A, Cs):
        sc.fill()
        sc.valid1[rng.random(sc.n1) < 0.2] = 0; sc.valid2[rng.random(sc.n2) < 0.2] = 0
        sc.st1[:] = rng.random(sc.n1) < 0.5; sc.st2[:] = rng.random(sc.n2) < 0.5; sc.has2[:] = rng.random(sc.n2) < 0.1
    a1, a2, b1, b2, c1, c2 = _bow_side(A, 0), _bow_side(A, 1), _bow_side(Bs, 0), _bow_side(Bs, 1), _bow_side(Cs, 0), _bow_side(Cs, 1)
    pairs = [(a1, a2), (a2, a1), (b1, b2), (_bow_side(E, 0), _bow_side(E, 1)), (a1, c2), (c1, c2)]      # a1, a2 and c2 are named twice
    for mode in (0, 1):
        got = H.search_by_bow_batch(mode, pairs, nnratio=0.8, check_ori=True, library=backend)
        total = 0
        for k, ((s1, s2), (n_g, m_g)) in enumerate(zip(pairs, got)):
            args = (s1["desc"], s1["angle"], s1["valid"], s1["fv"], s2["desc"], s2["angle"], s2["valid"] if mode == 1 else None, s2["fv"])
            n_o, m_o = oracle.search_by_bow(mode, *args, nnratio=0.8, check_ori=True)
            n_m, m_m = B.search_by_bow(mode, *args, nnratio=0.8, check_ori=True)
            n_s, m_s = orb_slam2_amd.search_by_bow(mode, *args, nnratio=0.8, check_ori=True, library=backend)
            assert n_m == n_o and np.array_equal(m_m, m_o), ("model != oracle", k)
            assert n_g == n_o == n_s and np.array_equal(m_g, m_o) and np.array_equal(m_s, m_o), (mode, k)
            total += n_o
        assert got[3][0] == 0 and len(got[3][1]) == 5 and np.all(got[3][1] == -1) and all(got[k][0] > 0 for k in (0, 1, 2, 5)) and total > 100
    # SearchForTriangulation: key frame 1 = A's side 1 against A's side 2 under two epipolar geometries (one side object), with other map points, an empty one, and Cs
    k1 = _tri_side(A, 0)
    n2 = _tri_side(A, 1)
    F2 = (F_X + np.array([[0, 1e-6, 0], [-1e-6, 0, 0], [0, 0, 2e-4]], np.float32)).astype(np.float32)
    empty = dict(desc=np.zeros((0, 32), np.uint8), kps=A.k2[:0], has_mp=np.zeros(0, np.uint8), stereo=np.zeros(0, np.uint8), fv=(np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32)),
                 scale_factors=A.scale, level_sigma2=A.sigma2)
    nbs = [dict(kf=n2, F12=F_X, ex=-5000.0, ey=-5000.0), dict(kf=n2, F12=F2, ex=float(A.k2["x"][0]), ey=float(A.k2["y"][0])),
           dict(kf=_tri_side(A, 1, has=(rng.random(A.n2) < 0.5).astype(np.uint8)), F12=F_X, ex=300.0, ey=200.0), dict(kf=empty, F12=F_X, ex=0.0, ey=0.0),
           dict(kf=_tri_side(Cs, 1), F12=F_X, ex=-5000.0, ey=-5000.0), dict(kf=_tri_side(Bs, 1), F12=F_X, ex=-5000.0, ey=-5000.0)]
    for only_stereo, ori in ((False, False), (True, True)):
        got = H.search_for_triangulation_batch(k1, nbs, only_stereo=only_stereo, check_ori=ori, library=backend)
        for k, (nb, (n_g, m_g)) in enumerate(zip(nbs, got)):
            if k == 3:
                assert n_g == 0 and np.all(m_g == -1) and len(m_g) == A.n1
                continue
            s2 = nb["kf"]
            args = (k1["desc"], k1["kps"], k1["has_mp"], k1["stereo"], k1["fv"], s2["desc"], s2["kps"], s2["has_mp"], s2["stereo"], s2["fv"], nb["F12"], np.float32(nb["ex"]), np.float32(nb["ey"]),
                    A.scale, A.sigma2)
            n_o, m_o = oracle.search_for_triangulation(*args, only_stereo=only_stereo, check_ori=ori)
            n_m, m_m = B.search_for_triangulation(*args, only_stereo=only_stereo, check_ori=ori)
            n_s, m_s = orb_slam2_amd.search_for_triangulation(*args, only_stereo=only_stereo, check_ori=ori, library=backend)
            assert n_m == n_o and np.array_equal(m_m, m_o), ("model != oracle", k)
            assert n_g == n_o == n_s and np.array_equal(m_g, m_o) and np.array_equal(m_s, m_o), (only_stereo, k)
        assert got[0][0] > 0 and got[1][0] > 0 and got[2][0] > 0


SWEEP_SEED, SWEEP_CASES, SWEEP_BUDGET = 20261018, 40, 3000


def _sweep_scene(rng, case):
    """The node count first: 1 .. 300, every fourth case 1 .. 12 (few, large nodes) and every fourth 290 .. 300 (bisection on both sides).  Sizes log-uniform
    in 1 .. hi on each side, hi = 1500 scaled down by SWEEP_BUDGET / nodes once that is below 250, so that a side stays some thousands of features.  One node
    in sixteen on one side only, random validity masks, 30 % contested side-2 features."""
    lo, hi = ((1, 300), (1, 12), (1, 300), (290, 300))[case % 4]
    nodes = int(rng.integers(lo, hi + 1))
    top = int(min(1500, max(8, 6 * SWEEP_BUDGET // nodes)))
    shape = []
    for j in range(nodes):
        c1, c2 = (int(np.exp(rng.uniform(0, np.log(top)))) for _ in range(2))
        lone = rng.random() < 1 / 16
        shape.append((3 * j + int(rng.integers(0, 3)), 0 if lone and j % 2 else c1, 0 if lone and not j % 2 else c2))
    if sum(s[1] for s in shape) == 0 or sum(s[2] for s in shape) == 0:
        shape.append((3 * nodes + 5, 4, 6))
    sc = B.Scene(rng, shape)
    sc.fill(contested=0.3)
    for flags, p in ((sc.valid1, 0.8), (sc.valid2, 0.8), (sc.has1, 0.2), (sc.has2, 0.2), (sc.st1, 0.5), (sc.st2, 0.5)):
        flags[:] = rng.random(len(flags)) < p
    return sc


def _sweep_covers(shapes):
    """shapes: per case (side-1 nodes, side-2 nodes, largest side-1 node, largest side-2 node) - the sweep holds what it is for"""
    assert sum(a > 256 and b > 256 for a, b, _, _ in shapes) >= 5, shapes          # many workgroups against a bisected side 2
    assert sum(a <= 12 and m2 > 256 for a, _, _, m2 in shapes) >= 5, shapes        # few nodes, the general walk
    assert max(m2 for *_, m2 in shapes) > 1000 and max(m1 for _, _, m1, _ in shapes) > 1000 and min(a for a, *_ in shapes) <= 3, shapes


def _sweep_shape(sc):
    return len(sc.fv1[0]), len(sc.fv2[0]), int(np.diff(sc.fv1[1]).max()), int(np.diff(sc.fv2[1]).max())


def test_seeded_sweep_search_by_bow(backend, oracle):
    """forty cases; model == oracle and product == oracle in every one of them"""
    rng = np.random.default_rng(SWEEP_SEED)
    total, shapes = 0, []
    for case in range(SWEEP_CASES):
        sc = _sweep_scene(rng, case)
        shapes.append(_sweep_shape(sc))
        mode, ratio, ori = case % 2, float(rng.choice([0.6, 0.75, 0.9])), bool(rng.integers(0, 2))
        args = sc.bow_args(mode)
        n_o, m_o = oracle.search_by_bow(mode, *args, nnratio=ratio, check_ori=ori)
        n_m, m_m = B.search_by_bow(mode, *args, nnratio=ratio, check_ori=ori)
        assert n_m == n_o and np.array_equal(m_m, m_o), f"model != oracle: seed {SWEEP_SEED} case {case}"
        n_g, m_g = orb_slam2_amd.search_by_bow(mode, *args, nnratio=ratio, check_ori=ori, library=backend)
        assert n_g == n_o and np.array_equal(m_g, m_o), f"seed {SWEEP_SEED} case {case}: nodes {len(sc.fv1[0])} / {len(sc.fv2[0])}, features {sc.n1} / {sc.n2}, mode {mode}, ratio {ratio}, ori {ori}"
        total += n_o
    _sweep_covers(shapes)
    assert total > 40 * SWEEP_CASES


def test_seeded_sweep_triangulation(backend, oracle):
    """forty cases; model == oracle and product == oracle in every one of them"""
    rng = np.random.default_rng(SWEEP_SEED + 1)
    total, shapes = 0, []
    for case in range(SWEEP_CASES):
        sc = _sweep_scene(rng, case)
        shapes.append(_sweep_shape(sc))
        only, ori = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        centre = int(rng.integers(0, sc.n2))
        args = sc.tri_args(F_X, sc.k2["x"][centre] + np.float32(1.5), sc.k2["y"][centre])
        n_o, m_o = oracle.search_for_triangulation(*args, only_stereo=only, check_ori=ori)
        n_m, m_m = B.search_for_triangulation(*args, only_stereo=only, check_ori=ori)
        assert n_m == n_o and np.array_equal(m_m, m_o), f"model != oracle: seed {SWEEP_SEED + 1} case {case}"
        n_g, m_g = orb_slam2_amd.search_for_triangulation(*args, only_stereo=only, check_ori=ori, library=backend)
        assert n_g == n_o and np.array_equal(m_g, m_o), f"seed {SWEEP_SEED + 1} case {case}: nodes {len(sc.fv1[0])} / {len(sc.fv2[0])}, features {sc.n1} / {sc.n2}, only_stereo {only}, ori {ori}"
        total += n_o
    _sweep_covers(shapes)
    assert total > 20 * SWEEP_CASES
