"""The windowed searches behind Fuse (both overloads) and both passes of SearchBySim3 - k_best_in_window / k_best_in_window_fc over the table of
k_match_grid / k_match_grid_big - at the shapes natural frames never reach: cells with up to a thousand key points (the in-cell sort that restores key point
order after the racing scatter, the prefix scan across waves), dozens of equal best distances with the winner in a chosen lane of a chosen 64-entry step,
key points exactly on the radius, the level window at level 0 and at the top level, chi-square products on either side of the literals 5.99 / 7.8, the sign
of mvuRight that selects the stereo branch, key points on exact rounding ties of the grid and key points the grid drops, queries on, beside and far outside
the bounds, and the call shapes (1..5 queries, empty slots, 64 shared slots with skip bits, a held slot).

Every answer must equal the oracle's (oracle.search_best_in_window / search_by_projection: the reference's loops one query at a time).  Every shape a test
claims is asserted from tests/window_shapes.py - a numpy restatement of the table order and of the run a query scans - BEFORE the library is called.
Emulation on the CPU (where the scatter's atomics already return ascending positions: the sorts are really exercised only with -m gpu), the real library with -m gpu."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_slam2_amd  # noqa: E402
from orb_slam2_amd import orbhip as H  # noqa: E402
import pose_opt_cases as Cs  # noqa: E402
import window_shapes as W  # noqa: E402

f32 = np.float32
VGA = (0.0, 0.0, 640.0, 480.0)                     # cells of 10 x 10 px
POW2 = (0.0, 0.0, 512.0, 384.0)                    # inverse cell size exactly 0.125: coordinates 8k + 4 are exact rounding ties
OFFSET = (-13.5, -9.25, 531.0, 397.5)              # bounds of non-zero origin, as a distorted camera gives
INV = Cs.inv_level_sigma2()                        # mvInvLevelSigma2 of the extractor: 8 levels, scale 1.2


def _emu(backend):
    return backend.endswith("_emu.so")


def _search(backend, oracle, kps, desc, bounds, q, qd, chi2, ur=None):
    """the library's answer, checked against the oracle's"""
    with oracle.image_bounds_set(bounds):
        bi_o, bd_o = oracle.search_best_in_window(kps, desc, 0, 0, INV, q, qd, chi2, u_right=ur)
    bi_g, bd_g = orb_slam2_amd.search_best_in_window(kps, desc, 0, 0, INV, q, qd, chi2, u_right=ur, bounds=bounds, library=backend)
    bad = np.flatnonzero((bi_g != bi_o) | (bd_g != bd_o))
    assert len(bad) == 0, f"queries {bad[:8]}: library {bi_g[bad[:8]]} / {bd_g[bad[:8]]}, oracle {bi_o[bad[:8]]} / {bd_o[bad[:8]]}"
    return bi_o, bd_o


def _first_in_table(tab, q):
    """with every candidate at one distance: the first entry of the scanned run that passes the radius and the level window"""
    out = np.full(len(q), -1, np.int32)
    for i in range(len(q)):
        pos, idx = tab.level_window(q[i])
        if len(idx):
            out[i] = idx[0]
    return out


def _cell_queries(rng, bounds, px, py, nq=70):
    """queries on and around cell (px, py): radii 0.5 .. 5 px, levels 0 .. 3; the first one on the cell's centre with a radius that covers the cell"""
    gw, gh = W.inv_cell(bounds)
    cx, cy = f32(bounds[0]) + f32(px) / gw, f32(bounds[1]) + f32(py) / gh
    q = W.queries(cx + rng.uniform(-6, 6, nq).astype(f32), cy + rng.uniform(-6, 6, nq).astype(f32), rng.uniform(0.5, 5.0, nq).astype(f32), rng.integers(0, 4, nq))
    q["x"][0], q["y"][0], q["radius"][0], q["level"][0] = cx, cy, 0.5 / gw, 1
    q["ur"] = q["x"] - f32(4.0)
    return q


# ------------------------------------------------------------------------------------------------------------------------------ a. crowded cells, LDS form
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1024])
def test_one_crowded_cell(backend, oracle, n):
    """Every key point of the frame in ONE cell, all with one descriptor: every candidate ties, the answer is the first in table order that passes the gates -
    which is key point order, whatever order the scatter's atomics handed out.  Then the ties in four clumps of four descriptors through the order-dependent
    reader of the same table, search_by_projection."""
    if _emu(backend):
        n = min(n, 257)
    rng = np.random.default_rng(n)
    px, py = 20, 17
    kps = W.one_cell_frame(rng, n, VGA, px, py)
    tab = W.Table(kps, VGA)
    assert tab.population(px, py) == n and len(tab.dropped()) == 0 and np.array_equal(tab.order, np.arange(n))
    D = W.descriptor(1)
    desc = np.tile(D, (n, 1))
    q = _cell_queries(rng, VGA, px, py)
    assert len(tab.in_window(q[0])[1]) == n                                      # the first query sees the whole cell
    qd = np.tile(W.at_distance(D, 3), (len(q), 1))
    want = _first_in_table(tab, q)
    assert (want >= 0).sum() >= (10 if n > 2 else 1)
    bi, bd = _search(backend, oracle, kps, desc, VGA, q, qd, False)
    assert np.array_equal(bi, want) and np.all(bd[want >= 0] == 3)
    ur = np.where(rng.random(n) < 0.5, kps["x"] - f32(4.0) + rng.normal(0, 1.0, n), -1.0).astype(f32)
    _search(backend, oracle, kps, desc, VGA, q, qd, True)
    _search(backend, oracle, kps, desc, VGA, q, qd, True, ur=ur)
    # four clumps, four descriptors, the order-dependent search
    Ds = np.stack([W.descriptor(10 + k) for k in range(4)])
    clump = rng.integers(0, 4, n)
    desc4 = Ds[clump]
    kps["angle"] = rng.choice([0.0, 90.0], n)
    pq = np.zeros(len(q), oracle.PROJ_QUERY_DTYPE)
    pq["x"], pq["y"], pq["radius"], pq["ur"] = q["x"], q["y"], q["radius"], q["ur"]
    pq["min_level"], pq["max_level"] = q["level"] - 1, q["level"] + 1
    pq["blocks"] = rng.random(len(q)) < 0.7
    pqd = Ds[rng.integers(0, 4, len(q))].copy()
    for i in range(len(q)):
        pqd[i] = W.at_distance(pqd[i], int(rng.integers(0, 4)))
    _search(backend, oracle, kps, desc4, VGA, q, pqd, False)
    matches = 0
    for mode in (0, 1):
        with oracle.image_bounds_set(VGA):
            n_o, f_o = oracle.search_by_projection(kps, desc4, 0, 0, pq, pqd, mode, nnratio=0.9, th_high=100, check_ori=True)
        n_g, f_g = orb_slam2_amd.search_by_projection(kps, desc4, 0, 0, pq, pqd, mode, nnratio=0.9, th_high=100, check_ori=True, bounds=VGA, library=backend)
        assert n_g == n_o and np.array_equal(f_g, f_o), f"mode {mode}"
        matches += n_o
    assert matches > 0


def test_three_crowded_cells_across_the_waves(backend, oracle):
    """2048 key points over three cells whose counters lie in the 12-cell ranges of three different threads in three different waves, one of them the last
    thread's: the exclusive scan across the wave totals and the table's end, start[3072]."""
    rng = np.random.default_rng(5)
    cells, counts = [(5, 7), (30, 10), (63, 40)], [700, 700, 648]
    owner = [(px * W.ROWS + py) // 12 for px, py in cells]
    assert owner[2] == 255 and len({t // 64 for t in owner}) == 3
    parts = [W.one_cell_frame(rng, c, VGA, px, py) for (px, py), c in zip(cells, counts)]
    kps = np.concatenate(parts)[rng.permutation(2048)]
    tab = W.Table(kps, VGA)
    assert [tab.population(px, py) for px, py in cells] == counts and tab.start[W.CELLS] == 2048
    D = W.descriptor(2)
    desc = np.tile(D, (2048, 1))
    for px, py in cells:
        q = _cell_queries(rng, VGA, px, py, 24)
        qd = np.tile(D, (len(q), 1))
        want = _first_in_table(tab, q)
        assert (want >= 0).sum() >= 8
        bi, bd = _search(backend, oracle, kps, desc, VGA, q, qd, False)
        assert np.array_equal(bi, want)
        _search(backend, oracle, kps, desc, VGA, q, qd, True)


# ------------------------------------------------------------------------------------------------------------------------------ b. crowded cells, large-frame form
@pytest.mark.gpu
def test_crowded_cells_of_a_frame_too_large_for_lds(gpu_lib, oracle):
    """24 000 key points: the table is built in place in device memory (k_match_grid_big), its cells sorted there.  Three cells hold 64, 65 and 512 key points
    of one descriptor, the others a uniform spread; the queries sit on the three cells."""
    n = 24000
    assert W.grid_lds_bytes((n + 63) & ~63) > W.GRID_LDS_MAX and W.grid_lds_bytes(23000) <= W.GRID_LDS_MAX
    rng = np.random.default_rng(24)
    cells, counts = [(12, 9), (33, 30), (50, 21)], [64, 65, 512]
    nrest = n - sum(counts)
    x, y = rng.uniform(0, 639, nrest).astype(f32), rng.uniform(0, 479, nrest).astype(f32)
    px, py = W.grid_coords(x, y, VGA)
    for cx, cy in cells:                                                          # the spread keeps out of the three cells
        hit = (px == cx) & (py == cy)
        x[hit] += f32(30.0)
    rest = W.keypoints(x, y, rng.integers(0, 4, nrest))
    kps = np.concatenate([rest] + [W.one_cell_frame(rng, c, VGA, cx, cy) for (cx, cy), c in zip(cells, counts)])
    perm = rng.permutation(n)
    kps = kps[perm]
    crowded = perm >= nrest
    tab = W.Table(kps, VGA)
    assert [tab.population(cx, cy) for cx, cy in cells] == counts
    Ds = np.stack([W.descriptor(20 + k) for k in range(4)])
    desc = Ds[rng.integers(1, 4, n)]
    desc[crowded] = Ds[0]
    for cx, cy in cells:
        q = _cell_queries(rng, VGA, cx, cy, 70)
        q["radius"][1:8] = 12.0
        qd = np.tile(W.at_distance(Ds[0], 2), (len(q), 1))
        bi, bd = _search(gpu_lib, oracle, kps, desc, VGA, q, qd, False)
        assert (bd == 2).sum() >= 10
        _search(gpu_lib, oracle, kps, desc, VGA, q, qd, True)


# ------------------------------------------------------------------------------------------------------------------------------ c. winner lane and step
SWEEP = list(range(64)) + [64 * c + l for c in (1, 2) for l in (0, 1, 31, 62, 63)]


@pytest.fixture(scope="module")
def tie_frame():
    """210 key points in three neighbouring cells of two grid columns, their indices interleaved over the cells (table order is not index order), all inside
    ONE query's window; 7 more in a column left of the run the query scans, so that the run does not start at the table's first entry"""
    rng = np.random.default_rng(11)
    n = 210
    cells = np.array([(30, 20), (30, 21), (31, 20)])[np.arange(n) % 3]
    x = (cells[:, 0] + rng.uniform(-0.2, 0.2, n)) * 10.0
    y = (cells[:, 1] + rng.uniform(-0.2, 0.2, n)) * 10.0
    kps = np.concatenate([W.keypoints(x, y, 2), W.keypoints(np.full(7, 270.0), np.full(7, 205.0), 2)])
    q = W.queries([305.0], [205.0], 9.0, level=2)
    tab = W.Table(kps, VGA)
    t_lo, t_hi = tab.column_run(q["x"][0], q["radius"][0])
    assert t_lo == 7 and t_hi == n + 7
    pos, idx = tab.in_window(q[0])
    assert np.array_equal(pos, np.arange(n)) and not np.array_equal(idx, np.arange(n)) and sorted(idx) == list(range(n))
    return kps, q, idx                                                            # idx[p]: the key point at run position p


def test_winner_by_level_at_every_lane(backend, oracle, tie_frame):
    """All candidates tie; only those at run positions >= p are inside the query's level window: the winner stands in lane p % 64 of step p // 64"""
    kps0, q, at = tie_frame
    D = W.descriptor(3)
    desc = np.tile(D, (len(kps0), 1))
    qd = W.at_distance(D, 5)[None]
    for p in SWEEP:
        kps = kps0.copy()
        kps["octave"][at[:p]] = np.where(np.arange(p) % 2, 3, 0)                  # above and below the window 1 .. 2
        kps["octave"][at[p:]] = np.where(np.arange(len(at) - p) % 2, 2, 1)
        pos, idx = W.Table(kps, VGA).level_window(q[0])
        assert pos[0] == p and len(pos) == len(at) - p and idx[0] == at[p]
        bi, bd = _search(backend, oracle, kps, desc, VGA, q, qd, False)
        assert bi[0] == at[p] and bd[0] == 5, f"position {p}"


@pytest.mark.parametrize("d", [0, 1, 255])
def test_winner_by_distance_at_every_lane(backend, oracle, tie_frame, d):
    """The candidates before run position p are at distance d + 1, the one at p and all later ones at d (d + 1 = 256: never a candidate)"""
    kps, q, at = tie_frame
    D = W.descriptor(4)
    near, far = W.at_distance(D, d), W.at_distance(D, d + 1)
    assert W.hamming(D, near) == d and W.hamming(D, far) == d + 1
    tab = W.Table(kps, VGA)
    for p in SWEEP:
        desc = np.tile(near, (len(kps), 1))
        desc[at[:p]] = far
        pos, idx = tab.level_window(q[0])
        assert np.array_equal(idx, at) and np.all(desc[idx[:p]] == far) and np.all(desc[idx[p:]] == near)
        bi, bd = _search(backend, oracle, kps, desc, VGA, q, D[None], False)
        assert bi[0] == at[p] and bd[0] == d, f"position {p}"


def test_distance_256_never_wins(backend, oracle, tie_frame):
    kps, q, at = tie_frame
    D = W.descriptor(5)
    desc = np.tile(W.at_distance(D, 256), (len(kps), 1))
    assert W.hamming(D, desc[0]) == 256 and len(W.Table(kps, VGA).level_window(q[0])[1]) == len(at)
    bi, bd = _search(backend, oracle, kps, desc, VGA, q, D[None], False)
    assert bi[0] == -1 and bd[0] == 256


# ------------------------------------------------------------------------------------------------------------------------------ d. radius and level edges
@pytest.mark.parametrize("r", [3, 10])
def test_key_points_exactly_on_the_radius(backend, oracle, r):
    """|dx| < r and |dy| < r are strict: a key point at q +- r is outside, one at q +- (r - 1) inside, in x and in y separately.  Query k carries key point k's
    descriptor: an excluded key point must lose to a stranger at a distance around 128."""
    qx, qy = 300.0, 200.0
    offs = [(s * e, 0) for e in (r, r - 1) for s in (1, -1)] + [(0, s * e) for e in (r, r - 1) for s in (1, -1)]
    inside = np.array([max(abs(dx), abs(dy)) < r for dx, dy in offs])
    kps = W.keypoints([qx + dx for dx, dy in offs], [qy + dy for dx, dy in offs], 0)
    desc = np.random.default_rng(r).integers(0, 256, (len(kps), 32), dtype=np.uint8)
    q = W.queries(np.full(len(kps), qx), np.full(len(kps), qy), float(r), level=0)
    tab = W.Table(kps, VGA)
    assert sorted(tab.in_window(q[0])[1]) == list(np.flatnonzero(inside)) and inside.sum() == 4
    bi, bd = _search(backend, oracle, kps, desc, VGA, q, desc, False)
    assert np.array_equal(bi[inside], np.flatnonzero(inside)) and np.all(bd[inside] == 0)
    assert np.all(inside[bi[~inside]]) and np.all(bd[~inside] > 60)
    _search(backend, oracle, kps, desc, VGA, q, desc, True)


def test_level_window_at_the_bottom_and_the_top(backend, oracle):
    """Key points of level L-1 .. L only, for L = 0 (nothing below), 1 and 7: key points at L-2 .. L+1 on one spot, each sought by its own descriptor"""
    for L in (0, 1, 7):
        lv = np.array([l for l in range(L - 2, L + 2) if l >= 0])
        kps = W.keypoints(300.0 + np.arange(len(lv)), np.full(len(lv), 200.0), lv)
        desc = np.random.default_rng(L).integers(0, 256, (len(lv), 32), dtype=np.uint8)
        q = W.queries(np.full(len(lv), 301.0), np.full(len(lv), 200.0), 6.0, level=L)
        tab = W.Table(kps, VGA)
        inside = (lv >= L - 1) & (lv <= L)
        assert sorted(tab.level_window(q[0])[1]) == list(np.flatnonzero(inside)) and len(tab.in_window(q[0])[1]) == len(lv)
        bi, bd = _search(backend, oracle, kps, desc, VGA, q, desc, False)
        assert np.array_equal(bi[inside], np.flatnonzero(inside)) and np.all(inside[bi[~inside]]) and np.all(bd[~inside] > 60), f"level {L}"


# ------------------------------------------------------------------------------------------------------------------------------ e. the chi-square gate
CENTRED = (-320.0, -240.0, 320.0, 240.0)           # the key point of the gate tests stands on (0, 0): ex = q.x exactly, at the full resolution of a small float


def _straddle(literal, level, stereo):
    """two queries among the float32 neighbours of a point on the gate's boundary: the one with the largest product (W.chi2_product) at or below the literal,
    and the one with the smallest product above it.  The squares skip floats, so the search runs over neighbouring columns AND rows."""
    inv = INV[level]
    qur, ur = f32(1.5), (f32(0.5) if stereo else None)
    rest = 0.75 ** 2 + (1.0 if stereo else 0.0)
    xs, ys = np.meshgrid(W.neighbours(np.sqrt(literal / float(inv) - rest), 256), W.neighbours(0.75, 32))
    prod = W.chi2_product(xs, ys, qur, 0.0, 0.0, ur, inv)
    assert prod.dtype == f32 and prod.shape == xs.shape
    below = prod.astype(np.float64) <= literal
    assert below.any() and not below.all()
    i = np.unravel_index(np.argmax(np.where(below, prod, -np.inf)), prod.shape)
    o = np.unravel_index(np.argmin(np.where(below, np.inf, prod)), prod.shape)
    return (xs[i], ys[i], prod[i]), (xs[o], ys[o], prod[o]), qur


@pytest.mark.parametrize("level", [0, 3])
@pytest.mark.parametrize("stereo", [False, True])
def test_chi_square_gate_at_the_literal(backend, oracle, stereo, level):
    """e2 * invSigma2 is a float product compared as a double with 5.99 (monocular) / 7.8 (stereo): accepted at or below, rejected above"""
    literal = 7.8 if stereo else 5.99
    (x_in, y_in, p_in), (x_out, y_out, p_out), qur = _straddle(literal, level, stereo)
    kps = W.keypoints([0.0], [0.0], level)
    ur = np.array([0.5 if stereo else -1.0], f32)
    D = W.descriptor(6)
    q = W.queries([x_in, x_out], [y_in, y_out], 20.0, level=level, ur=qur)
    p_in, p_out = (W.chi2_product(qq["x"], qq["y"], qq["ur"], kps["x"][0], kps["y"][0], ur[0] if stereo else None, INV[level]) for qq in q)
    print(f"\n[chi2 gate {literal} level {level}] products {p_in!r} (+{W.float_steps(p_in, f32(literal))} float steps from the literal's float) and {p_out!r} "
          f"(+{W.float_steps(p_out, f32(literal))})")
    assert float(p_in) <= literal < float(p_out)
    assert W.float_steps(p_in, f32(literal)) <= 8 and W.float_steps(p_out, f32(literal)) <= 8
    assert all(len(W.Table(kps, CENTRED).level_window(qq)[1]) == 1 for qq in q)
    bi, bd = _search(backend, oracle, kps, D[None], CENTRED, q, np.tile(D, (2, 1)), True, ur=ur)
    assert list(bi) == [0, -1] and list(bd) == [0, 256]
    bi, bd = _search(backend, oracle, kps, D[None], CENTRED, q, np.tile(D, (2, 1)), False, ur=ur)
    assert list(bi) == [0, 0]


def test_stereo_branch_by_the_sign_of_the_right_coordinate(backend, oracle):
    """mvuRight >= 0 takes the stereo branch: 0.0 and -0.0 do, -1e-30 and -1.0 do not.  Two queries per key point: one the stereo gate accepts and the
    monocular gate rejects (ex^2 + ey^2 = 6.5, er = 0), one the other way round (ex^2 + ey^2 = 4, er = 3)."""
    urs = np.array([0.0, -0.0, -1e-30, -1.0], f32)
    assert np.signbit(urs[1]) and urs[2] < 0
    kx = np.array([-200.0, -100.0, 100.0, 200.0], f32)
    kps = W.keypoints(kx, np.zeros(4), 0)
    desc = np.random.default_rng(8).integers(0, 256, (4, 32), dtype=np.uint8)
    q = np.concatenate([W.queries(kx + f32(2.5), np.full(4, 0.5), 10.0, ur=0.0), W.queries(kx + f32(2.0), np.zeros(4), 10.0, ur=3.0)])
    qd = np.concatenate([desc, desc])
    want = []
    for i in range(8):
        k = i % 4
        stereo = bool(urs[k] >= 0)
        p = W.chi2_product(q["x"][i], q["y"][i], q["ur"][i], kx[k], 0.0, urs[k] if stereo else None, INV[0])
        other = W.chi2_product(q["x"][i], q["y"][i], q["ur"][i], kx[k], 0.0, None if stereo else urs[k], INV[0])
        ok, ok_other = float(p) <= (7.8 if stereo else 5.99), float(other) <= (5.99 if stereo else 7.8)
        assert ok != ok_other                                                     # the two branches disagree on every one of these
        want.append(k if ok else -1)
    assert want == [0, 1, -1, -1, -1, -1, 2, 3]
    bi, bd = _search(backend, oracle, kps, desc, CENTRED, q, qd, True, ur=urs)
    assert list(bi) == want


# ------------------------------------------------------------------------------------------------------------------------------ f. grid boundaries
def _boundary_frame(bounds, special):
    """a sparse lattice on the cells' rounding edges, a random spread that reaches past the bounds on every side, and the special points first"""
    rng = np.random.default_rng(int(abs(bounds[0]) * 4) + 9)
    gw, gh = W.inv_cell(bounds)
    lx = f32(bounds[0]) + (np.arange(0, 64, 3) + 0.5).astype(f32) / gw
    ly = f32(bounds[1]) + (np.arange(0, 48, 3) + 0.5).astype(f32) / gh
    gx, gy = np.meshgrid(lx, ly)
    x = np.concatenate([[p[0] for p in special], gx.ravel(), rng.uniform(bounds[0] - 25, bounds[2] + 25, 300)])
    y = np.concatenate([[p[1] for p in special], gy.ravel(), rng.uniform(bounds[1] - 25, bounds[3] + 25, 300)])
    kps = W.keypoints(x, y, rng.integers(0, 3, len(x)))
    Ds = np.stack([W.descriptor(30 + k) for k in range(4)])
    return kps, Ds[rng.integers(0, 4, len(x))], Ds, rng


def _edge_queries(tab, bounds, rng):
    """(x, radius) pairs whose window edges fall just below / at or above column coordinate 1.0 (left edge) and 62.0 (right edge)"""
    gw, _ = W.inv_cell(bounds)
    out = []
    for target, right in ((1.0, False), (62.0, True)):
        r = f32(12.0)
        x0 = f32(bounds[0]) + f32(target) / gw + (-r if right else r)
        xs = W.neighbours(abs(x0), 64) if x0 > 0 else -W.neighbours(abs(x0), 64)[::-1]
        ends = np.array([tab.column_ends(x, r)[1 if right else 0] for x in xs])
        k = int(np.searchsorted(ends >= f32(target), True))
        assert 0 < k < len(xs) and ends[k - 1] < target <= ends[k]
        out += [(xs[k - 1], r, target, right, False), (xs[k], r, target, right, True)]
    return out


@pytest.mark.parametrize("bounds", [POW2, OFFSET], ids=["pow2", "offset"])
def test_grid_boundaries(backend, oracle, bounds):
    """Key points on exact rounding ties of the grid, key points the grid drops (cell 64 / 48, negative cells), queries on them, in the first and last column,
    beside and far outside the bounds, over the whole table, and with window edges on either side of the column-run cut's branch points"""
    gw, gh = W.inv_cell(bounds)
    if bounds is POW2:
        assert gw == 0.125 and gh == 0.125
        ties = [(4.0, 4.0), (12.0, 20.0), (252.0, 188.0), (500.0, 372.0), (-3.9, 100.0)]
        gone = [(508.0, 100.0), (100.0, 380.0), (508.0, 380.0), (-4.0, 100.0), (100.0, -4.0), (-20.0, -20.0), (520.0, 100.0), (100.0, 390.0), (511.9, 383.9)]
    else:
        ties = [(-17.0, 100.0), (526.0, 100.0), (100.0, -13.0), (100.0, 393.0)]
        gone = [(527.0, 100.0), (530.0, 396.0), (-18.0, 100.0), (100.0, -14.0), (100.0, 394.0), (-40.0, -30.0), (540.0, 100.0)]
    kps, desc, Ds, rng = _boundary_frame(bounds, gone + ties)
    tab = W.Table(kps, bounds)
    ng = len(gone)
    assert np.all(tab.cell[:ng] < 0) and np.all(tab.cell[ng:ng + len(ties)] >= 0)          # the dropped key points really are dropped, the others are not
    assert np.any(tab.px[:ng] == 64) and np.any(tab.py[:ng] == 48) and np.any(tab.px[:ng] < 0) and np.any(tab.py[:ng] < 0)
    if bounds is POW2:
        vx = kps["x"].astype(np.float64) * 0.125
        assert (vx - np.floor(vx) == 0.5).sum() > 300 and np.any((vx == -0.5) & (tab.cell < 0))       # exact ties, one of them negative (rounds away from zero: dropped)
    assert len(tab.dropped()) > ng
    qs = []
    for x, y in gone:                                                             # on the dropped points: alone, and with neighbours in reach
        qs += [(x, y, 3.0), (x, y, 12.0)]
    mid_y = 0.5 * (bounds[1] + bounds[3])
    qs += [(bounds[0] + 2.0, mid_y, 9.0), (bounds[2] - 7.0, mid_y, 9.0)]          # column 0, column 63
    qs += [(bounds[0] - 30.0, mid_y, 40.0), (bounds[2] + 28.0, mid_y, 40.0), (bounds[0] + 100.0, bounds[1] - 30.0, 40.0), (bounds[0] + 100.0, bounds[3] + 28.0, 40.0)]
    qs += [(bounds[0] - 500.0, mid_y, 10.0), (bounds[2] + 1500.0, mid_y, 10.0), (100.0, bounds[1] - 900.0, 10.0)]      # far outside: no candidate
    qs += [(250.0, 190.0, 600.0), (-100.0, 500.0, 600.0)]                         # the whole table
    edge = _edge_queries(tab, bounds, rng)
    qs += [(x, mid_y, r) for x, r, *_ in edge]
    q = W.queries([a[0] for a in qs], [a[1] for a in qs], [a[2] for a in qs], level=1)
    q["ur"] = q["x"] - f32(5.0)
    for (x, r, target, right, above), qq in zip(edge, q[-len(edge):]):            # the side of the branch point each of them is on
        end = tab.column_ends(qq["x"], qq["radius"])[1 if right else 0]
        assert (end >= target) == above and abs(float(end) - target) < 1e-4
    first, last = tab.column_run(q["x"][2 * ng], q["radius"][2 * ng]), tab.column_run(q["x"][2 * ng + 1], q["radius"][2 * ng + 1])
    assert first[0] == 0 and last[1] == tab.start[W.CELLS] and first[1] < last[0]
    whole = 2 * ng + 9
    assert tab.column_run(q["x"][whole], 600.0) == (0, tab.start[W.CELLS]) and len(tab.in_window(q[whole])[1]) == tab.start[W.CELLS]
    for i in range(2 * ng + 6, 2 * ng + 9):
        assert len(tab.in_window(q[i])[1]) == 0
    qd = Ds[np.arange(len(q)) % 4].copy()
    for chi2 in (False, True):
        bi, bd = _search(backend, oracle, kps, desc, bounds, q, qd, chi2)
        assert not np.isin(bi, tab.dropped()).any()                               # a dropped key point is never returned, even with the query on top of it
        if not chi2:
            assert np.array_equal(bi, _first_in_distance(tab, q, desc, qd)) and (bi >= 0).sum() >= 10 and np.all(bi[2 * ng + 6:2 * ng + 9] == -1)


def _first_in_distance(tab, q, desc, qd):
    """the restatement's own answer without the chi-square gate: first smallest distance in scan order"""
    out = np.full(len(q), -1, np.int32)
    for i in range(len(q)):
        pos, idx = tab.level_window(q[i])
        if len(idx):
            d = np.array([W.hamming(desc[j], qd[i]) for j in idx])
            if d.min() < 256:
                out[i] = idx[int(np.argmin(d))]
    return out


# ------------------------------------------------------------------------------------------------------------------------------ g. call shapes
@pytest.fixture(scope="module")
def plain_frame():
    rng = np.random.default_rng(70)
    n = 300
    kps = W.keypoints(rng.uniform(0, 512, n), rng.uniform(0, 384, n), rng.integers(0, 4, n))
    Ds = np.stack([W.descriptor(40 + k) for k in range(6)])
    desc = Ds[rng.integers(0, 6, n)]
    src = rng.integers(0, n, 40)
    q = W.queries(kps["x"][src] + rng.normal(0, 1.5, 40).astype(f32), kps["y"][src] + rng.normal(0, 1.5, 40).astype(f32), rng.choice([3.0, 8.0, 20.0], 40), kps["octave"][src])
    q["ur"] = q["x"] - f32(6.0)
    ur = np.where(rng.random(n) < 0.5, kps["x"] - f32(6.0), -1.0).astype(f32)
    return kps, desc, ur, q, desc[src].copy()


@pytest.mark.parametrize("nq", [1, 3, 4, 5])
def test_query_counts_around_a_workgroup(backend, oracle, plain_frame, nq):
    """the kernel takes four queries per workgroup"""
    kps, desc, ur, q, qd = plain_frame
    bi, bd = _search(backend, oracle, kps, desc, POW2, q[7:7 + nq], qd[7:7 + nq], True, ur=ur)
    assert len(bi) == nq and (bi >= 0).any()


def test_batch_with_empty_slots(backend, oracle, plain_frame):
    """five slots: nothing at all, queries but no key points, key points but no queries, two ordinary ones with different bounds - each equals its own call"""
    kps, desc, ur, q, qd = plain_frame
    slot = lambda k, d, u, b, qq, qdd: dict(kps=k, desc=d, u_right=u, bounds=b, inv_level_sigma2=INV, queries=qq, qdesc=qdd)
    k2 = kps.copy(); k2["x"] += f32(3.0)
    slots = [slot(kps[:0], desc[:0], None, POW2, q[:0], qd[:0]), slot(kps[:0], desc[:0], None, POW2, q[:9], qd[:9]), slot(kps, desc, ur, POW2, q[:0], qd[:0]),
             slot(kps, desc, ur, POW2, q, qd), slot(k2[:211], desc[:211], None, OFFSET, q[:33], qd[:33])]
    for chi2 in (True, False):
        got = orb_slam2_amd.search_best_in_window_batch(slots, chi2, library=backend)
        assert len(got) == 5
        for s, (sl, (bi_g, bd_g)) in enumerate(zip(slots, got)):
            assert len(bi_g) == len(sl["queries"])
            if len(sl["kps"]) == 0 or len(sl["queries"]) == 0:
                assert np.all(bi_g == -1) and np.all(bd_g == 256), f"slot {s}"
                continue
            bi, bd = _search(backend, oracle, sl["kps"], sl["desc"], sl["bounds"], sl["queries"], sl["qdesc"], chi2, ur=sl["u_right"])
            assert np.array_equal(bi_g, bi) and np.array_equal(bd_g, bd) and (bi >= 0).sum() > 10, f"slot {s}"


@pytest.fixture()
def fuse_slots(backend):
    """64 slots of one small key frame under slightly different poses, ONE set of map points: the key points stand where slot 0's projection puts the points"""
    import test_parity_projection_algebra as A
    A._case.library = backend
    rng = np.random.default_rng(64)
    P, pts, log_sf, bounds = A._case(rng, "fuse", 0, npts=160)
    nlv = P.nlevels
    inv = (1.0 / (np.asarray(P.scale_factors[:nlv], f32) ** 2)).astype(f32)
    pdesc = rng.integers(0, 256, (len(pts), 32), dtype=np.uint8)
    empty = W.keypoints([1.0], [1.0], 0)
    _, _, q0 = H.project_best_in_window(empty, pdesc[:1], bounds, inv, P, pts, pdesc, True, library=backend)
    live = np.flatnonzero(q0["radius"] >= 0)
    assert len(live) >= 30
    kps = W.keypoints(q0["x"][live] + rng.normal(0, 0.6, len(live)).astype(f32), q0["y"][live] + rng.normal(0, 0.6, len(live)).astype(f32), q0["level"][live])
    desc = pdesc[live].copy()
    ur = np.where(rng.random(len(live)) < 0.5, q0["ur"][live] + f32(0.25), -1.0).astype(f32)
    Ps = []
    for s in range(64):
        Q = H.Projection.from_buffer_copy(P)
        Q.t[0] += f32(0.002 * (s % 5)); Q.t[1] -= f32(0.001 * (s % 3))
        Ps.append(Q)
    slots = [dict(kps=kps, desc=desc, u_right=ur, bounds=bounds, inv_level_sigma2=inv, proj=Ps[s]) for s in range(64)]
    return slots, pts, pdesc, inv, bounds


def _single(backend, oracle, sl, inv, bounds, pts, pdesc):
    """one slot's points through the one-frame entry; its flat queries through the oracle"""
    bi, bd, qo = H.project_best_in_window(sl["kps"], sl["desc"], bounds, inv, sl["proj"], pts, pdesc, True, u_right=sl["u_right"], library=backend)
    live = qo["radius"] >= 0
    with oracle.image_bounds_set(bounds):
        bi_o, bd_o = oracle.search_best_in_window(sl["kps"], sl["desc"], 0, 0, inv, qo[live], pdesc[live], True, u_right=sl["u_right"])
    assert np.array_equal(bi[live], bi_o) and np.array_equal(bd[live], bd_o) and np.all(bi[~live] == -1) and np.all(bd[~live] == 256)
    return bi, bd


def test_shared_points_over_64_slots_with_skip_bits(backend, oracle, fuse_slots):
    """orbhip_project_best_in_window_shared takes up to 64 slots, one skip bit each: bits 0 and 63 (and some between) set for some points.  A skipped point
    answers -1 / 256, every other one as the slot's own call does."""
    slots, pts, pdesc, inv, bounds = fuse_slots
    rng = np.random.default_rng(1)
    npt = len(pts)
    skip = np.zeros(npt, np.uint64)
    skip[rng.random(npt) < 0.4] |= np.uint64(1)
    skip[rng.random(npt) < 0.4] |= np.uint64(1) << np.uint64(63)
    skip[rng.random(npt) < 0.4] |= np.uint64(1) << np.uint64(31)
    skip[0], skip[1], skip[2] = np.uint64(1), np.uint64(1) << np.uint64(63), np.uint64(0xFFFFFFFFFFFFFFFF)
    got = H.project_best_in_window_shared(slots, pts, pdesc, skip, True, library=backend)
    assert len(got) == 64
    found = 0
    for s in ((0, 1, 30, 31, 32, 62, 63) if _emu(backend) else range(64)):
        bi, bd = _single(backend, oracle, slots[s], inv, bounds, pts, pdesc)
        off = ((skip >> np.uint64(s)) & np.uint64(1)) == 1
        assert off[2] and off[0] == (s == 0) and off[1] == (s == 63)
        assert np.all(got[s][0][off] == -1) and np.all(got[s][1][off] == 256), f"slot {s}"
        assert np.array_equal(got[s][0][~off], bi[~off]) and np.array_equal(got[s][1][~off], bd[~off]), f"slot {s}"
        if s in (0, 31, 63):
            assert (bi[off] >= 0).any()                                           # the bit hides points that would have matched
        found += int((bi >= 0).sum())
    assert found > 100


def test_held_slot_searched_again(backend, oracle, fuse_slots):
    """a middle slot of a shared call searched again with some of the points under changed descriptors: the slot's own call on those"""
    slots, pts, pdesc, inv, bounds = fuse_slots
    slots = slots[:5]
    rng = np.random.default_rng(2)
    H.project_best_in_window_shared(slots, pts, pdesc, None, True, library=backend)
    sub = rng.random(len(pts)) < 0.5
    pd2 = pdesc[sub] ^ (rng.random((int(sub.sum()), 32)) < 0.02).astype(np.uint8)
    hb, hd = H.project_best_in_window_held(2, slots[2]["proj"], pts[sub], pd2, True, library=backend)
    bi, bd = _single(backend, oracle, slots[2], inv, bounds, pts[sub], pd2)
    assert np.array_equal(hb, bi) and np.array_equal(hd, bd) and (bi >= 0).sum() > 10
