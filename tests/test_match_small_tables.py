"""SearchForInitialization with k_match_select's per-feature tables indexed by the POSITION of a feature in F2's bucket table (its octave-0 key
points inside the grid) and k_match_candidates' records carrying that position: frames in which position is not index, table lengths and level-0
counts around the 16 / 64 lane boundaries, the order-dependent paths (steal chains across the 64-query step, the list rescan, the rotation
histogram) and the resident batch path - match count and matches12 equal to the CPU oracle's, vbPrevMatched bit-identical; every case on the LDS
and on the device-memory form of the tables."""
import numpy as np
import pytest

import orb_slam2_amd
from orb_slam2_amd import synth

W, H = 400, 300


def _kps(rng, n, octave=0, x=None, y=None):
    k = np.zeros(n, orb_slam2_amd.KEYPOINT_DTYPE)
    k["x"] = rng.uniform(2, W - 2, n).astype(np.float32) if x is None else x
    k["y"] = rng.uniform(2, H - 2, n).astype(np.float32) if y is None else y
    k["size"], k["response"], k["class_id"] = 31.0, 1.0, -1
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k["octave"] = octave
    return k


def _flip(rng, d, nbits):
    """d with nbits distinct bits flipped: Hamming distance exactly nbits"""
    d = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _scene(rng, n1l0, n2l0, others1=7, others2=9, jitter=3.0, shuffle=True):
    """F2: n2l0 octave-0 key points + others2 of higher octaves; F1: n1l0 octave-0 key points near F2's (cycled, so several compete for one feature)
    with noisy copies of its descriptors + others1 of higher octaves; both in shuffled index order."""
    k2 = np.concatenate([_kps(rng, n2l0), _kps(rng, others2, octave=rng.integers(1, 8, others2))])
    d2 = _rand_desc(rng, len(k2))
    src = np.arange(n1l0) % max(n2l0, 1)
    k1 = _kps(rng, n1l0)
    d1 = _rand_desc(rng, n1l0)
    if n2l0:
        k1["x"] = k2["x"][src] + rng.uniform(-jitter, jitter, n1l0).astype(np.float32)
        k1["y"] = k2["y"][src] + rng.uniform(-jitter, jitter, n1l0).astype(np.float32)
        k1["angle"] = k2["angle"][src]
        d1 = np.stack([_flip(rng, d2[s], int(rng.integers(0, 40))) for s in src]) if n1l0 else d1
    k1 = np.concatenate([k1, _kps(rng, others1, octave=rng.integers(1, 8, others1))])
    d1 = np.concatenate([d1, _rand_desc(rng, others1)])
    if shuffle:
        p1, p2 = rng.permutation(len(k1)), rng.permutation(len(k2))
        k1, d1, k2, d2 = k1[p1], d1[p1], k2[p2], d2[p2]
    return k1, d1, k2, d2


def _check(backend, oracle, k1, d1, k2, d2, window=40, nnratio=0.9, ori=True, prev=None):
    m = orb_slam2_amd.ORBmatcher(nnratio, ori, library=backend)
    n_o, m_o, p_o = oracle.search_for_initialization(k1, d1, k2, d2, W, H, prev=prev, window=window, nnratio=nnratio, check_ori=ori)
    n_g, m_g, p_g = m.SearchForInitialization(k1, d1, k2, d2, W, H, vbPrevMatched=prev, windowSize=window)
    assert n_g == n_o and np.array_equal(m_g, m_o) and p_g.tobytes() == p_o.tobytes()
    return n_o, m_o


# ---------------------------------------------------------------------------------------------------------------- position is not index
def test_octaves_interleaved_and_shuffled(backend, oracle, select_tables):
    """octave-0 key points of F2 are neither a prefix of its key points nor ascending in the table"""
    rng = np.random.default_rng(101)
    k1, d1, k2, d2 = _scene(rng, 150, 120, others1=60, others2=200)
    l0 = np.flatnonzero(k2["octave"] == 0)
    assert l0[0] > 0 and l0[-1] > len(l0)                       # not a prefix
    n, m12 = _check(backend, oracle, k1, d1, k2, d2)
    assert n > 40 and m12.max() >= len(l0)                      # a matched index above any table position


def test_key_points_outside_the_grid(backend, oracle, select_tables):
    """octave-0 key points of F2 outside the image bounds take no table entry: positions skip indices"""
    rng = np.random.default_rng(102)
    k1, d1, k2, d2 = _scene(rng, 90, 80, shuffle=False)
    out = np.arange(0, 80, 3)
    k2["x"][out[::2]] = W + 5.0
    k2["x"][out[1::2]] = -20.0
    k2["y"][out[::4]] = H + 9.0
    p = rng.permutation(len(k2))
    n, m12 = _check(backend, oracle, k1, d1, k2[p], d2[p])
    assert n > 20
    _check(backend, oracle, k1, d1, k2[p], d2[p], window=1000)          # ... and with every entry a candidate of every query


def test_no_octave0_key_points_in_f2(backend, oracle, select_tables):
    rng = np.random.default_rng(103)
    k1, d1, k2, d2 = _scene(rng, 70, 0, others2=50)
    n, m12 = _check(backend, oracle, k1, d1, k2, d2, window=100)
    assert n == 0 and np.all(m12 == -1)


@pytest.mark.parametrize("length", [1, 15, 16, 17, 63, 64, 65])
def test_table_lengths(backend, oracle, select_tables, length):
    rng = np.random.default_rng(200 + length)
    k1, d1, k2, d2 = _scene(rng, 70, length, others2=30)
    n, _ = _check(backend, oracle, k1, d1, k2, d2, window=30)
    assert n > 0
    _check(backend, oracle, k1, d1, k2, d2, window=1000, ori=False)     # every candidate count == the table length == the lists' stride


# ---------------------------------------------------------------------------------------------------------------- rows of the candidate kernel
@pytest.mark.parametrize("n1l0", [1, 3, 4, 5, 63, 64, 65, 129])
def test_level0_counts_of_f1(backend, oracle, select_tables, n1l0):
    """ragged last waves of k_match_candidates and the 64-query step boundary of the select loop"""
    rng = np.random.default_rng(300 + n1l0)
    k1, d1, k2, d2 = _scene(rng, n1l0, 100)
    n, _ = _check(backend, oracle, k1, d1, k2, d2, window=50)
    assert n > 0


@pytest.mark.parametrize("full_row", [0, 1, 2, 3])
def test_one_long_run_beside_three_empty_ones(backend, oracle, select_tables, full_row):
    """a window so small that three of four consecutive level-0 key points of F1 have no table entry in reach, while the fourth has more than 64"""
    rng = np.random.default_rng(400 + full_row)
    nclu = 90
    k2 = _kps(rng, nclu, x=rng.uniform(300, 303, nclu).astype(np.float32), y=rng.uniform(100, 103, nclu).astype(np.float32))
    d2 = _rand_desc(rng, nclu)
    k1 = _kps(rng, 12, x=rng.uniform(30, 40, 12).astype(np.float32))                # twelve key points = three groups of four; nothing of F2 near x = 30..40
    d1 = _rand_desc(rng, 12)
    for g in range(3):
        j = 4 * g + full_row
        k1["x"][j], k1["y"][j] = 301.5, 101.5
        d1[j] = _flip(rng, d2[17 * g + 5], 3 + g)
    n, m12 = _check(backend, oracle, k1, d1, k2, d2, window=6, ori=False)
    assert n == 3 and [int(j) % 4 for j in np.flatnonzero(m12 >= 0)] == [full_row] * 3


def test_runs_of_different_lengths(backend, oracle, select_tables):
    """the four key points of one group reach 3, 20, 70 and 150 table entries"""
    rng = np.random.default_rng(500)
    sizes, xs = [3, 20, 70, 150], [40.0, 140.0, 240.0, 340.0]
    k2 = np.concatenate([_kps(rng, s, x=rng.uniform(x - 2, x + 2, s).astype(np.float32)) for s, x in zip(sizes, xs)])
    d2 = _rand_desc(rng, len(k2))
    order = [0, 1, 2, 3, 3, 2, 1, 0, 2, 0, 3, 1, 1, 3]                                 # last group ragged
    k1 = _kps(rng, len(order), x=np.array([xs[o] for o in order], np.float32))
    start = np.cumsum([0] + sizes)
    d1 = np.stack([_flip(rng, d2[start[o] + i % sizes[o]], i % 5) for i, o in enumerate(order)])
    for i, o in enumerate(order):
        k1["y"][i] = k2["y"][start[o] + i % sizes[o]]
    n, _ = _check(backend, oracle, k1, d1, k2, d2, window=10, ori=False)
    assert n >= 8


def test_candidate_count_reaches_the_list_stride(backend, oracle, select_tables):
    """one key point of F1 sees every table entry (its list is as long as the lists' stride), the others a handful"""
    rng = np.random.default_rng(600)
    k1, d1, k2, d2 = _scene(rng, 30, 140, shuffle=True)
    prev = np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32)
    j = int(np.flatnonzero(k1["octave"] == 0)[7])
    prev[j] = (200.0, 150.0)
    n, _ = _check(backend, oracle, k1, d1, k2, d2, window=15, prev=prev)
    assert n > 5
    _check(backend, oracle, k1, d1, k2, d2, window=250, prev=prev)       # 250 px around the centre of 400x300: every entry


# ---------------------------------------------------------------------------------------------------------------- order-dependent paths
@pytest.mark.parametrize("competitors", [70, 130])
def test_steal_chain_across_the_64_query_step(backend, oracle, select_tables, competitors):
    """many key points of F1 at one place compete for ONE descriptor of F2 at distances that fall along the index order: each later one steals the
    match of an earlier one (ORBmatcher.cc:463-467), across the 64-query steps of the select loop"""
    rng = np.random.default_rng(700 + competitors)
    N = competitors
    k2 = _kps(rng, N)
    d2 = _rand_desc(rng, N)
    k1 = _kps(rng, N, x=np.full(N, k2["x"][0], np.float32), y=np.full(N, k2["y"][0], np.float32))
    d1 = np.stack([_flip(rng, d2[0], max(0, 45 - i // 3) + (i % 3)) for i in range(N)])    # 45, 46, 47, 44, 45, 46, ...: falling with ties and rises
    n, m12 = _check(backend, oracle, k1, d1, k2, d2, window=100)
    assert n >= 1 and int((m12 == 0).sum()) == 1 and int(np.flatnonzero(m12 == 0)[0]) > 64
    _check(backend, oracle, k1, d1, k2, d2, window=100, ori=False)


@pytest.mark.parametrize("pad", [0, 60])
def test_rescan_of_a_used_up_record_set(backend, oracle, select_tables, pad):
    """a key point whose recorded best candidates are all matched at smaller distances by earlier key points when its turn comes, while its list
    holds more: its list is scanned again against the current state (pad = 60: its turn comes in the next 64-query step)"""
    rng = np.random.default_rng(800 + pad)
    base = _rand_desc(rng, 1)[0]
    x0, y0 = 210.0, 160.0
    near = np.stack([_flip(rng, base, 3) for _ in range(6)])                            # six features of F2 close to `base` ...
    q7 = _flip(rng, base, 3)
    far = np.stack([_flip(rng, q7, 40), _rand_desc(rng, 1)[0], _rand_desc(rng, 1)[0]])   # ... one at distance 40 of the last query, two anywhere
    k2 = _kps(rng, 9, x=(x0 + np.arange(9)).astype(np.float32), y=np.full(9, y0, np.float32))
    d2 = np.concatenate([near, far])
    npad = pad
    kpad = _kps(rng, npad, x=rng.uniform(5, 60, npad).astype(np.float32))               # key points of F1 far from everything (no candidates)
    k1 = np.concatenate([_kps(rng, 6, x=np.full(6, x0, np.float32), y=np.full(6, y0, np.float32)), kpad,
                         _kps(rng, 1, x=np.full(1, x0, np.float32), y=np.full(1, y0, np.float32))])
    d1 = np.concatenate([near, _rand_desc(rng, npad), q7[None]])                        # the first six take their features at distance 0
    for ori in (False, True):
        n, m12 = _check(backend, oracle, k1, d1, k2, d2, window=30, ori=ori)
        if not ori:
            assert n == 7 and list(m12[:6]) == [0, 1, 2, 3, 4, 5] and m12[-1] == 6      # the last one found the feature outside its four records


@pytest.mark.parametrize("second,third", [(5, 3), (30, 4), (30, 20)])
def test_rotation_histogram_maxima(backend, oracle, select_tables, second, third):
    """100 matches at rotation 0, `second` at 85 degrees and `third` at 180: with checkOri the bins under 10 % of the largest are dropped"""
    rng = np.random.default_rng(900 + second + third)
    N = 100 + second + third
    k2 = _kps(rng, N)
    d2 = _rand_desc(rng, N)
    k1 = k2.copy()
    rot = np.concatenate([np.zeros(100), np.full(second, 85.0), np.full(third, 180.0)]).astype(np.float32)
    k2["angle"] = rng.uniform(0, 170, N).astype(np.float32)
    k1["angle"] = k2["angle"] + rot
    p = rng.permutation(N)
    k1, d1 = k1[p], d2[p]
    n_on, _ = _check(backend, oracle, k1, d1, k2, d2, window=8, ori=True)
    n_off, _ = _check(backend, oracle, k1, d1, k2, d2, window=8, ori=False)
    assert n_off > n_on or (second >= 10 and third >= 10)
    if (second, third) == (5, 3):
        assert n_off - n_on == 8
    if (second, third) == (30, 4):
        assert n_off - n_on == 4


# ---------------------------------------------------------------------------------------------------------------- batches
@pytest.fixture(scope="module")
def nine_slots(oracle):
    """nine camera slots over three time steps, slot 4 blank at the last one; the oracle's key points and matches (computed once, never changed)"""
    w, h, n, B = 400, 300, 500, 9
    ora = oracle.OracleExtractor(n, 1.2, 8, 20, 7)
    seqs = [[im.copy() for im in synth.sequence(w, h, 3, seed=40 + s)] for s in range(B)]
    seqs[4][2][:] = 0
    K = [[ora.extract(im) for im in s] for s in seqs]
    assert len(K[4][2][0]) == 0 and len(K[4][1][0]) > 0
    want = {(t, s): oracle.search_for_initialization(K[s][t - 1][0], K[s][t - 1][1], K[s][t][0], K[s][t][1], w, h, window=100, nnratio=0.9)[:2] for t in (1, 2) for s in range(B)}
    return w, h, n, B, seqs, K, want


def test_resident_batch_of_nine_frames(backend, select_tables, nine_slots):
    """extract_device(match_prev=True) on nine camera slots (above the eight-frame switch of the schedule), twice; one frame of the second call blank"""
    w, h, n, B, seqs, K, want = nine_slots
    ex = orb_slam2_amd.ORBextractor(n, 1.2, 8, 20, 7, w, h, max_batch=B, library=backend)
    pitch = 448
    dbuf = orb_slam2_amd.DeviceBuffer(B * h * pitch, library=backend)
    for t in range(3):
        host = np.zeros((B, h, pitch), np.uint8)
        for s in range(B):
            host[s, :, :w] = seqs[s][t]
        ex.sync()
        dbuf.upload(host)
        ex.extract_device(dbuf.ptr, B, h * pitch, pitch, match_prev=(t > 0), window=100, nnratio=0.9, check_ori=True)
        ks, ds = ex.fetch(B)
        for s in range(B):
            assert ks[s].tobytes() == K[s][t][0].tobytes() and np.array_equal(ds[s], K[s][t][1]), (t, s)
        if t > 0:
            m12, nm = ex.fetch_matches(B)
            for s in range(B):
                assert nm[s] == want[t, s][0] and np.array_equal(m12[s], want[t, s][1]), (t, s)
    assert sum(want[1, s][0] for s in range(B)) > 200 and want[2, 4][0] == 0
    ex.close()
