"""Frame::ComputeStereoMatches away from the corner of its input space that tests/test_parity_stereo.py covers (at most 2000 key points, at most
520 rows, uniform disparity, a disparity limit far beyond the scene's): mvuRight / mvDepth bit-identical to the oracle where

  * a frame has more key points than k_stereo_rows (SR_T * SR_K = 4096 row ranges) and k_stereo_prune (256 * ST_PR = 4096 correlation distances) keep
    in registers, alone and next to a sparse frame in the same batch, and right at that count;
  * the image is high enough for the row table's prefix sum to give a thread two and three consecutive rows (per = (H + 1024) / 1024);
  * the disparity limit maxD = mbf / mb cuts into the scene's disparities: the candidate gate uR >= uL - maxD and the final disparity < maxD;
  * the disparity varies over the image, so that the correlation's rejections (best shift at an end of the band, parabola vertex further than one
    pixel away) occur and the median prune removes a real share;
  * a frame has none, one, two and a handful of accepted matches (the bisection for the k = n/2-th smallest distance).

Every pair goes through the three forms the library has: two contexts as a batch (the left context builds the row table), two contexts frame by
frame (from the second frame on the RIGHT context builds the table behind its own extraction), and orbhip_extract_stereo (one context, two slots).
Each case asserts on the oracle's own result that the regime it is written for is really reached; `classify` below restates the per-key-point
decision in numpy only to name the reason of every -1 for those assertions - it never judges the library.

Oracle counts per case (key points L / R; accepted; pruned; without candidate; ORB distance >= 75; best shift at a band end; disparity outside
[0, maxD)):
  752x480 / 6000            6003 / 6003   4666  456   68  741  72    0        the sparse slot beside it   1188 / 1098   986  95  6  86  14  1
  752x480 / 6000, 1.3 / 6   6000 / 6002   4652  446   56  756  90    0
  752x480 / 4089 4090 4092  4094 / 4094, 4097 / 4097, 4098 / 4099;  2928, 2932, 2933 accepted; 300 pruned each
  640x1040 / 1500           1504 / 1503    910   92  136  357   9    0        640x1041   1504 / 1505   921  95  135  337  16  0
  640x1100 / 1500           1504 / 1504    949   91  127  325  12    0        44 matched at y >= 1024
  1081x2048 / 1500          1505 / 1505   1011   98  165  230   1    0        484 matched at y >= 1024, 11 at y >= 2000
  480x360 / 600, 21 px      609 / 610     maxD 20: 2 0 434 66 1 106;  21: 135 15 278 58 1 122;  22: 319 23 205 43 1 18;  40: 354 30 158 65 2 0
  480x360 / 600, 9 px       607 / 605     maxD 9.5: 295 20 220 41 1 30;  20: 401 26 137 42 1 0
  gradient 2 + 0.1 x        608 / 608      365   30   53  150  10    0        two planes 4 / 30   606 / 606   350  44  53  152  7  0
  patches                   8 / 8 each: see FEW
What the cases are there to notice, tried once on the emulation with the kernel broken on purpose: a wrong index or a short row range in the
tail loops of k_stereo_rows, or k_stereo_prune's last loop not reaching every key point past 4096, fail the two 6000-feature tests; a prefix sum that adds
only the first of a thread's rows fails every tall shape; a candidate gate without uR >= uL - maxD and a final test without disparity < maxD fail
test_binding_disparity_limit.  One breakage survives: `<` for `<=` in k_stereo_prune's re-reading count alone moves the median only when a key point past
4096 holds exactly the median distance, and the cut only if another distance lies between 2.1 times the two neighbouring values."""
import os
import sys

import numpy as np
import pytest

import orb_slam2_amd
from orb_slam2_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_parity_stereo import MB, MBF, stereo_pair  # noqa: E402

REG = 4096                                         # SR_T * SR_K == 256 * ST_PR (orbhip_kernels_stereo.hip)
f32 = np.float32
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)
REASONS = ("no_candidate", "orb_distance", "border", "end_of_band", "delta", "disparity", "pruned", "accepted")


# ------------------------------------------------------------------------------------------------ scenes
def warped_pair(w, h, seed, disparity):
    """stereo_pair with a disparity that varies over the image: right(x, y) = scene(x + disparity(x, y), y), linear interpolation in float64,
    then the noise and the rounding of stereo_pair."""
    m = 64
    sc = synth.scene(w, h, seed=seed)
    left = synth.frame_from_scene(sc, w, h, t=0, seed=seed)
    yy, xx = np.mgrid[0:h, 0:w]
    xs = m // 2 + xx + np.asarray(disparity(xx, yy), np.float64)
    assert xs.min() >= 0 and xs.max() < sc.shape[1] - 1
    x0 = np.floor(xs).astype(np.int64)
    fr = xs - x0
    val = sc[m // 2 + yy, x0] * (1.0 - fr) + sc[m // 2 + yy, x0 + 1] * fr
    rng = np.random.default_rng(1000 + seed)
    right = np.clip(np.rint(val) + rng.integers(-6, 7, size=(h, w)), 0, 255).astype(np.uint8)
    return left, right


def windowed_pair(w, h, seed, disp, x0, y0, x1, y1, grey=128):
    """stereo_pair flat (`grey`) everywhere but in the window [x0, x1) x [y0, y1) of the left image and the same piece of scene in the right one."""
    left, right = stereo_pair(w, h, seed, disp)
    fl, fr = np.full_like(left, grey), np.full_like(right, grey)
    fl[y0:y1, x0:x1] = left[y0:y1, x0:x1]
    fr[y0:y1, x0 - disp:x1 - disp] = right[y0:y1, x0 - disp:x1 - disp]
    return fl, fr


# ------------------------------------------------------------------------------------------------ the oracle's side, computed once per pair
class OraclePair:
    def __init__(self, oracle, left, right, n, scale, levels):
        self.O, self.left, self.right = oracle, left, right
        self.eL, self.eR = oracle.OracleExtractor(n, scale, levels, 20, 7), oracle.OracleExtractor(n, scale, levels, 20, 7)
        self.kl, self.dl = self.eL.extract(left)
        self.kr, self.dr = self.eR.extract(right)
        self._stereo, self._why = {}, {}

    def stereo(self, mbf, mb):
        if (mbf, mb) not in self._stereo:
            self._stereo[(mbf, mb)] = self.O.stereo_matches(self.eL, self.eR, mbf, mb)
        return self._stereo[(mbf, mb)]

    def why(self, mbf, mb):
        """classify() of this pair; it must agree with the oracle on which key points end with a right coordinate."""
        if (mbf, mb) not in self._why:
            reason, sad, disp = classify(self.eL, self.eR, self.kl, self.dl, self.kr, self.dr, mbf, mb)
            assert np.array_equal(reason == "accepted", self.stereo(mbf, mb)[0] >= 0)
            self._why[(mbf, mb)] = (reason, sad, disp)
        return self._why[(mbf, mb)]


_PAIRS = {}


def oracle_pair(oracle, key, make, n, scale=1.2, levels=8):
    """The pair `make()` builds and the oracle's extraction of it, shared by every test (and both backends) of the session under `key`."""
    key = (key, n, scale, levels)
    if key not in _PAIRS:
        left, right = make()
        _PAIRS[key] = OraclePair(oracle, left, right, n, scale, levels)
    return _PAIRS[key]


def classify(eL, eR, kl, dl, kr, dr, mbf, mb):
    """Why the oracle's ComputeStereoMatches gives each left key point what it gives (Frame.cc:466-640): one of REASONS per key point, the
    correlation distance where one was accepted (-1 elsewhere) and the disparity where one was computed (NaN elsewhere).  Float operations are
    single precision in the reference's order; the sums are integers."""
    par = eL.params()
    sf, isf = par["scale_factors"], par["inv_scale_factors"]
    max_d = f32(mbf) / f32(mb)
    pl = [eL.level(l) for l in range(eL.nlevels)]
    pr = [eR.level(l) for l in range(eR.nlevels)]
    r = f32(2.0) * sf[kr["octave"]]
    lo, hi = np.floor(kr["y"] - r).astype(np.int64), np.ceil(kr["y"] + r).astype(np.int64)
    n = len(kl)
    reason = np.full(n, "no_candidate", dtype="U12")
    sad, disp = np.full(n, -1, np.int64), np.full(n, np.nan, np.float32)

    def rnd(v):                                                       # roundf: halves away from zero (all values are positive)
        return int(np.floor(np.float64(v) + 0.5))

    for i in range(n):
        u_l, v_l, lev = kl["x"][i], kl["y"][i], int(kl["octave"][i])
        c = (lo <= int(v_l)) & (int(v_l) <= hi) & (np.abs(kr["octave"] - lev) <= 1) & (kr["x"] >= u_l - max_d) & (kr["x"] <= u_l)
        idx = np.nonzero(c)[0]
        if len(idx) == 0:
            continue
        dist = _POP[dl[i][None, :] ^ dr[idx]].sum(1)
        j = int(np.argmin(dist))                                      # the first of the smallest: candidates are visited in index order
        if dist[j] >= 75:
            reason[i] = "orb_distance"
            continue
        su_l, sv_l, su_r = rnd(u_l * isf[lev]), rnd(v_l * isf[lev]), rnd(kr["x"][idx[j]] * isf[lev])
        il, ir = pl[lev].astype(np.int64), pr[lev].astype(np.int64)
        if su_r < 0 or su_r + 11 >= ir.shape[1] or su_r - 10 < 0 or su_l - 5 < 0 or su_l + 6 > il.shape[1] or sv_l - 5 < 0 or sv_l + 6 > il.shape[0]:
            reason[i] = "border"
            continue
        a = il[sv_l - 5:sv_l + 6, su_l - 5:su_l + 6] - il[sv_l, su_l]
        d = np.array([np.abs(a - (ir[sv_l - 5:sv_l + 6, su_r + k - 10:su_r + k + 1] - ir[sv_l, su_r + k - 5])).sum() for k in range(11)])
        b = int(np.argmin(d))
        if b in (0, 10):
            reason[i] = "end_of_band"
            continue
        d1, d2, d3 = f32(d[b - 1]), f32(d[b]), f32(d[b + 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = (d1 - d3) / (f32(2.0) * (d1 + d3 - f32(2.0) * d2))
        if delta < -1 or delta > 1:
            reason[i] = "delta"
            continue
        disp[i] = u_l - sf[lev] * ((f32(su_r) + f32(b - 5)) + delta)
        if not (disp[i] >= 0 and disp[i] < max_d):
            reason[i] = "disparity"
            continue
        reason[i], sad[i] = "accepted", d[b]
    if (sad >= 0).any():
        s = np.sort(sad[sad >= 0])
        th = f32(1.5) * f32(1.4) * f32(s[len(s) // 2])
        reason[(sad >= 0) & ~(sad.astype(np.float32) < th)] = "pruned"
    return reason, sad, disp


def counts(reason):
    return {k: int((reason == k).sum()) for k in REASONS}


# ------------------------------------------------------------------------------------------------ the library's side
def _same(u, d, uo, do, what):
    nk = len(uo)
    assert u[:nk].tobytes() == uo.tobytes() and d[:nk].tobytes() == do.tobytes(), what
    assert np.all(u[nk:] == -1) and np.all(d[nk:] == -1), what


def check(backend, w, h, n, pairs, cameras=((MBF, MB),), scale=1.2, levels=8, one_call=True):
    """`pairs` (OraclePair) against the oracle under every (mbf, mb) of `cameras`, through the library's three forms."""
    B = len(pairs)
    xl = orb_slam2_amd.ORBextractor(n, scale, levels, 20, 7, w, h, max_batch=B, library=backend)
    xr = orb_slam2_amd.ORBextractor(n, scale, levels, 20, 7, w, h, max_batch=B, library=backend)
    # frame by frame: the first call builds the row table on the left context's stream; it also tells the right context to build the table behind
    # its next extraction (orbhip_host_path.hip: frame_epilogues), which the second round then takes
    p = pairs[0]
    for rnd in ("rows by the left context", "rows behind the right extraction"):
        kl, _ = xl.extract_batch([p.left])
        xr.extract_batch([p.right])
        assert kl[0].tobytes() == p.kl.tobytes()
        for mbf, mb in cameras:
            u, d = xl.ComputeStereoMatches(xr, mbf, mb, nimg=1)
            _same(u[0], d[0], *p.stereo(mbf, mb), (rnd, mbf, mb))
    # the batch
    if B > 1:
        xl.extract_batch([p.left for p in pairs])
        xr.extract_batch([p.right for p in pairs])
        for mbf, mb in cameras:
            u, d = xl.ComputeStereoMatches(xr, mbf, mb, nimg=B)
            for f, p in enumerate(pairs):
                _same(u[f], d[f], *p.stereo(mbf, mb), ("batch slot %d" % f, mbf, mb))
    xl.close()
    xr.close()
    # one call
    if one_call:
        x = orb_slam2_amd.ORBextractor(n, scale, levels, 20, 7, w, h, max_batch=2, library=backend)
        for f, p in enumerate(pairs):
            for mbf, mb in cameras:
                kl, dl, kr, dr, u, d = x.extract_stereo(p.left, p.right, mbf, mb)
                assert kl.tobytes() == p.kl.tobytes() and np.array_equal(dl, p.dl) and kr.tobytes() == p.kr.tobytes() and np.array_equal(dr, p.dr)
                uo, do = p.stereo(mbf, mb)
                assert u.tobytes() == uo.tobytes() and d.tobytes() == do.tobytes(), ("one call, pair %d" % f, mbf, mb)
        x.close()


# ------------------------------------------------------------------------------------------------ 1. more than 4096 key points per frame
BIG = (752, 480, 6000)


def _big_pair():
    return stereo_pair(BIG[0], BIG[1], 11, 12)


def _sparse_pair():
    return windowed_pair(BIG[0], BIG[1], 13, 12, 300, 170, 480, 300)


def _assert_past_registers(p):
    uo, _ = p.stereo(MBF, MB)
    ok = uo >= 0
    assert len(p.kl) > REG and len(p.kr) > REG and int(ok.sum()) > REG
    assert ok[REG:].any() and (~ok[REG:]).any()                       # key points beyond the registers: some matched, some not


def test_more_than_4096_key_points_in_a_batch_with_a_sparse_frame(backend, oracle):
    """6003 / 6003 key points, 4666 accepted (1475 of them at index >= 4096, 432 there without a match) next to a frame of 1188 / 1098 (986 accepted): one slot
    of the batch runs the re-computing loops of k_stereo_rows and the re-reading loops of k_stereo_prune, the other stays in registers."""
    w, h, n = BIG
    big, sparse = oracle_pair(oracle, "big", _big_pair, n), oracle_pair(oracle, "sparse", _sparse_pair, n)
    _assert_past_registers(big)
    us, _ = sparse.stereo(MBF, MB)
    assert 100 < len(sparse.kl) < 1500 and 100 < len(sparse.kr) < 1500 and 50 < int((us >= 0).sum())
    check(backend, w, h, n, [big, sparse])
    if not backend.endswith("_emu.so"):
        check(backend, w, h, n, [sparse, big], one_call=False)       # and with the slots exchanged (the emulation needs 20 s for it)


def test_more_than_4096_key_points_scale_1_3_six_levels(backend, oracle):
    """The same frame at scale factor 1.3 with 6 levels: the row table's bound out_cap * (ceil(4 * sf[L-1]) + 3) away from 1.2 / 8."""
    w, h, n = BIG
    big = oracle_pair(oracle, "big", _big_pair, n, 1.3, 6)
    _assert_past_registers(big)
    assert int(big.kr["octave"].max()) == 5
    check(backend, w, h, n, [big], scale=1.3, levels=6)


AROUND = (4089, 4090, 4092)                         # nFeatures -> left key points on both sides of 4096 (asserted below)


def test_key_point_counts_around_4096(backend, oracle):
    """Counts within a few of 4096: the last register-resident key point, the first one beyond, and a frame that just fills the registers."""
    w, h, _ = BIG
    seen = set()
    for n in AROUND:
        p = oracle_pair(oracle, "big", _big_pair, n)
        assert 4090 <= len(p.kl) <= 4100 and int((p.stereo(MBF, MB)[0] >= 0).sum()) > 2000
        seen.add(len(p.kl) > REG)
        seen.add(("right", len(p.kr) > REG))
        check(backend, w, h, n, [p], one_call=False)
    assert seen == {True, False, ("right", True), ("right", False)}


# ------------------------------------------------------------------------------------------------ 2. tall frames
@pytest.mark.parametrize("w,h,per", [(640, 1040, 2), (640, 1041, 2), (640, 1100, 2), (1081, 2048, 3)])
def test_tall_frames(backend, oracle, w, h, per):
    """Heights at which a thread of k_stereo_rows' prefix sum owns `per` consecutive ones of the H + 1 row counters: per == 2 with an odd number of
    counters (1040, 1100: the last thread in range owns one) and an even number (1041), and per == 3, which begins at 2048 rows (2049 counters).  A key point lies at least 19 px inside the image, so one at y >= 1024 needs H >= 1044: 640x1040 and 640x1041 cannot have any, 640x1100
    and 1081x2048 must have matched ones; every shape must have matches in the first and the last rows that can hold a key point.
    Contexts refuse a portrait shape where the reference's quadtree would start a level with round(w'/h') = 0 root nodes: at 2048 rows 1081 is
    the narrowest width accepted, 1080x2048 is refused."""
    assert (h + 1024) // 1024 == per
    n = 1500
    p = oracle_pair(oracle, ("tall", w, h), lambda: stereo_pair(w, h, 12, 10), n)
    uo, _ = p.stereo(MBF, MB)
    ok = uo >= 0
    assert len(p.kl) > 1400 and int(ok.sum()) > 800
    if h >= 1044:
        assert int((ok & (p.kl["y"] >= 1024)).sum()) > 10
    if per == 3:
        assert int((ok & (p.kl["y"] >= 2000)).sum()) > 0
        with pytest.raises(orb_slam2_amd.OrbHipError):
            orb_slam2_amd.ORBextractor(n, 1.2, 8, 20, 7, w - 1, h, library=backend)
    assert (ok & (p.kl["y"] >= h - 40)).any() and (ok & (p.kl["y"] < 40)).any()           # the first and the last rows that can hold a key point
    check(backend, w, h, n, [p])


# ------------------------------------------------------------------------------------------------ 3. a disparity limit that binds
def test_binding_disparity_limit(backend, oracle):
    """Disparity 21 px under maxD = 20, 21, 22, 40 and disparity 9 px under maxD = 9.5 (mb = 1, mbf = maxD: the quotient is exact).  The accepted
    counts differ from one limit to the next, so both the candidate gate and the final comparison decide.  Key points lie at x >= 19, so
    uL < maxD (a negative minU) exists for the limits from 20 up and cannot for 9.5."""
    w, h, n = 480, 360, 600
    p21 = oracle_pair(oracle, "disp21", lambda: stereo_pair(w, h, 5, 21), n)
    p9 = oracle_pair(oracle, "disp9", lambda: stereo_pair(w, h, 4, 9), n)
    limits = (20.0, 21.0, 22.0, 40.0, 9.5)
    acc21 = [int((p21.stereo(m, 1.0)[0] >= 0).sum()) for m in limits]
    acc9 = [int((p9.stereo(m, 1.0)[0] >= 0).sum()) for m in limits]
    assert acc21[0] < 10 and acc21[0] < acc21[1] < acc21[2] < acc21[3] and acc21[2] > 250 and acc21[4] == 0
    assert 100 < acc9[4] < acc9[0] - 50                                                   # 9.5 cuts into the 9 px scene; 20 does not
    for m in limits[:4]:
        assert (p21.kl["x"] < m).any()
    for m in (20.0, 22.0, 9.5):                                                           # what the limit itself rejects, by reason
        why21, why9 = counts(p21.why(m, 1.0)[0]), counts(p9.why(m, 1.0)[0])
        if m != 9.5:
            assert why21["disparity"] > 0
        else:
            assert why9["disparity"] > 0 and why9["no_candidate"] > counts(p9.why(40.0, 1.0)[0])["no_candidate"]
    check(backend, w, h, n, [p21, p9], cameras=[(m, 1.0) for m in limits])


# ------------------------------------------------------------------------------------------------ 4. disparity that varies over the image
GRADIENT = dict(d0=2.0, g=0.1)


def _gradient_pair():
    return warped_pair(480, 360, 21, lambda x, y: GRADIENT["d0"] + GRADIENT["g"] * x)


def _two_plane_pair():
    return warped_pair(480, 360, 22, lambda x, y: np.where(y < 180, 4.0, 30.0))


@pytest.mark.parametrize("scene", ["gradient", "two_planes"])
def test_varying_disparity(backend, oracle, scene):
    """d(x) = 2 + 0.1 x (the right image is the scene compressed by a tenth: patches no longer match under a pure shift), and two planes at 4 and
    30 px.  Accepted disparities span at least 15 px, the prune invalidates at least 5 % of the correlated key points, and the best of the 11
    shifts lies at an end of the band for some key points (bestincR == -L or L, Frame.cc:593).
    The other rejection of the sub-pixel step, deltaR outside [-1, 1] (Frame.cc:602), cannot be reached by any input, so no gradient up to 0.15
    reaches it either (measured: none at 0.05, 0.08, 0.1, 0.12, 0.15 on three scenes): dist2 is the FIRST minimum of the 11 distances and not at
    an end, so a = dist1 - dist2 > 0 and b = dist3 - dist2 >= 0, and deltaR = (a - b) / (2 (a + b)) lies in [-1/2, 1/2].  The distances are
    integers below 2^24, exact in float.  The case asserts that `classify` never names it."""
    w, h, n = 480, 360, 600
    p = oracle_pair(oracle, scene, _gradient_pair if scene == "gradient" else _two_plane_pair, n)
    uo, _ = p.stereo(MBF, MB)
    ok = uo >= 0
    disp = p.kl["x"][ok] - uo[ok]
    assert int(ok.sum()) > 100 and disp.max() - disp.min() >= 15
    why = counts(p.why(MBF, MB)[0])
    assert why["pruned"] >= 0.05 * (why["pruned"] + why["accepted"])
    assert why["end_of_band"] >= 1 and why["delta"] == 0
    check(backend, w, h, n, [p])


# ------------------------------------------------------------------------------------------------ 5. very few accepted matches
# accepted correlations before the prune -> (seed, disparity, window).  At disparity 0 the sub-pixel step lands on either side of uL, and the negative
# side is rejected (disparity >= 0): that is what brings a patch's eight key points down to none, one and two.
FEW = {0: (36, 0, 150, 110, 170, 130), 1: (30, 0, 150, 110, 162, 122), 2: (31, 0, 150, 110, 162, 122), 3: (31, 0, 150, 110, 158, 118),
       7: (30, 7, 150, 110, 174, 134), 8: (30, 7, 150, 110, 170, 130)}
PRUNED = {0: 0, 1: 0, 2: 0, 3: 1, 7: 2, 8: 1}      # ... of which the prune removes


def _few_pair(k):
    seed, disp, x0, y0, x1, y1 = FEW[k]
    return windowed_pair(400, 300, seed, disp, x0, y0, x1, y1)


def test_few_matches(backend, oracle):
    """Flat 400x300 frames with one textured patch each, sized so that exactly 0, 1, 2, 3, 7 and 8 correlations are accepted before the prune (which
    then removes 1 of the 3, 2 of the 7 and 1 of the 8): the median's index k = n/2 for n = 1, 2, odd and even, a frame with key points and no
    match beside them, all as the slots of one batch."""
    w, h, n = 400, 300, 400
    pairs = []
    for k in FEW:
        p = oracle_pair(oracle, ("few", k), lambda k=k: _few_pair(k), n)
        why = counts(p.why(MBF, MB)[0])
        assert why["accepted"] + why["pruned"] == k and why["pruned"] == PRUNED[k], (k, why)
        assert len(p.kl) > 0 and len(p.kr) > 0
        pairs.append(p)
    check(backend, w, h, n, pairs)
