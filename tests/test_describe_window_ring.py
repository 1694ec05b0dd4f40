"""k_describe keeps a ring of window buffers per wave: the blurred windows of a wave's first RING key point slots are requested at its start, and
when slot k's BRIEF reads have returned the window of slot k + RING is requested into the buffer slot k used.  Every wait is a counted
s_waitcnt; the counts are static because an invalid slot requests what the wave's first valid slot requests.  Everything here is compared bit
for bit with the oracle.

* validity patterns of a wave's four slots, asserted from the oracle's counts per level and the level offsets before anything is compared: all
  four valid; valid then invalid to the end (a level ends inside the wave); invalid then valid (the next level starts inside the wave); a hole
  between valid slots (an under-filled level followed by the next level in the same wave); a single valid slot in each of the four positions;
  waves that never refill (one valid slot, exactly RING valid slots);
* window alignment on a refilled slot: a window of three tile columns ((cx - 18) % 32 > 27) on slot 2 or 3, and a window of two tile columns
  refilled into the buffer that a window of three used before it;
* both fp_contract modes; one frame, nine frames, two groups of nine on two streams (the second at frame offset 9);
* ring depths 2 (what launches of more than eight frames take), 3 and 4 (every window up front, no refill: what launches of up to eight frames
  take): the library holds all three and ORBHIP_TEST_DESCRIBE_RING, read at every launch, chooses - so every depth runs at every frame count,
  in the same binary that is benchmarked, where a build define would test another one;
* the emulation cases start every workgroup on garbage LDS (HIPEMU_POISON_LDS).

The emulation performs an LDS-DMA at once, so it checks which buffer a slot reads and what an invalid slot requests, not the timing of the ring;
the device cases run the real requests.  (At size: bench.py --full compares 64 slots of 512 frames with the oracle.)

backend = "emu" (kernel sources under the test-only fiber emulation, CPU) or "gpu" (real liborbhip.so, marked gpu).
"""
import numpy as np
import pytest

import orb_slam2_amd

from test_blur_tiled_layout import LH, LW, lattice_frame

LEVELS = 8
RINGS = [2, 3, 4]
NFEAT_LATTICE, NFEAT_LONE = 342, 50
_ref_cache = {}


def lone_blob_frame():
    """one blob on a flat background: one key point on every level, so every level's first slot is the only valid one of its wave"""
    img = np.full((LH, LW), 40, np.uint8)
    img[113:116, 157:160] = 151
    img[114, 158] = 200
    return img


def _frame(name):
    return lone_blob_frame() if name == "lone" else lattice_frame(int(name[len("lattice"):]))


def _nfeat(name):
    return NFEAT_LONE if name == "lone" else NFEAT_LATTICE


def _reference(oracle, name, fp):
    key = (name, fp)
    if key not in _ref_cache:
        img = _frame(name)
        ora = oracle.OracleExtractor(_nfeat(name), 1.2, LEVELS, 20, 7, fast=True, blur_round_mode=0, fp_contract=fp)
        ko, do = ora.extract(img)
        for a in (img, ko, do):
            a.setflags(write=False)
        p = ora.params()
        _ref_cache[key] = dict(img=img, kp=ko, desc=do, sizes=[ora.level_size(l) for l in range(LEVELS)], sf=p["scale_factors"], fpl=[int(v) for v in p["features_per_level"]])
    return _ref_cache[key]


def _slot_capacity(ref):
    """level l owns max(nfeatures of the level + 3, 4 x quadtree roots) key point slots"""
    return [max(ref["fpl"][l] + 3, 4 * int(np.floor((ref["sizes"][l][0] - 32) / (ref["sizes"][l][1] - 32) + 0.5))) for l in range(LEVELS)]


def _waves(ref):
    """(valid, three) per wave and slot: a level's key points take the first of its slots in output order; a wave takes four consecutive slots"""
    ko = ref["kp"]
    lv = ko["octave"].astype(int)
    cx = np.rint(ko["x"] / ref["sf"][lv]).astype(int)
    assert np.array_equal((cx * ref["sf"][lv]).astype(np.float32).view(np.int32), ko["x"].view(np.int32))
    assert np.all(np.diff(lv) >= 0)                                   # level-major output
    cap = _slot_capacity(ref)
    off = np.concatenate([[0], np.cumsum(cap)])
    n = np.bincount(lv, minlength=LEVELS)
    assert np.all(n <= cap)
    first = np.concatenate([[0], np.cumsum(n)])
    slots = (int(off[-1]) + 3) // 4 * 4
    valid, three = np.zeros(slots, bool), np.zeros(slots, bool)
    slot = off[lv] + np.arange(len(ko)) - first[lv]
    valid[slot] = True
    three[slot] = (cx - 18) % 32 > 27
    return valid.reshape(-1, 4), three.reshape(-1, 4)


def _patterns(ref):
    valid, _ = _waves(ref)
    return {"".join("V" if v else "I" for v in w) for w in valid if w.any()}


def _assert_pattern_coverage(refs):
    pats = set().union(*[_patterns(r) for r in refs])
    assert "VVVV" in pats, pats
    assert pats & {"VIII", "VVII", "VVVI"}, f"no level ends inside a wave: {sorted(pats)}"
    assert pats & {"IVVV", "IIVV", "IIIV"}, f"no level starts inside a wave behind invalid slots: {sorted(pats)}"
    assert pats & {"VIVV", "VIIV", "VVIV"}, f"no hole between valid slots: {sorted(pats)}"
    assert {"VIII", "IVII", "IIVI", "IIIV"} <= pats, f"single valid slot: {sorted(pats)}"
    assert {"VVII", "VVVI"} <= pats, f"waves with exactly two and exactly three valid slots from slot 0 on (no refill that is used): {sorted(pats)}"


def _assert_alignment_coverage(refs, ring):
    on_refilled = three_then_two = False
    for ref in refs:
        valid, three = _waves(ref)
        on_refilled = on_refilled or bool(np.any(valid[:, ring:] & three[:, ring:]))
        for j in range(4 - ring):
            three_then_two = three_then_two or bool(np.any(valid[:, j] & three[:, j] & valid[:, j + ring] & ~three[:, j + ring]))
    assert on_refilled, f"no three-column window on a refilled slot at depth {ring}"
    assert three_then_two, f"no two-column window refilled into a three-column window's buffer at depth {ring}"


def test_inputs_meet_every_pattern(oracle):
    """the coverage the tests below rely on, from the oracle alone"""
    one = [_reference(oracle, "lattice5", 0), _reference(oracle, "lone", 0)]
    _assert_pattern_coverage(one)
    assert _patterns(one[1]) >= {"VIII", "IVII", "IIVI"}
    assert {"VVVV", "IIIV", "VVII", "VVVI"} <= _patterns(one[0])
    for ring in (2, 3):
        _assert_alignment_coverage(one[:1], ring)
        _assert_alignment_coverage([_reference(oracle, f"lattice{s}", 0) for s in range(1, 10)], ring)


def _check_keys(kps, desc, ref, what):
    ko, do = ref["kp"], ref["desc"]
    assert len(kps) == len(ko), f"{what}: {len(kps)} key points, the oracle {len(ko)}"
    for name in ko.dtype.names:
        bad = np.flatnonzero(kps[name].view(np.int32) != ko[name].view(np.int32))
        assert len(bad) == 0, f"{what}: key point field {name}: {len(bad)} differ, first at index {bad[0]}"
    bad = np.argwhere(desc != do)
    assert len(bad) == 0, f"{what}: descriptors: {len(bad)} bytes differ, first at (key point, byte) = {tuple(bad[0])}"


@pytest.fixture
def ring_env(backend, monkeypatch):
    def set_(ring):
        monkeypatch.setenv("ORBHIP_TEST_DESCRIBE_RING", str(ring))
        if backend.endswith("emu.so"):
            monkeypatch.setenv("HIPEMU_POISON_LDS", "1")
    return set_


@pytest.mark.parametrize("fp", [0, 1])
@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("name", ["lattice5", "lone"])
def test_validity_patterns_one_frame(backend, oracle, ring_env, name, ring, fp):
    ref = _reference(oracle, name, fp)
    _assert_pattern_coverage([_reference(oracle, "lattice5", fp), _reference(oracle, "lone", fp)])
    if name == "lattice5" and ring < 4:
        _assert_alignment_coverage([ref], ring)
    ring_env(ring)
    ex = orb_slam2_amd.ORBextractor(_nfeat(name), 1.2, LEVELS, 20, 7, LW, LH, library=backend)
    try:
        assert ex.capacity == int(np.sum(_slot_capacity(ref))), (ex.capacity, _slot_capacity(ref))       # the slots are what this test takes them for
        ex.SetFpContract(fp)
        k, d = ex(ref["img"])
        _check_keys(k, d, ref, f"{name}, depth {ring}, fp_contract {fp}")
    finally:
        ex.close()


@pytest.mark.parametrize("fp", [0, 1])
@pytest.mark.parametrize("ring", RINGS)
def test_nine_frames(backend, oracle, ring_env, ring, fp):
    refs = [_reference(oracle, f"lattice{s}", fp) for s in range(1, 10)]
    if ring < 4:
        _assert_alignment_coverage(refs, ring)
    ring_env(ring)
    ex = orb_slam2_amd.ORBextractor(NFEAT_LATTICE, 1.2, LEVELS, 20, 7, LW, LH, max_batch=9, library=backend)
    try:
        ex.SetFpContract(fp)
        kps, descs = ex.extract_batch(np.stack([r["img"] for r in refs]))
        for s in range(9):
            _check_keys(kps[s], descs[s], refs[s], f"frame {s}, depth {ring}, fp_contract {fp}")
    finally:
        ex.close()


@pytest.mark.parametrize("fp", [0, 1])
@pytest.mark.parametrize("ring", RINGS)
def test_two_groups_of_nine_on_two_streams(backend, oracle, ring_env, ring, fp):
    """eighteen resident frames: two launches of nine frames each, the second at frame offset 9"""
    B, PITCH = 18, 384
    refs = [_reference(oracle, f"lattice{s}", fp) for s in range(1, 10)]
    host = np.zeros((B, LH, PITCH), np.uint8)
    host[:, :, :LW] = np.stack([refs[s % 9]["img"] for s in range(B)])
    ring_env(ring)
    ex = orb_slam2_amd.ORBextractor(NFEAT_LATTICE, 1.2, LEVELS, 20, 7, LW, LH, max_batch=B, library=backend, num_streams=2)
    dbuf = orb_slam2_amd.DeviceBuffer.from_array(host, library=backend)
    try:
        ex.SetFpContract(fp)
        ex.extract_device(dbuf.ptr, B, LH * PITCH, PITCH)
        kps, descs = ex.fetch(B)
        for s in range(B):
            _check_keys(kps[s], descs[s], refs[s % 9], f"slot {s}, depth {ring}, fp_contract {fp}")
    finally:
        ex.close()
        dbuf.free()
