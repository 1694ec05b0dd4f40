"""The blurred planes are stored as 32-column x 4-row tiles (orbhip_blur_tile_addr): every blur kernel writes them through that address
function, k_describe stages its 37 x 37 windows from them one tile row per LDS-DMA pass, and orbhip_debug_blurred_level puts them back
into rows.  Everything here is compared bit for bit with the oracle.

* every writer: one frame (k_blur_mfma's tile, launched with the quadtree), nine frames (k_blur_strip), ORBHIP_BLUR=valu (k_blur) and both
  GaussianBlur rounding modes, on level-0 sizes with w % 32 in {0, 1, 31} and h % 4 in {0, 1, 3} (the scaled levels bring other residues):
  every byte of every level, the last columns and rows of partly filled tiles included;
* window alignments: frames of isolated corner blobs on a lattice whose pitches (37 x 13 px) are coprime with the tile (32 x 4), so that the
  key points of the eight levels meet every alignment of a window against the tiles - asserted on the oracle's key points before anything is
  compared: (cx - 18) % 32 in {0, 27} (a span of two tile columns at its two ends), {28, 31} (the span of three), every (cy - 18) % 4, and
  above level 0 a key point on the last column and one on the last row that the reference can detect (w - 20, h - 20: its window ends one pixel
  inside the plane, in a tile that the image fills only partly); both fp_contract modes; one frame, and two groups of nine frames on two
  streams (the second at frame offset 9);
* level boundaries: a wave whose four key point slots lie on two levels, and a level whose key points end inside a wave (fewer key points
  than the wave has slots), asserted from the oracle's counts per level.

backend = "emu" (kernel sources under the test-only fiber emulation, CPU) or "gpu" (real liborbhip.so, marked gpu).
"""
import numpy as np
import pytest

import orb_slam2_amd
from orb_slam2_amd import synth

LEVELS = 8
NFEAT = 400
SHAPES = [(352, 249), (353, 251), (351, 252)]          # w % 32 = 0, 1, 31; h % 4 = 1, 3, 0
LW, LH = 353, 251                                      # the lattice frames
PX, PY = 37, 13                                        # lattice pitches: coprime with 32 and with 4
_ref_cache = {}


def test_shapes_are_the_residues_asked_for():
    assert {w % 32 for w, h in SHAPES} == {0, 1, 31} and {h % 4 for w, h in SHAPES} == {0, 1, 3}
    assert np.gcd(PX, 32) == 1 and np.gcd(PY, 4) == 1


def lattice_frame(seed):
    """3 x 3 blobs with a brighter centre (one strict maximum of the FAST score each) every 13 rows and 37 columns, the columns of each row
    shifted against the row above, brightness varied so that the quadtree has something to choose from"""
    img = np.full((LH, LW), 40, np.uint8)
    k = 0
    for j, y in enumerate(range(4 + seed % 5, LH - 3, PY)):
        for x in range(3 + (seed * 3 + j * 11) % PX, LW - 3, PX):
            k += 1
            v = 110 + ((k * 2654435761 + seed * 97) >> 7) % 100
            img[y:y + 3, x:x + 3] = v
            img[y + 1, x + 1] = v + 40
    return img


def _oracle_frame(oracle, img, mode, fp):
    ora = oracle.OracleExtractor(NFEAT, 1.2, LEVELS, 20, 7, fast=True, blur_round_mode=mode, fp_contract=fp)
    ko, do = ora.extract(img)
    pyr = [ora.level(l) for l in range(LEVELS)]
    blur = [ora.blurred(l) for l in range(LEVELS)]
    # (a level without key points is never blurred by the reference's operator(); the kernels blur every level: the oracle's GaussianBlur of that level)
    blur = [oracle.blur(pyr[l], mode) if blur[l] is None else blur[l] for l in range(LEVELS)]
    sizes = [ora.level_size(l) for l in range(LEVELS)]
    sf = ora.params()["scale_factors"]
    for a in [ko, do] + blur:
        a.setflags(write=False)
    return dict(kp=ko, desc=do, blur=blur, sizes=sizes, sf=sf)


def _synth_reference(oracle, w, h, mode, frames):
    key = ("synth", w, h, mode)
    if key not in _ref_cache:
        imgs = np.stack([synth.frame(w, h, seed=3 * w + h + 11 * s) for s in range(9)])
        imgs.setflags(write=False)
        _ref_cache[key] = (imgs, {f: _oracle_frame(oracle, imgs[f], mode, 0) for f in (0, 8)})
    imgs, ref = _ref_cache[key]
    return imgs, {f: ref[f] for f in frames}


def _lattice_reference(oracle, fp):
    key = ("lattice", fp)
    if key not in _ref_cache:
        imgs = np.stack([lattice_frame(1 + s) for s in range(9)])
        imgs.setflags(write=False)
        _ref_cache[key] = (imgs, [_oracle_frame(oracle, imgs[s], 0, fp) for s in range(9)])
    return _ref_cache[key]


def _check_planes(ex, ref, frame, what):
    for l in range(LEVELS):
        want = ref["blur"][l]
        got = ex.blurred_level(l, frame=frame)
        assert got.shape == want.shape == ref["sizes"][l][::-1]
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"{what}: blurred level {l} ({want.shape[1]}x{want.shape[0]}) of frame {frame}: {len(bad)} bytes differ, first at (y, x) = {tuple(bad[0])}"


def _check_keys(kps, desc, ref, what):
    ko, do = ref["kp"], ref["desc"]
    assert len(kps) == len(ko), f"{what}: {len(kps)} key points, the oracle {len(ko)}"
    for name in ko.dtype.names:
        bad = np.flatnonzero(kps[name].view(np.int32) != ko[name].view(np.int32))
        assert len(bad) == 0, f"{what}: key point field {name}: {len(bad)} differ, first at index {bad[0]}"
    bad = np.argwhere(desc != do)
    assert len(bad) == 0, f"{what}: descriptors: {len(bad)} bytes differ, first at (key point, byte) = {tuple(bad[0])}"


# ---------------------------------------------------------------------------------------------------------------- every writer
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("writer", ["mfma_one_frame", "strip_nine_frames", "valu_one_frame"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_every_writer_stores_through_the_tiles(backend, oracle, monkeypatch, w, h, writer, mode):
    if writer.startswith("valu"):
        monkeypatch.setenv("ORBHIP_BLUR", "valu")
    else:
        monkeypatch.delenv("ORBHIP_BLUR", raising=False)
    B = 9 if writer.endswith("nine_frames") else 1
    frames = (0, 8) if B == 9 else (0,)
    imgs, ref = _synth_reference(oracle, w, h, mode, frames)
    ex = orb_slam2_amd.ORBextractor(NFEAT, 1.2, LEVELS, 20, 7, w, h, max_batch=B, library=backend, blur_round_mode=mode)
    try:
        kps, descs = ex.extract_batch(imgs[:B])
        for f in frames:
            what = f"{writer}, {w}x{h}, rounding mode {mode}"
            # levels whose width is no multiple of 32 / height no multiple of 4 end in partly filled tiles: their last columns and rows are compared like every other byte
            assert any(sw % 32 and sh % 4 for sw, sh in ref[f]["sizes"])
            _check_planes(ex, ref[f], f, what)
            _check_keys(kps[f], descs[f], ref[f], f"{what}, frame {f}")
    finally:
        ex.close()


# ---------------------------------------------------------------------------------------------------------------- window alignments
def _level_coordinates(ref):
    """the key points' integer coordinates on their own level (pt = level coordinates * scale, ORBextractor.cc:1095-1101)"""
    ko = ref["kp"]
    s = ref["sf"][ko["octave"]]
    cx, cy = np.rint(ko["x"] / s).astype(int), np.rint(ko["y"] / s).astype(int)
    assert np.array_equal((cx * s).astype(np.float32).view(np.int32), ko["x"].view(np.int32)) and np.array_equal((cy * s).astype(np.float32).view(np.int32), ko["y"].view(np.int32))
    return ko["octave"].astype(int), cx, cy


def _assert_alignment_coverage(refs):
    ax, ay, right, bottom = set(), set(), False, False
    for ref in refs:
        lv, cx, cy = _level_coordinates(ref)
        w = np.array([ref["sizes"][l][0] for l in lv]); h = np.array([ref["sizes"][l][1] for l in lv])
        assert np.all(cx >= 18) and np.all(cy >= 18) and np.all(cx + 18 < w) and np.all(cy + 18 < h)
        ax |= set(((cx - 18) % 32).tolist()); ay |= set(((cy - 18) % 4).tolist())
        right = right or bool(np.any((lv > 0) & (w - cx <= 20)))
        bottom = bottom or bool(np.any((lv > 0) & (h - cy <= 20)))
    assert {0, 27, 28, 31} <= ax, f"window column alignments met: {sorted(ax)}"
    assert ay == {0, 1, 2, 3}, f"window row alignments met: {sorted(ay)}"
    assert right, "no key point within 20 px of the right border above level 0"
    assert bottom, "no key point within 20 px of the bottom border above level 0"


@pytest.mark.parametrize("fp", [0, 1])
def test_lattice_meets_every_window_alignment(oracle, fp):
    """the coverage the two tests below rely on, from the oracle alone: of the single frame, and of the frames compared in the batch"""
    imgs, refs = _lattice_reference(oracle, fp)
    _assert_alignment_coverage(refs[:1])
    _assert_alignment_coverage(refs)


@pytest.mark.parametrize("fp", [0, 1])
def test_window_alignments_one_frame(backend, oracle, fp):
    imgs, refs = _lattice_reference(oracle, fp)
    _assert_alignment_coverage(refs[:1])
    ex = orb_slam2_amd.ORBextractor(NFEAT, 1.2, LEVELS, 20, 7, LW, LH, library=backend)
    try:
        ex.SetFpContract(fp)
        k, d = ex(imgs[0])
        _check_keys(k, d, refs[0], f"lattice frame, fp_contract {fp}")
        _check_planes(ex, refs[0], 0, f"lattice frame, fp_contract {fp}")
    finally:
        ex.close()


@pytest.mark.parametrize("fp", [0, 1])
def test_window_alignments_nine_frames_at_a_frame_offset(backend, oracle, fp):
    """eighteen resident frames on two streams: two groups of nine (k_blur_strip and k_describe over nine frames each), the second at frame offset 9"""
    B, PITCH = 18, 384
    imgs, refs = _lattice_reference(oracle, fp)
    _assert_alignment_coverage(refs)
    host = np.zeros((B, LH, PITCH), np.uint8)
    host[:, :, :LW] = imgs[np.arange(B) % 9]
    ex = orb_slam2_amd.ORBextractor(NFEAT, 1.2, LEVELS, 20, 7, LW, LH, max_batch=B, library=backend, num_streams=2)
    dbuf = orb_slam2_amd.DeviceBuffer.from_array(host, library=backend)
    try:
        ex.SetFpContract(fp)
        ex.extract_device(dbuf.ptr, B, LH * PITCH, PITCH)
        kps, descs = ex.fetch(B)
        for s in range(B):
            _check_keys(kps[s], descs[s], refs[s % 9], f"slot {s}, fp_contract {fp}")
        for s in (0, 8, 9, 17):
            _check_planes(ex, refs[s % 9], s, f"slot {s}")
    finally:
        ex.close()
        dbuf.free()


# ---------------------------------------------------------------------------------------------------------------- level boundaries
def test_waves_across_level_boundaries(backend, oracle):
    """k_describe gives a wave four consecutive key point slots; level l owns max(nfeatures of the level + 3, 4 x quadtree roots) of them, its key
    points the first of those.  Asserted from the oracle's counts: some level's slots start inside a wave, so that wave's slots lie on two levels
    (and the later level has key points in it), and some level's key points end inside a wave - fewer key points than the wave has slots."""
    imgs, refs = _lattice_reference(oracle, 0)
    ref = refs[0]
    ex = orb_slam2_amd.ORBextractor(NFEAT, 1.2, LEVELS, 20, 7, LW, LH, library=backend)
    try:
        nfeat = ex.features_per_level()
        n = np.bincount(ref["kp"]["octave"], minlength=LEVELS)
        cap = [max(int(nfeat[l]) + 3, 4 * int(np.floor((ref["sizes"][l][0] - 32) / (ref["sizes"][l][1] - 32) + 0.5))) for l in range(LEVELS)]
        off = np.concatenate([[0], np.cumsum(cap)])[:LEVELS]
        assert ex.capacity == int(np.sum(cap)), (ex.capacity, cap)           # the slots are what this test takes them for
        assert any(off[l] % 4 and n[l] > 0 for l in range(1, LEVELS)), (off, n)
        assert any(0 < n[l] < cap[l] and n[l] % 4 for l in range(LEVELS)), (n, cap)
        k, d = ex(imgs[0])
        _check_keys(k, d, ref, "lattice frame")
    finally:
        ex.close()
