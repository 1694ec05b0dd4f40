"""Batches above sixteen frames and non-zero frame offsets produce the oracle's bytes in EVERY camera slot.

The other batch tests stop at 12 frames and look at two to four of them.  Here the batch sizes are the ones at which the launch code takes another
path: runs of four pyramid tiles per workgroup (from 384 frames on, with the ragged runs of 3, 2 and 1 tiles behind full ones), several groups of
eight frames plus a ragged one in xcd_frame_map, per-stream groups and default host chunks of more than eight frames that start at a frame offset
(P.frame0 != 0 in k_blur_strip, k_pyramid_level_g, k_fast_cells, the quadtree, k_describe, the key point undistortion) and groups of up to eight
frames at an offset (k_pyramid_cascade, the fused blur-quadtree launch).

Slots: a batch of B slots is filled from S = 61 scenes, slot s <- scene s % 61.  61 is coprime with the eight-slot grouping of xcd_frame_map and
with every chunk and group size below, so a workgroup that serves the wrong slot always lands on another image.  The oracle extracts each scene once
per (shape, rounding mode, levels, time step); nothing else is a checker and everything is compared bit for bit: count, every key point field and
the descriptors of every slot; the pyramid and the blurred planes of a fixed set of slots (_plane_slots).

Two things the entry points decide:
  * the tiles per workgroup of k_pyramid_level_g follow the frames of ONE launch, and the host-buffer path cuts a batch into chunks of at most 128
    frames: only the device-resident entry (extract_device, one stream) launches 384 frames at once.  Cases 1 and 2 therefore go through it;
  * level 0 of a device-resident call is the caller's own buffer (orbhip_pyramid_level refuses it): those cases compare pyramid levels 1 .. L-1,
    the host-buffer cases every level.  The blurred planes are compared on every level everywhere.
The pipeline matcher's prev_matched array stays in device memory - no entry point downloads it - so the stream-group cases compare the match count
and matches12 of every slot; by ORBmatcher.cc:478-481 prev_matched is those matches applied to key points that have just been compared.

backend = "emu" (kernel sources under the test-only fiber emulation, CPU) or "gpu" (real liborbhip.so, marked gpu).
"""
import contextlib

import numpy as np
import pytest

import orb_slam2_amd
from orb_slam2_amd import synth

S = 61                                    # distinct scenes
W, H, NFEAT, LEVELS = 320, 221, 300, 8      # the smallest height at which eight levels meet the conditions test_pyramid_runs_of_four_tiles asserts (level 7 is 89 x 62, the smallest supported)
PITCH = 352                               # row pitch of the device-resident frames (not the width)
SEED = 500
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314)      # Examples/Monocular/TUM1.yaml
CAM = (TUM1[0] * W / 640.0, TUM1[1] * H / 480.0, TUM1[2] * W / 640.0, TUM1[3] * H / 480.0) + TUM1[4:]
_ref_cache = {}


def _reference(oracle, mode, t=0):
    """frame t of the 61 scenes and what the oracle makes of each: (key points, descriptors, pyramid levels, blurred levels); computed once per
    (rounding mode, time step), never modified"""
    key = (W, H, mode, LEVELS, t)
    if key not in _ref_cache:
        ora = oracle.OracleExtractor(NFEAT, 1.2, LEVELS, 20, 7, fast=True, blur_round_mode=mode)       # the -O3 build of the same source: same bytes (test_oracle_kat.py)
        imgs = np.stack([synth.frame(W, H, seed=SEED + s, t=t) for s in range(S)])
        imgs.setflags(write=False)
        ref = []
        for s in range(S):
            ko, do = ora.extract(imgs[s])
            pyr = [ora.level(l) for l in range(LEVELS)]
            blur = [ora.blurred(l) for l in range(LEVELS)]
            # (a level without key points is never blurred by the reference's operator(); the kernels blur every level: the oracle's GaussianBlur of that level)
            blur = [oracle.blur(pyr[l], mode) if blur[l] is None else blur[l] for l in range(LEVELS)]
            for a in [ko, do] + pyr + blur:
                a.setflags(write=False)
            ref.append((ko, do, pyr, blur))
        assert np.array_equal(pyr[0], imgs[S - 1])
        _ref_cache[key] = (imgs, ref)
    return _ref_cache[key]


def _plane_slots(B, parts=()):
    """slots whose planes are compared: 0, 7, 8, the last full group's first and last slot, every slot of the ragged last group, B - 1, every 37th
    slot, and the first and last slot of each group or chunk [f0, f1) of `parts`"""
    full = B // 8
    s = {0, 7, 8, B - 1} | set(range(full * 8, B)) | set(range(0, B, 37))
    if full:
        s |= {(full - 1) * 8, (full - 1) * 8 + 7}
    for f0, f1 in parts:
        s |= {f0, f1 - 1}
    return sorted(x for x in s if 0 <= x < B)


def _check_slots(kps, descs, ref, B, what):
    assert len(kps) == B and len(descs) == B
    for s in range(B):
        ko, do = ref[s % S][:2]
        assert len(kps[s]) == len(ko), f"{what}: slot {s} (scene {s % S}) has {len(kps[s])} key points, the oracle {len(ko)}"
        for name in ko.dtype.names:
            bad = np.flatnonzero(kps[s][name].view(np.int32) != ko[name].view(np.int32))
            assert len(bad) == 0, f"{what}: slot {s} (scene {s % S}), key point field {name}: {len(bad)} differ, first at index {bad[0]}"
        bad = np.argwhere(descs[s] != do)
        assert len(bad) == 0, f"{what}: slot {s} (scene {s % S}), descriptors: {len(bad)} bytes differ, first at (key point, byte) = {tuple(bad[0])}"


def _check_planes(ex, ref, slots, first_level, what):
    for s in slots:
        pyr, blur = ref[s % S][2:]
        for name, fetch, want, l0 in (("pyramid", ex.mvImagePyramid, pyr, first_level), ("blurred", ex.blurred_level, blur, 0)):
            for l in range(l0, LEVELS):
                got = fetch(l, frame=s)
                assert got.shape == want[l].shape
                bad = np.argwhere(got != want[l])
                assert len(bad) == 0, f"{what}: {name} level {l} of slot {s} (scene {s % S}): {len(bad)} bytes differ, first at (y, x) = {tuple(bad[0])}"


def _resident(backend, imgs, B):
    """slots 0 .. B-1 (slot s <- scene s % 61) as one device buffer of PITCH-byte rows"""
    host = np.zeros((B, H, PITCH), np.uint8)
    host[:, :, :W] = imgs[np.arange(B) % S]
    return orb_slam2_amd.DeviceBuffer.from_array(host, library=backend)


def _device_batch(backend, oracle, B, mode):
    """one extract_device call of B resident frames on one stream: every launch covers all B frames"""
    imgs, ref = _reference(oracle, mode)
    ex = orb_slam2_amd.ORBextractor(NFEAT, 1.2, LEVELS, 20, 7, W, H, max_batch=B, library=backend, blur_round_mode=mode)
    dbuf = _resident(backend, imgs, B)
    try:
        ex.extract_device(dbuf.ptr, B, H * PITCH, PITCH)
        kps, descs = ex.fetch(B)
        what = f"B = {B}, mode {mode}"
        _check_slots(kps, descs, ref, B, what)
        _check_planes(ex, ref, _plane_slots(B), 1, what)
    finally:
        ex.close()
        dbuf.free()


def test_pyramid_runs_of_four_tiles(backend, oracle):
    """387 frames = 48 groups of eight plus three: k_pyramid_level_g takes four tiles per workgroup, the third step staging into the buffer the first
    one computed from; the levels of this shape end in runs of 3, 1 and 2 tiles behind full ones (and in full runs only)."""
    B = 387
    ex = orb_slam2_amd.ORBextractor(NFEAT, 1.2, LEVELS, 20, 7, W, H, library=backend)
    size = [ex.level_size(l) for l in range(LEVELS)]
    ex.close()
    TW, TH = 256, 16                                               # PYR_TW x PYR_TH, the output tile of k_pyramid_level_g
    gy = [-(-size[l][1] // TH) for l in range(1, LEVELS)]         # tile rows of levels 1 .. 7
    assert {g % 4 for g in gy} == {0, 1, 2, 3}, gy                # a last run of every length
    for r in (1, 2, 3):
        assert any(g % 4 == r and g >= 5 for g in gy), (r, gy)    # ... behind at least one full run
    assert size[1][0] > TW                                         # two tile columns on level 1
    _device_batch(backend, oracle, B, 1)


@pytest.mark.parametrize("B", [17, 40, 383, 384])
def test_batch_sizes_at_the_switches(backend, oracle, B):
    """three groups of eight with a ragged one; five full groups; the last size with two tiles per workgroup; the first with four, on a multiple of eight"""
    _device_batch(backend, oracle, B, 0)


@pytest.mark.parametrize("B,num_streams,distorted", [(20, 2, False), (16, 2, False), (19, 3, False), (27, 2, True)])
def test_stream_groups_with_frame_offsets(backend, oracle, B, num_streams, distorted):
    """run_pipeline cuts the batch into one group of frames per stream: 10 + 10 (the strip blur and k_pyramid_level_g at frame0 = 10, the blur on the
    group's own stream), 8 + 8 (the cascade and the fused blur-quadtree at frame0 = 8), 6 + 6 + 7 (the fewer-than-eight map at an offset), 13 + 14
    (two ragged groups; this one with a distorted camera: mvKeysUn of every slot).  Two calls on consecutive frames of each scene, the second matched
    against the first: SearchForInitialization of every slot (one wavefront per slot in the matcher's kernels)."""
    parts = [(B * g // num_streams, B * (g + 1) // num_streams) for g in range(num_streams)]       # run_pipeline's groups (for the reader; not asserted against the product)
    ref = [_reference(oracle, 0, t) for t in (0, 1)]
    bounds = oracle.image_bounds(CAM, W, H) if distorted else None
    ex = orb_slam2_amd.ORBextractor(NFEAT, 1.2, LEVELS, 20, 7, W, H, max_batch=B, library=backend, num_streams=num_streams)
    bufs = []
    try:
        if distorted:
            ex.set_camera(CAM)
            assert ex.bounds().tobytes() == bounds.tobytes()
        for t in (0, 1):
            what = f"B = {B} on {num_streams} streams, call {t}"
            ex.sync()
            bufs.append(_resident(backend, ref[t][0], B))
            ex.extract_device(bufs[-1].ptr, B, H * PITCH, PITCH, match_prev=(t > 0), window=100, nnratio=0.9, check_ori=True)
            kps, descs = ex.fetch(B)
            _check_slots(kps, descs, ref[t][1], B, what)
            _check_planes(ex, ref[t][1], _plane_slots(B, parts), 1, what)
            if distorted:
                un = ex.fetch_undistorted(B, [len(k) for k in kps])
                for s in range(B):
                    assert un[s].tobytes() == oracle.undistort_keypoints(CAM, ref[t][1][s % S][0]).tobytes(), f"{what}: mvKeysUn of slot {s}"
        m12, nm = ex.fetch_matches(B)
        for s in range(B):
            (k1, d1), (k2, d2) = ref[0][1][s % S][:2], ref[1][1][s % S][:2]
            if distorted:
                k1, k2 = oracle.undistort_keypoints(CAM, k1), oracle.undistort_keypoints(CAM, k2)
            with oracle.image_bounds_set(bounds) if distorted else contextlib.nullcontext():
                n_o, m_o, _ = oracle.search_for_initialization(k1, d1, k2, d2, W, H, window=100, nnratio=0.9)
            assert nm[s] == n_o, f"{what}: slot {s} has {nm[s]} matches, the oracle {n_o}"
            assert np.array_equal(m12[s], m_o), f"{what}: matches12 of slot {s}"
    finally:
        ex.close()
        for b in bufs:
            b.free()


@pytest.mark.parametrize("B,pinned", [(40, False), (40, True), (33, False)])
def test_default_host_chunking(backend, oracle, monkeypatch, B, pinned):
    """The unforced chunk rule of the host-buffer path (host_chunk_frames): pageable frames through extract_batch, pinned frames and pinned named
    result buffers through submit / collect.  Every chunk but the first starts at a frame offset; the last chunk of the pinned case has eight
    frames (the handful-of-frames kernels at frame0 = 32)."""
    monkeypatch.delenv("ORBHIP_HOST_CHUNK", raising=False)
    if pinned and backend.endswith("_emu.so"):
        monkeypatch.setenv("HIPEMU_ALL_PINNED", "1")
    # host_chunk_frames for 32 frames and more (for the reader; not asserted against the product): 40 pageable -> 24 + 16, 40 pinned -> 16 + 16 + 8, 33 pageable -> 24 + 9
    ch = min(max(((B + 3) // 4 + 7) & ~7, 16), 64) if pinned else min(max(((B + 1) // 2 + 7) & ~7, 16), 128)
    parts = [(f0, min(f0 + ch, B)) for f0 in range(0, B, ch)]
    assert len(parts) > 1 and max(f1 - f0 for f0, f1 in parts) > 8
    if B == 40:
        assert any(f1 - f0 <= 8 for f0, f1 in parts) == pinned
    imgs, ref = _reference(oracle, 0)
    ex = orb_slam2_amd.ORBextractor(NFEAT, 1.2, LEVELS, 20, 7, W, H, max_batch=B, library=backend)
    try:
        if pinned:
            src = orb_slam2_amd.pinned_array((B, H, W), np.uint8, library=backend)
            src[:] = imgs[np.arange(B) % S]
            cap = ex.capacity
            out = (orb_slam2_amd.pinned_array((B, cap), orb_slam2_amd.KEYPOINT_DTYPE, library=backend),
                   orb_slam2_amd.pinned_array((B, cap, 32), np.uint8, library=backend), np.zeros(B, np.int32))
            nout = ex.collect(ex.submit(src, out=out))
            kps, descs = [out[0][s, :nout[s]] for s in range(B)], [out[1][s, :nout[s]] for s in range(B)]
        else:
            kps, descs = ex.extract_batch([imgs[s % S] for s in range(B)])
        what = f"B = {B}, {'pinned' if pinned else 'pageable'}, chunks of {ch}"
        _check_slots(kps, descs, ref, B, what)
        _check_planes(ex, ref, _plane_slots(B, parts), 0, what)
    finally:
        ex.close()
