"""The batched matrix-core blur (k_blur_strip: more than eight frames, a workgroup blurs a run of vertically adjacent tiles with the next tile's
rows in flight) produces the oracle's bytes on every level.

The single-image tests go through k_blur_quadtree and never reach this kernel, so everything here is a batch of nine frames - the smallest one
that takes the batched path - through extract_batch: the border shapes of the 224-column tiles (w % 4 = 0..3, a strip one block wide, a strip
that ends exactly at the border; top levels with fewer tile rows than a run holds, level 0 with 9-10 tile rows), both GaussianBlur rounding
modes, the serial schedule, and a height of 13 tile rows, which leaves a single tile in the last run of every level-0 strip for runs of 2, 3
and 4 tiles alike (the step that has no tile to prefetch then follows one that prefetched).
Everything above eleven frames - every slot of a batch, frame offsets, the larger run lengths of the pyramid - is in tests/test_large_batches.py.

backend = "emu" (kernel sources under the test-only fiber emulation, CPU) or "gpu" (real liborbhip.so, marked gpu).
"""
import numpy as np
import pytest

import orb_slam2_amd
from orb_slam2_amd import synth

B = 9
NFEAT = 600
FRAMES = (0, 8)
_ref_cache = {}


def _reference(oracle, w, h, mode):
    """the nine frames of a shape and the oracle's results for frames 0 and 8 (computed once per shape and rounding mode, never modified)"""
    key = (w, h, mode)
    if key not in _ref_cache:
        imgs = np.stack([synth.frame(w, h, seed=w + h + 7 * s) for s in range(B)])
        imgs.setflags(write=False)
        ref = {}
        for f in FRAMES:
            ora = oracle.OracleExtractor(NFEAT, 1.2, 8, 20, 7, blur_round_mode=mode)
            ko, do = ora.extract(imgs[f])
            planes = [ora.blurred(l) for l in range(8)]
            assert all(p is not None for p in planes), f"the oracle has no blurred plane for a level of {w}x{h}"
            ref[f] = (ko, do, planes)
        _ref_cache[key] = (imgs, ref)
    return _ref_cache[key]


def _check(backend, oracle, w, h, mode):
    imgs, ref = _reference(oracle, w, h, mode)
    ex = orb_slam2_amd.ORBextractor(NFEAT, 1.2, 8, 20, 7, w, h, max_batch=B, library=backend, blur_round_mode=mode)
    try:
        kps, descs = ex.extract_batch(imgs)
        for f in FRAMES:
            ko, do, planes = ref[f]
            for l in range(8):
                got = ex.blurred_level(l, frame=f)
                assert got.shape == planes[l].shape
                bad = np.argwhere(got != planes[l])
                assert len(bad) == 0, f"blurred level {l} of frame {f} ({w}x{h}, mode {mode}): {len(bad)} bytes differ, first at (y, x) = {tuple(bad[0])}"
            assert len(kps[f]) == len(ko), (f, len(kps[f]), len(ko))
            for name in ko.dtype.names:
                assert np.array_equal(kps[f][name].view(np.int32), ko[name].view(np.int32)), (f, name)
            assert np.array_equal(descs[f], do), f
    finally:
        ex.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("w,h", [(224 + 62, 230), (333, 250), (450, 224), (227, 231)])
def test_strip_blur_border_shapes(backend, oracle, mode, w, h):
    _check(backend, oracle, w, h, mode)


def test_strip_blur_serial_schedule(backend, oracle, monkeypatch):
    """ORBHIP_SERIAL=1 keeps the blur on the main stream: the same kernel, launched between FAST and the quadtree"""
    monkeypatch.setenv("ORBHIP_SERIAL", "1")
    _check(backend, oracle, 333, 250, 1)


@pytest.mark.parametrize("mode", [0, 1])
def test_strip_blur_last_run_is_one_tile(backend, oracle, mode):
    w, h = 350, 320
    assert -(-h // 26) == 13          # 13 % 2 == 13 % 3 == 13 % 4 == 1
    _check(backend, oracle, w, h, mode)
