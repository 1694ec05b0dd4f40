"""Frame::ComputeStereoMatches (Frame.cc:466-640) on the device-resident results of a left and a right
extractor: mvuRight / mvDepth bit-identical to the oracle's restatement.
The shapes here stay below 2000 key points and 520 rows, with uniform disparity and a disparity limit far beyond it; the matcher's limits (more than
4096 key points, 1040 rows and more, a limit that binds, varying disparity, a handful of matches) are in tests/test_stereo_limits.py."""
import numpy as np
import pytest

import orb_slam2_amd
from orb_slam2_amd import synth

MBF, MB = 386.1448, 386.1448 / 718.856           # KITTI00-02.yaml: Camera.bf, bf / fx


def stereo_pair(w, h, seed, disp):
    """Left frame + the same scene seen `disp` px further left (uniform disparity) with independent sensor noise."""
    m = 64
    sc = synth.scene(w, h, seed=seed)
    left = synth.frame_from_scene(sc, w, h, t=0, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    right = np.clip(np.rint(sc[m // 2:m // 2 + h, m // 2 + disp:m // 2 + disp + w]) + rng.integers(-6, 7, size=(h, w)), 0, 255).astype(np.uint8)
    return left, right


def _check(backend, oracle, w, h, n, pairs):
    eL, eR = oracle.OracleExtractor(n, 1.2, 8, 20, 7), oracle.OracleExtractor(n, 1.2, 8, 20, 7)
    xl = orb_slam2_amd.ORBextractor(n, 1.2, 8, 20, 7, w, h, max_batch=len(pairs), library=backend)
    xr = orb_slam2_amd.ORBextractor(n, 1.2, 8, 20, 7, w, h, max_batch=len(pairs), library=backend)
    xl.extract_batch([p[0] for p in pairs])
    xr.extract_batch([p[1] for p in pairs])
    u, d = xl.ComputeStereoMatches(xr, MBF, MB, nimg=len(pairs))
    matched = []
    for f, (left, right) in enumerate(pairs):
        kl, _ = eL.extract(left)
        eR.extract(right)
        uo, do = oracle.stereo_matches(eL, eR, MBF, MB)
        nk = len(uo)
        assert u[f, :nk].tobytes() == uo.tobytes() and d[f, :nk].tobytes() == do.tobytes()
        assert np.all(u[f, nk:] == -1) and np.all(d[f, nk:] == -1)
        matched.append((kl, uo))
    xl.close()
    xr.close()
    return matched


def test_stereo_matches_bit_exact(backend, oracle):
    w, h, n = 480, 360, 600
    res = _check(backend, oracle, w, h, n, [stereo_pair(w, h, 4, 9), stereo_pair(w, h, 5, 21)])
    for (kl, uo), disp in zip(res, (9, 21)):
        ok = uo >= 0
        assert ok.sum() > 100
        assert abs(np.median(kl["x"][ok] - uo[ok]) - disp) < 0.5          # the synthetic rig's disparity is recovered


def test_stereo_random_sweep(backend, oracle):
    """Randomised sweep: image size, feature count, disparity (0 .. 40 px: the far / near ends of the search band) - ComputeStereoMatches bit for bit.
    3 pairs on the emulation, 24 on the GPU."""
    rng = np.random.default_rng(20260922)
    for case in range(3 if backend.endswith("_emu.so") else 24):
        w, h = int(rng.integers(80, 230)) * 4, int(rng.integers(60, 125)) * 4
        n = int(rng.choice([200, 500, 1000, 1500]))
        pairs = [stereo_pair(w, h, 100 + 2 * case + k, int(rng.integers(0, 41))) for k in range(1 if backend.endswith("_emu.so") else 2)]
        res = _check(backend, oracle, w, h, n, pairs)
        assert sum(int((uo >= 0).sum()) for _, uo in res) > 20, (case, w, h, n)
        if not backend.endswith("_emu.so") and case % 3 == 0:
            _pair_as_one_call(backend, oracle, w, h, n, pairs)                   # the same pairs through orbhip_extract_stereo (one context, two camera slots)


def test_stereo_edge_cases(backend, oracle):
    w, h, n = 400, 300, 400
    left, right = stereo_pair(w, h, 6, 0)
    # zero disparity (identical scenes): the `disparity <= 0 -> 0.01` branch (Frame.cc:611-615); no right keypoints at all;
    # no left keypoints at all
    _check(backend, oracle, w, h, n, [(left, right), (left, synth.zeros(w, h)), (synth.zeros(w, h), right), (left, left)])


@pytest.mark.gpu
def test_stereo_kitti_config(gpu_lib, oracle):
    """configs[1]: KITTI stereo 1241x376, 2000 features per image."""
    w, h, n = 1241, 376, 2000
    res = _check(gpu_lib, oracle, w, h, n, [stereo_pair(w, h, 7, 14), stereo_pair(w, h, 8, 40)])
    assert all((uo >= 0).sum() > 500 for _, uo in res)


def _pair_as_one_call(backend, oracle, w, h, n, pairs, max_batch=2):
    """orbhip_extract_stereo: both images through ONE context, the stereo matcher queued behind the extraction; everything it returns must equal the oracle
    (= two extractions + ComputeStereoMatches), and the follow-ups on the resident left frame must see it as frame 0."""
    x = orb_slam2_amd.ORBextractor(n, 1.2, 8, 20, 7, w, h, max_batch=max_batch, library=backend)
    eL, eR = oracle.OracleExtractor(n, 1.2, 8, 20, 7), oracle.OracleExtractor(n, 1.2, 8, 20, 7)
    sf = x.GetScaleFactors()
    for rep, (left, right) in enumerate(pairs):
        kl, dl, kr, dr, u, d = x.extract_stereo(left, right, MBF, MB)
        kol, dol = eL.extract(left); kor, dor = eR.extract(right)
        uo, do = oracle.stereo_matches(eL, eR, MBF, MB)
        assert kl.tobytes() == kol.tobytes() and np.array_equal(dl, dol) and kr.tobytes() == kor.tobytes() and np.array_equal(dr, dor)
        assert u.tobytes() == uo.tobytes() and d.tobytes() == do.tobytes()
        if len(kl) == 0:
            continue
        # the resident frame is the LEFT image, with its stereo columns: a motion-model search on it (twice: the second call finds the grid built behind the extraction)
        rng = np.random.default_rng(rep)
        q = np.zeros(len(kl), orb_slam2_amd.PROJ_QUERY_DTYPE)
        q["x"], q["y"] = kl["x"] + rng.normal(0, 1, len(kl)).astype(np.float32), kl["y"] + rng.normal(0, 1, len(kl)).astype(np.float32)
        q["radius"] = (7.0 * sf[kl["octave"]]).astype(np.float32); q["ur"] = q["x"] - 12.0
        q["min_level"], q["max_level"], q["blocks"], q["angle"] = kl["octave"] - 1, kl["octave"] + 1, 1, kl["angle"]
        for _ in range(2):
            n_g, f_g = x.search_by_projection(0, len(kl), q, dl, 1, nnratio=0.9, use_u_right=True)
            n_o, f_o = oracle.search_by_projection(kol, dol, w, h, q, dol, 1, nnratio=0.9, th_high=100, check_ori=True, u_right=uo)
            assert n_g == n_o and np.array_equal(f_g, f_o)
    x.close()


def test_stereo_pair_as_one_call(backend, oracle):
    w, h, n = 480, 360, 600
    _pair_as_one_call(backend, oracle, w, h, n, [stereo_pair(w, h, 4, 9), stereo_pair(w, h, 5, 21), (stereo_pair(w, h, 6, 0)[0], synth.zeros(w, h)), (synth.zeros(w, h), stereo_pair(w, h, 6, 0)[1]),
                                                  stereo_pair(w, h, 7, 3)])
    _pair_as_one_call(backend, oracle, 400, 300, 400, [stereo_pair(400, 300, 8, 11)], max_batch=3)      # a context with more slots than the pair


@pytest.mark.gpu
def test_stereo_pair_as_one_call_kitti(gpu_lib, oracle):
    _pair_as_one_call(gpu_lib, oracle, 1241, 376, 2000, [stereo_pair(1241, 376, 7, 14), stereo_pair(1241, 376, 8, 40)])
