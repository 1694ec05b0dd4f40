"""The fused device arithmetic of the matchers (ORBHIP_FP_CONTRACT) on the MI355X.

1. The boundary-straddling cases of tests/test_native_flags_matcher_exact.py as the device calls the drop-in classes make for them, recorded from the
   native-flags build (fused forms) and the canonical build together with the answers that made each equal the reference built the same way
   (tests/golden/native_flags_matcher_calls.npz): liborbhip.so gives the same answers.
2. General scenes through the C ABI: the fused kernels' derived queries (queries_out), matches and Fuse answers equal the emulation's fused ones, and differ
   from the canonical kernels' on some points - the flag reaches the kernel.  The same for SearchForTriangulation's entry."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
import orb_slam2_amd  # noqa: E402
from orb_slam2_amd import orbhip as H  # noqa: E402

GOLDEN = os.path.join(TESTS, "golden", "native_flags_matcher_calls.npz")


def _replay(rec, library):
    """one recorded device call of a drop-in member (tests/golden/make_golden_native_matcher.py) through the C ABI of `library` -> (answers, recorded answers)"""
    kps = rec["kps"].view(orb_slam2_amd.KEYPOINT_DTYPE); desc = rec["desc"].reshape(-1, 32)
    ur = None if rec.get("u_right") is None else rec["u_right"].view(np.float32)
    bounds = tuple(float(v) for v in rec["bounds"].view(np.float32))
    proj = H.Projection.from_buffer_copy(rec["proj"].tobytes())
    pts = rec["points"].view(H.MAP_POINT_DTYPE); pdesc = rec["pdesc"].reshape(-1, 32)
    ipar = rec["ipar"].view(np.int32)
    if int(rec["tag"]) == 1:
        bl = None if rec.get("blocked") is None else rec["blocked"]
        nm, fq, _ = H.project_search(kps, desc, bounds, proj, pts, pdesc, nnratio=float(rec["fpar"].view(np.float32)[0]), th_high=int(ipar[0]), check_ori=bool(ipar[1]),
                                     u_right=ur, blocked=bl, library=library)
        return np.append(fq, nm), np.append(rec["feature_query"].view(np.int32), ipar[2])
    inv = rec["inv_level_sigma2"].view(np.float32)
    bi, bd, _ = H.project_best_in_window(kps, desc, bounds, inv, proj, pts, pdesc, bool(ipar[0]), u_right=ur, library=library)
    return np.concatenate([bi, bd]), np.concatenate([rec["best_idx"].view(np.int32), rec["best_dist"].view(np.int32)])


def _records(g, tag):
    out = []
    for i in range(int(g[tag + ".n"])):
        pre = f"{tag}.{i}."
        out.append({k[len(pre):]: g[k] for k in g.files if k.startswith(pre)})
    return out


@pytest.mark.gpu
def test_device_replays_the_dropin_calls_of_both_reference_builds(gpu_lib):
    """The device calls the drop-in classes make on the boundary-straddling cases, recorded from the native-flags build (fused forms requested) and the
    canonical one: liborbhip.so answers each exactly as the emulation did when those answers made the members equal the native-flags / canonical reference."""
    g = np.load(GOLDEN)
    assert int(g["moved"]) >= 20
    answers = {}
    for tag in ("native", "canonical"):
        recs = _records(g, tag)
        assert len(recs) >= 5
        for i, rec in enumerate(recs):
            kind = int(H.Projection.from_buffer_copy(rec["proj"].tobytes()).kind)
            assert bool(kind & H.FP_CONTRACT) == (tag == "native"), (tag, i, kind)       # the native-flags drop-in asked for the fused forms, the canonical one did not
            got, want = _replay(rec, gpu_lib)
            assert np.array_equal(got, want), (tag, i, int((got != want).sum()))
            answers[(tag, i)] = want
    assert any(not np.array_equal(answers[("native", i)], answers[("canonical", i)]) for i in range(int(g["native.n"])))


def _projection_cases(library):
    import test_parity_projection_algebra as T
    T._case.library = library
    rng = np.random.default_rng(2024)
    n = 900
    kps = np.zeros(n, orb_slam2_amd.KEYPOINT_DTYPE)
    kps["x"] = rng.uniform(0, T.W, n).astype(np.float32); kps["y"] = rng.uniform(0, T.HT, n).astype(np.float32)
    kps["octave"] = rng.integers(0, 8, n); kps["angle"] = rng.uniform(0, 360, n).astype(np.float32); kps["size"] = 31.0
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ur = np.where(rng.random(n) < 0.6, kps["x"] - rng.uniform(1, 60, n), -1.0).astype(np.float32)
    out = []
    for kind in T.KINDS:
        P, pts, _, bounds = T._case(rng, kind, 0, npts=2000)
        pdesc = desc[rng.integers(0, n, len(pts))] ^ (rng.random((len(pts), 32)) < 0.04).astype(np.uint8)
        out.append((kind, P, pts, pdesc, bounds))
    return kps, desc, ur, out


def _run_projection(lib_path, kps, desc, ur, cases, fc):
    res = []
    for kind, P, pts, pdesc, bounds in cases:
        if kind in ("last_frame", "frame_kf", "kf_sim3"):
            nm, fq, q = H.project_search(kps, desc, bounds, P, pts, pdesc, nnratio=0.9, th_high=100, check_ori=kind != "kf_sim3",
                                         u_right=ur if kind == "last_frame" else None, library=lib_path, fp_contract=fc)
            res.append((kind, q, np.append(fq, nm)))
        else:
            inv = (1.0 / (np.asarray(P.scale_factors[:P.nlevels], np.float32) ** 2)).astype(np.float32)
            chi2 = kind == "fuse"
            bi, bd, q = H.project_best_in_window(kps, desc, bounds, inv, P, pts, pdesc, chi2, u_right=ur if chi2 else None, library=lib_path, fp_contract=fc)
            res.append((kind, q, np.concatenate([bi, bd])))
    return res


@pytest.mark.gpu
def test_fused_kernels_equal_the_emulation_and_differ_from_the_canonical(gpu_lib, emu_lib):
    kps, desc, ur, cases = _projection_cases(emu_lib)
    g1, e1 = _run_projection(gpu_lib, kps, desc, ur, cases, 1), _run_projection(emu_lib, kps, desc, ur, cases, 1)
    g0 = _run_projection(gpu_lib, kps, desc, ur, cases, 0)
    moved = {}
    for (kind, qg, og), (_, qe, oe), (_, q0, o0) in zip(g1, e1, g0):
        assert qg.tobytes() == qe.tobytes(), f"{kind}: the fused kernel's queries differ from the emulation's"
        assert np.array_equal(og, oe), f"{kind}: the fused kernel's answers differ from the emulation's"
        moved[kind] = int(((qg["x"] != q0["x"]) | (qg["y"] != q0["y"]) | (qg["ur"] != q0["ur"])).sum())
    assert all(moved[k] > 0 for k in moved), moved          # every statement sequence has points whose u / v / ur move with the flag


def _triangulation_case(rng, n=240):
    k1 = np.zeros(n, orb_slam2_amd.KEYPOINT_DTYPE); k2 = np.zeros(n, orb_slam2_amd.KEYPOINT_DTYPE)
    for k in (k1, k2):
        k["x"] = rng.uniform(0, 640, n).astype(np.float32); k["y"] = rng.uniform(0, 480, n).astype(np.float32)
        k["octave"] = rng.integers(0, 4, n); k["angle"] = rng.uniform(0, 360, n).astype(np.float32); k["size"] = 31.0
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d2 = d1[rng.permutation(n)] ^ (rng.random((n, 32)) < 0.05).astype(np.uint8)
    # F12 of a small sideways motion: epipolar lines nearly horizontal, so y2 - y1 decides; the points of side 2 sit near side 1's rows
    k2["y"] = (k1["y"][rng.permutation(n)] + rng.normal(0, 1.5, n)).astype(np.float32)
    F = np.array([[0, -1e-4, 0.011], [1e-4, 0, -0.96], [-0.012, 0.97, 0.8]], np.float64) + rng.normal(0, 1e-6, (3, 3))
    fv = (np.array([7], np.uint32), np.array([0, n], np.int32), np.arange(n, dtype=np.uint32))
    z = np.zeros(n, np.uint8)
    sf = (1.2 ** np.arange(8)).astype(np.float32)
    return (d1, k1, z, z, fv, d2, k2, z, z, fv, F.astype(np.float32), float(rng.uniform(-5e3, 5e3)), float(rng.uniform(-5e3, 5e3)), sf, sf * sf)


@pytest.mark.gpu
def test_fused_triangulation_equals_the_emulation(gpu_lib, emu_lib):
    rng = np.random.default_rng(8)
    total = 0
    for _ in range(4):
        a = _triangulation_case(rng)
        for fc in (0, 1):
            ng, mg = H.search_for_triangulation(*a, check_ori=False, library=gpu_lib, fp_contract=fc)
            ne, me = H.search_for_triangulation(*a, check_ori=False, library=emu_lib, fp_contract=fc)
            assert ng == ne and np.array_equal(mg, me), fc
            total += ng
        outs = H.search_for_triangulation_batch(dict(desc=a[0], kps=a[1], has_mp=a[2], stereo=a[3], fv=a[4], scale_factors=a[13], level_sigma2=a[14]),
                                                [dict(kf=dict(desc=a[5], kps=a[6], has_mp=a[7], stereo=a[8], fv=a[9], scale_factors=a[13], level_sigma2=a[14]), F12=a[10], ex=a[11], ey=a[12])],
                                                library=gpu_lib, fp_contract=1)
        n1, m1 = H.search_for_triangulation(*a, check_ori=False, library=gpu_lib, fp_contract=1)
        assert outs[0][0] == n1 and np.array_equal(outs[0][1], m1)
    assert total > 10


def test_flag_bits_are_validated(emu_lib):
    """kind | ORBHIP_FP_CONTRACT is accepted, any other high bit is ORBHIP_ERR_INVALID; batch slots must agree on the flag"""
    kps, desc, ur, cases = _projection_cases(emu_lib)
    kind, P, pts, pdesc, bounds = cases[3]                  # fuse
    inv = (1.0 / (np.asarray(P.scale_factors[:P.nlevels], np.float32) ** 2)).astype(np.float32)
    H.project_best_in_window(kps, desc, bounds, inv, P, pts[:50], pdesc[:50], True, u_right=ur, library=emu_lib, fp_contract=1)
    bad = H.Projection.from_buffer_copy(P); bad.kind |= 0x200
    with pytest.raises(H.OrbHipError):
        H.project_best_in_window(kps, desc, bounds, inv, bad, pts[:50], pdesc[:50], True, u_right=ur, library=emu_lib)
    fused = H._proj_fc(P, 1)
    slot = dict(kps=kps, desc=desc, u_right=ur, bounds=bounds, inv_level_sigma2=inv, points=pts[:50], pdesc=pdesc[:50])
    with pytest.raises(H.OrbHipError):
        H.project_best_in_window_batch([dict(slot, proj=P), dict(slot, proj=fused)], True, library=emu_lib)
    a, b = H.project_best_in_window_batch([dict(slot, proj=fused)] * 2, True, library=emu_lib)
    bi, bd, _ = H.project_best_in_window(kps, desc, bounds, inv, P, pts[:50], pdesc[:50], True, u_right=ur, library=emu_lib, fp_contract=1)
    assert np.array_equal(a[0], bi) and np.array_equal(b[1], bd)
