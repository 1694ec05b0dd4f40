"""The fused device arithmetic of the matchers (ORBHIP_FP_CONTRACT) on the MI355X.

1. The boundary-straddling cases of tests/test_native_flags_matcher_exact.py as the device calls the drop-in classes make for them, recorded from the
   native-flags build (fused forms) and the canonical build together with the answers that made each equal the reference built the same way
   (tests/golden/native_flags_matcher_calls.npz): liborbhip.so gives the same answers.  Members: Fuse (mono and stereo), SearchByProjection(KF, Scw),
   Fuse(KF, Scw), SearchByProjection(Current, Last), SearchByProjection(Current, KF) of relocalisation, SearchBySim3 (both passes), and - in
   tests/golden/native_flags_triangulation_calls.npz - SearchForTriangulation (epipolar-line gate, long nodes, stereo key frames, the epipole's distance gate),
   through the single and the batched entry.  The triangulation replay also runs on the CPU emulation, so that a stale fixture shows without a GPU.
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
GOLDEN_TRI = os.path.join(TESTS, "golden", "native_flags_triangulation_calls.npz")
# the record counts tests/golden/make_golden_native_matcher.py printed when it wrote the fixtures (per build: the native-flags and the canonical one record the same calls)
CALLS = {"fuse": 1, "fuse_stereo": 1, "kf_sim3": 1, "fuse_sim3": 1, "last": 1, "reloc": 1, "sim3": 2}
TRI_CALLS = 72


def _replay(rec, library):
    """one recorded device call of a drop-in member (tests/golden/make_golden_native_matcher.py) through the C ABI of `library` -> (answers, recorded answers).
    SearchBySim3's two slots of orbhip_project_best_in_window_batch were recorded slot by slot; here each goes through the single entry, _replay_sim3_batch
    sends the two together through the batched one."""
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
    # (SearchBySim3's slots have no chi-square gate and hand the device no inverse sigmas: any will do)
    inv = np.ones(int(proj.nlevels), np.float32) if rec.get("inv_level_sigma2") is None else rec["inv_level_sigma2"].view(np.float32)
    bi, bd, _ = H.project_best_in_window(kps, desc, bounds, inv, proj, pts, pdesc, bool(ipar[0]), u_right=ur, library=library)
    return np.concatenate([bi, bd]), np.concatenate([rec["best_idx"].view(np.int32), rec["best_dist"].view(np.int32)])


def _replay_sim3_batch(recs, library):
    """the two recorded slots of SearchBySim3 (the last records: tests/golden/make_golden_native_matcher.py runs the member last) as ONE batch call, as the
    drop-in made it -> [(answers, recorded answers)] per slot"""
    slots = []
    for rec in recs[-CALLS["sim3"]:]:
        proj = H.Projection.from_buffer_copy(rec["proj"].tobytes())
        assert not int(rec["ipar"].view(np.int32)[0]) and rec.get("inv_level_sigma2") is None       # no chi-square gate: SearchBySim3's slots
        slots.append(dict(kps=rec["kps"].view(orb_slam2_amd.KEYPOINT_DTYPE), desc=rec["desc"].reshape(-1, 32), u_right=None, bounds=tuple(float(v) for v in rec["bounds"].view(np.float32)),
                          inv_level_sigma2=np.ones(int(proj.nlevels), np.float32), points=rec["points"].view(H.MAP_POINT_DTYPE), pdesc=rec["pdesc"].reshape(-1, 32), proj=proj))
    outs = H.project_best_in_window_batch(slots, False, library=library)
    return [(np.concatenate([o[0], o[1]]), np.concatenate([rec["best_idx"].view(np.int32), rec["best_dist"].view(np.int32)])) for o, rec in zip(outs, recs[-CALLS["sim3"]:])]


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
        assert {m: int(g[f"{tag}.n.{m}"]) for m in CALLS} == CALLS and len(recs) == int(g[f"{tag}.n"]) == sum(CALLS.values()), tag      # a fixture that lost a member fails
        for i, rec in enumerate(recs):
            kind = int(H.Projection.from_buffer_copy(rec["proj"].tobytes()).kind)
            assert bool(kind & H.FP_CONTRACT) == (tag == "native"), (tag, i, kind)       # the native-flags drop-in asked for the fused forms, the canonical one did not
            got, want = _replay(rec, gpu_lib)
            assert np.array_equal(got, want), (tag, i, int((got != want).sum()))
            answers[(tag, i)] = want
        for got, want in _replay_sim3_batch(recs, gpu_lib):      # both projections of SearchBySim3 in one launch, fused (native) and canonical
            assert np.array_equal(got, want), (tag, "sim3 batch", int((got != want).sum()))
    assert any(not np.array_equal(answers[("native", i)], answers[("canonical", i)]) for i in range(int(g["native.n"])))
    assert int(g["moved.reloc"]) >= 5 and int(g["moved.sim3"]) >= 5 and int(g["moved.sim3_pass1"]) >= 1 and int(g["moved.sim3_pass2"]) >= 1


def _tri_records(g, tag):
    """the triangulation records of one build: per-call arrays cut out of <tag>.<field>, pooled ones looked up (tests/golden/make_golden_native_matcher.py)"""
    out = []
    for i in range(int(g[f"{tag}.n"])):
        rec = {}
        for key in g:
            if not key.startswith(tag + ".") or key.endswith(".off") or key.count(".") != 1:
                continue
            name = key[len(tag) + 1:]
            if name.endswith("@"):
                rec[name[:-1]] = g[f"pool.{int(g[key][i])}"]
            elif name != "n":
                off = g[key + ".off"]
                rec[name] = g[key][off[i]:off[i + 1]]
        out.append(rec)
    return out


def _tri_side(rec, s):
    kp = rec[f"kp{s}"].view(np.float32).reshape(-1, 4)
    k = np.zeros(len(kp), orb_slam2_amd.KEYPOINT_DTYPE)
    k["x"], k["y"], k["angle"], k["octave"] = kp[:, 0], kp[:, 1], kp[:, 2], kp[:, 3].astype(np.int32)
    fv = (rec[f"fv{s}_node"].view(np.uint32), rec[f"fv{s}_off"].view(np.int32), rec[f"fv{s}_feat"].view(np.uint32))
    return dict(desc=rec[f"desc{s}"].reshape(-1, 32), kps=k, has_mp=rec[f"has_mp{s}"], stereo=rec[f"stereo{s}"], fv=fv,
                scale_factors=rec["scale_factors2"].view(np.float32), level_sigma2=rec["level_sigma2_2"].view(np.float32))


def _replay_triangulation(library):
    with np.load(GOLDEN_TRI) as z:
        g = {k: z[k] for k in z.files}                       # (an archive member is decompressed on every access: once)
    kinds = [str(k) for k in g["kinds"]]
    assert int(g["moved"]) >= 20 and all(k in kinds for k in ("long", "epi", "only_stereo", "stereo", "epi_stereo"))
    answers = {}
    for tag in ("native", "canonical"):
        recs = _tri_records(g, tag)
        assert len(recs) == TRI_CALLS == len(kinds), tag
        groups = {}
        for i, rec in enumerate(recs):
            ipar = rec["ipar"].view(np.int32)
            fc = bool(ipar[1] & H.FP_CONTRACT)
            assert fc == (tag == "native"), (tag, i, int(ipar[1]))      # the native-flags drop-in asked for the fused forms, the canonical one did not
            a, b = _tri_side(rec, 1), _tri_side(rec, 2)
            ex, ey = rec["epipole"].view(np.float32)
            want = np.append(rec["match12"].view(np.int32), ipar[2])
            n, m12 = H.search_for_triangulation(a["desc"], a["kps"], a["has_mp"], a["stereo"], a["fv"], b["desc"], b["kps"], b["has_mp"], b["stereo"], b["fv"],
                                                rec["F12"].view(np.float32), ex, ey, b["scale_factors"], b["level_sigma2"], only_stereo=bool(ipar[0]),
                                                check_ori=bool(ipar[1] & 1), library=library, fp_contract=int(fc))
            got = np.append(m12, np.int32(n))
            assert np.array_equal(got, want), (tag, i, str(kinds[i]), int((got != want).sum()))
            answers[(tag, i)] = want
            key = (int(ipar[0]), int(ipar[1])) + tuple(rec[f].tobytes() for f in ("desc1", "kp1", "has_mp1", "stereo1", "fv1_node", "fv1_off", "fv1_feat"))
            groups.setdefault(key, []).append((a, dict(kf=b, F12=rec["F12"].view(np.float32), ex=ex, ey=ey), want))
        # the batched entry: the recorded calls that share key frame 1 as the pairs of one batch
        assert max(len(v) for v in groups.values()) >= 3
        for key, members in groups.items():
            outs = H.search_for_triangulation_batch(members[0][0], [m[1] for m in members], only_stereo=bool(key[0]), check_ori=bool(key[1] & 1),
                                                    library=library, fp_contract=int(tag == "native"))
            for (n, m12), (_, _, want) in zip(outs, members):
                assert np.array_equal(np.append(m12, np.int32(n)), want), (tag, "batch")
    differ = [i for i in range(TRI_CALLS) if not np.array_equal(answers[("native", i)], answers[("canonical", i)])]
    assert len(differ) >= TRI_CALLS - 2                      # the flag reaches the triangulation kernel: all but the two agreeing calls answer differently
    assert any(kinds[i] == "long" for i in differ) and any(kinds[i] == "epi" for i in differ)


def test_device_replays_the_triangulation_calls_of_both_reference_builds(backend):
    """SearchForTriangulation as the drop-in classes called the device for the boundary-straddling cases (aimed pairs on the epipolar-line gate, side-2 nodes of
    more than 256 features, stereo key frames, the epipole on its distance gate): liborbhip.so answers every call - single entry and batch - as the emulation did
    when those answers made the member equal the native-flags / canonical reference.  On the CPU emulation too: the fixture belongs to the kernels as they are."""
    _replay_triangulation(backend)


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


def _triangulation_case(rng, n=240, aimed=False):
    """aimed (with n = 600: one node of 600 features on side 2, the kernel's long-node loop): feature perm[i] of side 2 copies the descriptor of feature i of
    side 1 and its y is solved (in double) so that num*num/den of the pair sits at 3.84 * sigma2[octave] - within the float rounding of y, which is the rounding
    the fused and the unfused forms differ by"""
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
    if aimed:
        perm = rng.permutation(n)
        d2 = np.zeros_like(d1); d2[perm] = d1
        G = F.astype(np.float32).astype(np.float64)
        x1, y1, x2 = k1["x"].astype(np.float64), k1["y"].astype(np.float64), k2["x"][perm].astype(np.float64)
        a = x1 * G[0, 0] + y1 * G[1, 0] + G[2, 0]; b = x1 * G[0, 1] + y1 * G[1, 1] + G[2, 1]; c = x1 * G[0, 2] + y1 * G[1, 2] + G[2, 2]
        num = rng.choice([-1.0, 1.0], n) * np.sqrt(3.84 * (sf * sf).astype(np.float64)[k2["octave"][perm]] * (a * a + b * b))
        k2["y"][perm] = ((num - a * x2 - c) / b).astype(np.float32)
    return (d1, k1, z, z, fv, d2, k2, z, z, fv, F.astype(np.float32), float(rng.uniform(-5e3, 5e3)), float(rng.uniform(-5e3, 5e3)), sf, sf * sf)


@pytest.mark.gpu
def test_fused_triangulation_equals_the_emulation(gpu_lib, emu_lib):
    rng = np.random.default_rng(8)
    total = moved = 0
    for case in range(6):                                   # the last two: one node of 600 features on side 2 (the long-node loop), pairs aimed at the line gate
        a = _triangulation_case(rng, 600, aimed=True) if case >= 4 else _triangulation_case(rng)
        answers = []
        for fc in (0, 1):
            ng, mg = H.search_for_triangulation(*a, check_ori=False, library=gpu_lib, fp_contract=fc)
            ne, me = H.search_for_triangulation(*a, check_ori=False, library=emu_lib, fp_contract=fc)
            assert ng == ne and np.array_equal(mg, me), (case, fc)
            total += ng
            answers.append(mg)
        moved += int((answers[0] != answers[1]).sum())
        if case >= 4:
            assert ng > 100 and (answers[0] != answers[1]).any(), case      # aimed pairs on both sides of the gate, and the flag moves some of them
        outs = H.search_for_triangulation_batch(dict(desc=a[0], kps=a[1], has_mp=a[2], stereo=a[3], fv=a[4], scale_factors=a[13], level_sigma2=a[14]),
                                                [dict(kf=dict(desc=a[5], kps=a[6], has_mp=a[7], stereo=a[8], fv=a[9], scale_factors=a[13], level_sigma2=a[14]), F12=a[10], ex=a[11], ey=a[12])],
                                                library=gpu_lib, fp_contract=1)
        n1, m1 = H.search_for_triangulation(*a, check_ori=False, library=gpu_lib, fp_contract=1)
        assert outs[0][0] == n1 and np.array_equal(outs[0][1], m1)
        if case >= 4:                                       # the long node through the canonical batch kernel too
            o0 = H.search_for_triangulation_batch(dict(desc=a[0], kps=a[1], has_mp=a[2], stereo=a[3], fv=a[4], scale_factors=a[13], level_sigma2=a[14]),
                                                  [dict(kf=dict(desc=a[5], kps=a[6], has_mp=a[7], stereo=a[8], fv=a[9], scale_factors=a[13], level_sigma2=a[14]), F12=a[10], ex=a[11], ey=a[12])],
                                                  library=gpu_lib, fp_contract=0)
            assert np.array_equal(o0[0][1], answers[0])
    assert total > 10 and moved > 0                         # fp_contract = 0 and = 1 are two kernels


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
