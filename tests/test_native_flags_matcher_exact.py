"""H3 closed for the matcher's device arithmetic: the drop-in built with the reference's OWN flags (-O3 -march=native: its ORBmatcher.cc sees __FMA__ and asks the device for
the fused forms, ORBHIP_FP_CONTRACT) against the reference built the same way, on BOUNDARY-STRADDLING cases - map points placed so that the projected u / v, the search
radius or Fuse's chi-square value lies within a few ulps of its gate, kept where the native-flags reference and the canonical (-ffp-contract=off) one disagree.  On
these cases a device that rounded every operation once would follow the canonical build; the drop-in must follow the native one, member output for member output.
CPU only (-march=native is the build host's; kernels under the emulation).  tests/golden/make_golden_native_matcher.py records the device calls both drop-in
builds make on these cases for the -m gpu replay (tests/test_native_flags_matcher_gpu.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import gpu_session  # noqa: E402
from orb_slam2_amd import synth  # noqa: E402

W, H, N = 480, 360, 700
CAM = dict(fx=300.0, fy=300.0, cx=240.0, cy=180.0)
SF = 1.2
MEMBERS = ("fuse", "fuse_stereo", "kf_sim3", "fuse_sim3", "last")


def _pose(rng, max_deg=8.0, max_t=0.3):
    import test_projection_poses as T
    return T._pose(rng, max_deg, max_t)


def _world_at(T, u, v, z, scale=1.0):
    """world points that the camera [R | t / scale] sees at pixel (u, v), depth z"""
    cam = np.stack([(u - CAM["cx"]) / CAM["fx"] * z, (v - CAM["cy"]) / CAM["fy"] * z, z], 1)
    R, t = T[:3, :3], T[:3, 3] / scale
    w = (R.T @ (cam - t).T).T
    return [np.ascontiguousarray(w[:, i], np.float32) for i in range(3)]


def frames(S, library):
    """the two frames every case is built on (mono pair + the stereo key frame of Fuse's three-term gate)"""
    seq = synth.sequence(W, H, 2, seed=41)
    kw = dict(nfeatures=N, bf=40.0, **CAM)
    return {"f0": S.RefFrame(seq[0], library=library, **kw), "f1": S.RefFrame(seq[1], library=library, **kw),
            "st": S.RefFrame(seq[1], np.roll(seq[1], -9, axis=1), library=library, **kw)}


def candidates(F, seed=5, per_key=3):
    """points aimed at a gate of each member (within an ulp or so of it after the float world coordinates and R*x+t): Fuse's chi-square bound 5.99 / 7.8 at the key
    point's level, the radius window of KF_SIM3 / FUSE_SIM3 / LAST_FRAME.  Each point copies the descriptor of the key point it is aimed at (distance 0)."""
    rng = np.random.default_rng(seed)
    A = _pose(rng)
    s12 = float(rng.uniform(0.9, 1.15))
    out = {"A": A, "s12": s12}
    for name, fr in (("fuse", "f1"), ("fuse_stereo", "st"), ("kf_sim3", "f1"), ("fuse_sim3", "f1")):
        k = F[fr].keys_un
        idx = np.repeat(np.arange(len(k)), per_key)
        if name == "fuse_stereo":
            idx = idx[F[fr].u_right[idx] >= 0]
        oct_ = k["octave"][idx].astype(np.int32)
        n = len(idx)
        th = {"fuse": 3.0, "fuse_stereo": 3.0, "kf_sim3": 10.0, "fuse_sim3": 4.0}[name]
        sf = SF ** oct_
        ang = rng.uniform(0, 2 * np.pi, n)
        if name.startswith("fuse") and name != "fuse_sim3":
            rho = np.sqrt(5.99 * sf * sf) if name == "fuse" else np.sqrt(7.8 * sf * sf / 1.49)    # stereo: er = 0.7 rho below
        else:
            ang = rng.choice([0.0, np.pi], n) + rng.uniform(-0.3, 0.3, n)                              # the x edge of the window: |kx - u| < r
            rho = th * sf / np.abs(np.cos(ang))
        rho = rho * (1.0 + rng.integers(-3, 4, n) * 2.0 ** -23)
        u = k["x"][idx] + rho * np.cos(ang); v = k["y"][idx] + rho * np.sin(ang)
        z = rng.uniform(3.0, 9.0, n)
        if name == "fuse_stereo":                              # the right coordinate's share: ur - kpr = (u - kx) + disparity - bf/z = +-0.7 rho
            disp = k["x"][idx] - F[fr].u_right[idx]
            z = 40.0 / np.maximum(rho * np.cos(ang) + disp - 0.7 * rho * rng.choice([-1, 1], n), 0.5)
        X, Y, Z = _world_at(A, u, v, z, scale=s12 if name in ("kf_sim3", "fuse_sim3") else 1.0)
        out[name] = dict(idx=idx.astype(np.int32), X=X, Y=Y, Z=Z, level=oct_, desc=F[fr].desc[idx], th=th)
    # LAST_FRAME: one point per feature of the last frame, aimed at the radius edge around a key point of the current frame of a level the search accepts
    kl, kc = F["f0"].keys_un, F["f1"].keys_un
    nq = len(kl)
    th = 15.0
    tgt = np.zeros(nq, np.int32)
    for i in range(nq):
        ok = np.nonzero(np.abs(kc["octave"] - kl["octave"][i]) <= 1)[0]
        tgt[i] = ok[rng.integers(len(ok))]
    r = th * SF ** kl["octave"].astype(np.float64)
    ang = rng.choice([0.0, np.pi], nq) + rng.uniform(-0.3, 0.3, nq)
    rho = r / np.abs(np.cos(ang)) * (1.0 + rng.integers(-3, 4, nq) * 2.0 ** -23)
    u = kc["x"][tgt] + rho * np.cos(ang); v = kc["y"][tgt] + rho * np.sin(ang)
    X, Y, Z = _world_at(A, u, v, rng.uniform(3.0, 9.0, nq))
    out["last"] = dict(idx=tgt, X=X, Y=Y, Z=Z, level=kl["octave"].astype(np.int32), desc=F["f1"].desc[tgt], th=th)
    return out


def run(S, L, F, cases, which=MEMBERS):
    """every member on its cases through library L (frames F made by L) -> {member: output array}"""
    A, s12 = cases["A"], cases["s12"]
    S.set_test_poses(A, A, s12, None, None, library=L)
    try:
        res = {}
        for m in which:
            c = cases[m]
            nq = len(c["X"])
            z8 = np.zeros(nq, np.uint8)
            if m in ("fuse", "fuse_stereo"):
                fr = F["f1" if m == "fuse" else "st"]
                n, out = S.fuse(fr, np.zeros(fr.N, np.uint8), c["X"], c["Y"], c["Z"], c["level"], np.zeros(nq, np.int32), z8, c["desc"], th=c["th"])
            elif m == "kf_sim3":
                n, out = S.search_by_projection_kf(F["f1"], np.zeros(F["f1"].N, np.uint8), c["X"], c["Y"], c["Z"], c["level"], z8, c["desc"], th=int(c["th"]))
            elif m == "fuse_sim3":
                n, out = S.fuse_sim3(F["f1"], np.zeros(F["f1"].N, np.uint8), c["X"], c["Y"], c["Z"], c["level"], z8, c["desc"], th=c["th"])
            else:
                n, out = S.search_by_projection_last(F["f1"], F["f0"], np.ones(nq, np.uint8), c["X"], c["Y"], c["Z"], c["desc"], th=c["th"], mono=True, nnratio=0.9, check_ori=False)
            res[m] = np.append(np.asarray(out, np.int32), np.int32(n))
        return res
    finally:
        S.set_test_poses(None, library=L)


def _subset(c, keep):
    d = dict(c)
    for f in ("idx", "X", "Y", "Z", "level", "desc"):
        d[f] = np.ascontiguousarray(c[f][keep])
    return d


def straddling_cases(S, nat, can, Fn, Fc, seed=5):
    """candidates() reduced to the points whose member outputs differ between the native-flags reference (nat) and the canonical one (can).  LAST_FRAME keeps
    every point (one per feature of the last frame: its claims interact), the other members the points that moved an output."""
    cases = candidates(Fn, seed)
    rn, rc = run(S, nat, Fn, cases), run(S, can, Fc, cases)
    for m in ("fuse", "fuse_stereo", "fuse_sim3"):
        keep = np.nonzero(rn[m][:-1] != rc[m][:-1])[0]
        cases[m] = _subset(cases[m], keep)
    a, b = rn["kf_sim3"][:-1], rc["kf_sim3"][:-1]                 # feature -> point: keep the points named on either side where they differ
    q = np.unique(np.concatenate([a[(a != b) & (a >= 0)], b[(a != b) & (b >= 0)]]))
    cases["kf_sim3"] = _subset(cases["kf_sim3"], q)
    return cases


def _libs(request):
    if gpu_session(request.config):
        pytest.skip("CPU only")
    from oracle import orbslam_ref as S
    if not (S.build() and S.build_native() and S.build_dropin() and S.build_dropin_native()):
        pytest.skip("reference sources not mounted")
    return S


def test_dropin_follows_the_native_reference_across_the_gates(request, capsys):
    S = _libs(request)
    nat, can, dnat, dcan = S.native_lib(), None, S.dropin_native_lib(), S.dropin_full_lib()
    S.RefFrame._geometry = None
    S.RefFrame._geometry_other.clear()
    Fn, Fc, Fdn, Fdc = frames(S, nat), frames(S, can), frames(S, dnat), frames(S, dcan)
    try:
        for k in Fn:                                          # the extractor's own exposure (H3) is not what this test measures: same key points on every side
            assert Fn[k].keys_un.tobytes() == Fdn[k].keys_un.tobytes() and Fc[k].keys_un.tobytes() == Fdc[k].keys_un.tobytes()
        cases = straddling_cases(S, nat, can, Fn, Fc)
        rn, rc, rdn, rdc = run(S, nat, Fn, cases), run(S, can, Fc, cases), run(S, dnat, Fdn, cases), run(S, dcan, Fdc, cases)
        moved = {m: int((rn[m] != rc[m]).sum()) for m in MEMBERS}
        with capsys.disabled():
            print("\nboundary cases: points " + ", ".join(f"{m} {len(cases[m]['X'])}" for m in MEMBERS) +
                  "; member outputs that differ between the native-flags and the canonical reference: " + ", ".join(f"{m} {moved[m]}" for m in MEMBERS))
        assert sum(moved.values()) >= 20, moved                # the cases straddle gates: the two reference builds answer differently
        assert sum(moved[m] > 0 for m in MEMBERS) >= 3, moved
        for m in MEMBERS:
            assert np.array_equal(rdn[m], rn[m]), (m, int((rdn[m] != rn[m]).sum()))       # native drop-in == native reference, every output
            assert np.array_equal(rdc[m], rc[m]), (m, int((rdc[m] != rc[m]).sum()))       # canonical drop-in == canonical reference (mode 0 unchanged)
    finally:
        for F in (Fn, Fc, Fdn, Fdc):
            for f in F.values():
                f.close()
        S.RefFrame._geometry = None
        S.RefFrame._geometry_other.clear()


def test_native_builds_agree_strictly_under_general_poses(request):
    """tests/test_projection_poses.py's general poses, strict: every member and ORBmatcher::IsInFrustum, native drop-in against native reference"""
    S = _libs(request)
    import test_projection_poses as T
    checked, differs = T._run(S, S.dropin_native_lib(), strict=True, base=S.native_lib())
    assert not any(differs.values()) and checked["last"] > 800, (checked, differs)

