"""H3 closed for the matcher's device arithmetic: the drop-in built with the reference's OWN flags (-O3 -march=native: its ORBmatcher.cc sees __FMA__ and asks the device for
the fused forms, ORBHIP_FP_CONTRACT) against the reference built the same way, on BOUNDARY-STRADDLING cases - map points placed so that the projected u / v, the search
radius or Fuse's chi-square value lies within a few ulps of its gate, kept where the native-flags reference and the canonical (-ffp-contract=off) one disagree.  On
these cases a device that rounded every operation once would follow the canonical build; the drop-in must follow the native one, member output for member output.
Members: Fuse (mono, stereo), SearchByProjection(KF, Scw), Fuse(KF, Scw), SearchByProjection(Current, Last); SearchByProjection(Current, KF) of relocalisation and
SearchBySim3 (radius window, both passes); SearchForTriangulation (an aimed pair per call on the epipolar-line gate 3.84 sigma2 - small nodes, side-2 nodes of more
than 256 features, a stereo key frame 2, bOnlyStereo - and the epipole on its distance gate 100 sf[octave]).
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
NEW_MEMBERS = ("reloc", "sim3", "tri")                     # SearchByProjection(Frame, KeyFrame) of relocalisation, SearchBySim3 (both passes), SearchForTriangulation
ALL_MEMBERS = MEMBERS + NEW_MEMBERS


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
    right = np.roll(seq[1], -9, axis=1)
    return {"f0": S.RefFrame(seq[0], library=library, **kw), "f1": S.RefFrame(seq[1], library=library, **kw),
            "st": S.RefFrame(seq[1], right, library=library, **kw),
            # SearchForTriangulation's second key frame: the same image again, so that feature i of both sides is one key point with one descriptor
            "f1b": S.RefFrame(seq[1], library=library, **kw), "stb": S.RefFrame(seq[1], right, library=library, **kw)}


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
    out["reloc"] = _reloc_candidates(rng, F, A)
    out["sim3"] = _sim3_candidates(rng, F, A, s12)
    out["tri"] = _tri_candidates(rng, F)
    return out


def _edge(rng, r):
    """offsets (du, dv) from a key point that put it on the x edge of a search window of radius r (|kx - u| < r), within 3 ulps of r"""
    n = len(r)
    ang = rng.choice([0.0, np.pi], n) + rng.uniform(-0.3, 0.3, n)
    rho = r / np.abs(np.cos(ang)) * (1.0 + rng.integers(-3, 4, n) * 2.0 ** -23)
    return rho * np.cos(ang), rho * np.sin(ang)


def _world_from(M, u, v, z):
    """world points that the camera-from-world transform M (4x4, a scale inside its rotation block allowed) sees at pixel (u, v), depth z"""
    cam = np.stack([(u - CAM["cx"]) / CAM["fx"] * z, (v - CAM["cy"]) / CAM["fy"] * z, z, np.ones(len(z))], 1)
    w = (np.linalg.inv(M) @ cam.T).T
    return [np.ascontiguousarray(w[:, i], np.float32) for i in range(3)], np.linalg.norm(cam[:, :3], axis=1)


def _level_for(want, world, dist):
    """the level to hand the wrapper's query point (its mfMaxDistance = |world| * 1.2^(level - 0.4)) so that MapPoint::PredictScale at distance `dist` lands
    on `want`, and the level it then lands on (the float world coordinates and the clamp to 0..7 can make it another one)"""
    delta = np.log(np.linalg.norm(np.stack(world, 1).astype(np.float64), axis=1) / dist) / np.log(SF)
    level = np.clip(np.floor(want + 0.4 - delta), 0, 7).astype(np.int32)
    return level, np.clip(np.ceil(level - 0.4 + delta), 0, 7).astype(np.int32)


def _reloc_candidates(rng, F, A, th=10.0):
    """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist): one point per feature of the key frame (f0), aimed at the radius window
    |kx - u| < th * sf[predicted level] around a key point of the current frame (f1) whose octave is the predicted level or next to it"""
    kk, kc = F["f0"].keys_un, F["f1"].keys_un
    nq = len(kk)
    tgt = rng.integers(0, len(kc), nq).astype(np.int32)
    want = np.clip(kc["octave"][tgt] + rng.integers(-1, 2, nq), 0, 7)
    z = rng.uniform(3.0, 9.0, nq)
    Ow = -A[:3, :3].T @ A[:3, 3]
    level = pred = want
    seed = int(rng.integers(1 << 30))
    for _ in range(2):                                            # the predicted level depends (weakly) on where the point is, and the radius on the predicted level
        du, dv = _edge(np.random.default_rng(seed), th * SF ** pred.astype(np.float64))
        X, Y, Z = _world_at(A, kc["x"][tgt] + du, kc["y"][tgt] + dv, z)
        w = np.stack([X, Y, Z], 1).astype(np.float64)
        level, pred = _level_for(want, (X, Y, Z), np.linalg.norm(w - Ow, axis=1))
    return dict(idx=tgt, X=X, Y=Y, Z=Z, level=level, desc=F["f1"].desc[tgt], th=th)


def _sim3_candidates(rng, F, A, s12, th=7.5):
    """SearchBySim3: feature i1 of key frame 1 (f0, pose A) paired with a feature i2 of key frame 2 (f1, pose B) of the same octave; each carries a point with the
    OTHER one's descriptor.  A match needs both passes to agree: one pass sees its point exactly on the partner's key point, the other on the edge of the radius
    window th * sf[predicted level] - which pass is the aimed one alternates, so both projections of the batch entry decide outputs."""
    import test_projection_poses as T
    B = T._pose(rng)
    T12 = A @ np.linalg.inv(B)
    R12, t12 = T12[:3, :3], T12[:3, 3]
    k1, k2 = F["f0"].keys_un, F["f1"].keys_un
    i1s, i2s = [], []
    for o in range(8):
        a, b = rng.permutation(np.nonzero(k1["octave"] == o)[0]), rng.permutation(np.nonzero(k2["octave"] == o)[0])
        m = min(len(a), len(b))
        i1s.append(a[:m]); i2s.append(b[:m])
    i1, i2 = np.concatenate(i1s), np.concatenate(i2s)
    n = len(i1)
    first = rng.random(n) < 0.5                                      # the pass that is aimed at the edge: key frame 1's points into key frame 2, or the reverse
    octave = k1["octave"][i1].astype(np.float64)
    M1 = np.eye(4); M1[:3, :3] = R12.T / s12; M1[:3, 3] = -(R12.T / s12) @ t12                    # camera 2 from camera 1
    M2 = np.eye(4); M2[:3, :3] = s12 * R12; M2[:3, 3] = t12                                       # camera 1 from camera 2
    out = dict(B=B, R12=R12, t12=t12, th=th, i1=i1.astype(np.int32), i2=i2.astype(np.int32), first=first)
    for side, M, ksrc, isrc, kdst, idst, aimed in ((1, M1 @ A, k1, i1, k2, i2, first), (2, M2 @ B, k2, i2, k1, i1, ~first)):
        du, dv = _edge(rng, th * SF ** octave)
        du, dv = np.where(aimed, du, 0.0), np.where(aimed, dv, 0.0)
        world, dist = _world_from(M, kdst["x"][idst] + du, kdst["y"][idst] + dv, rng.uniform(3.0, 9.0, n))
        level, pred = _level_for(octave, world, dist)
        has = np.zeros(len(ksrc), np.uint8); has[isrc] = pred == octave
        full = [np.zeros(len(ksrc), np.float32) for _ in range(3)]
        for f, w in zip(full, world):
            f[isrc] = w
        lev = np.zeros(len(ksrc), np.int32); lev[isrc] = level
        desc = np.zeros((len(ksrc), 32), np.uint8); desc[isrc] = (F["f1"] if side == 1 else F["f0"]).desc[idst]
        out[f"has{side}"], out[f"P{side}"], out[f"level{side}"], out[f"desc{side}"] = has, full, lev, desc
    return out


def _f32_sf():
    sf = np.ones(8, np.float32)
    for i in range(1, 8):
        sf[i] = sf[i - 1] * np.float32(SF)                          # ORBextractor's mvScaleFactor
    return sf


def _epipole_t2w(rng, x2, y2, octave, tries=40000):
    """translations (tx, ty, 1) of key frame 2 whose epipole (fx tx + cx, fy ty + cy) lies at the distance gate of SearchForTriangulation around (x2, y2):
    distex^2 + distey^2 against 100 * sf[octave].  One ulp of the epipole moves the sum by about 80 ulps, so the aim is a random search, pre-selected by a float32
    model of `fl(fl(d*d) + fl(e*e))` against `fl(d*d + fl(e*e))`: the model only picks which calls are made, the two reference builds decide which are kept."""
    f = np.float32
    thr = f(100.0) * _f32_sf()[octave]
    ang = rng.uniform(0, 2 * np.pi, tries)
    r = np.sqrt(float(thr))
    tx = ((x2 + r * np.cos(ang) - CAM["cx"]) / CAM["fx"]).astype(f); ty = ((y2 + r * np.sin(ang) - CAM["cy"]) / CAM["fy"]).astype(f)
    d = (f(CAM["fx"]) * tx + f(CAM["cx"])) - f(x2); e = (f(CAM["fy"]) * ty + f(CAM["cy"])) - f(y2)
    plain = d * d + e * e
    fused = (d.astype(np.float64) * d.astype(np.float64) + (e * e).astype(np.float64)).astype(f)
    hit = np.nonzero((plain < thr) != (fused < thr))[0]
    return [np.array([tx[i], ty[i], 1.0], np.float32) for i in hit], tries


def _tri_candidates(rng, F):
    """SearchForTriangulation calls, one aimed pair (i, i) each: both key frames are made of the same image, so the pair has descriptor distance 0 and decides
    match12[i].  A generic F12 per call; F22 solved (in double) so that num*num/den of the pair sits at 3.84 * sigma2[octave], then stepped -3..+3 ulps.
    kind "line": the aimed node is small; "long": side 2's node holds more than 256 features (the kernel's second loop); "stereo": key frame 2 is the stereo one;
    "only_stereo": both stereo, bOnlyStereo; "epi": the line gate wide open (num = 0) and the epipole at its distance gate (_epipole_t2w)."""
    k = F["f1"].keys_un
    n = len(k)
    assert all(F[f].keys_un.tobytes() == k.tobytes() for f in ("f1b", "st", "stb")), "the same left image must give the same key points"
    stereo = F["st"].u_right >= 0
    sig2 = (_f32_sf() * _f32_sf()).astype(np.float64)               # mvLevelSigma2
    x, y = k["x"].astype(np.float64), k["y"].astype(np.float64)
    calls, tried = [], 0

    def fv(targets, others, full):
        """an aimed node per target (id 3 + g) = the target and others[g] more features; 40 further features in five nodes, or (full) every feature in forty nodes"""
        rest = rng.permutation(np.setdiff1d(np.arange(n), targets))
        if not full:
            rest = rest[:sum(others) + 40]
        node = rng.integers(10, 50 if full else 15, len(rest))
        node[:sum(others)] = np.repeat(3 + np.arange(len(targets)), others)
        ids = sorted(set(node.tolist()) | set(range(3, 3 + len(targets))))
        feats = [rng.permutation(np.concatenate([[targets[m - 3]], rest[node == m]]) if m < 10 else rest[node == m]) for m in ids]
        off = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int32)
        return np.array(ids, np.uint32), off, np.concatenate(feats).astype(np.uint32)

    def group(kind, targets, kf1, kf2, t2ws, open_line=False, only_stereo=False, check_ori=False, others2=6, full=False):
        """calls that share key frame 1 (its nodes and map-point flags), as the neighbours of one key frame do in LocalMapping: call j is aimed at targets[j % len]"""
        targets = [int(i) for i in targets]
        fv1 = fv(targets, [6] * len(targets), full)
        has1 = (rng.random(n) < 0.05).astype(np.uint8); has1[targets] = 0
        for j, t2w in enumerate(t2ws):
            g = j % len(targets); i = targets[g]
            Fm = (np.array([[0, -1e-4, 0.011], [1e-4, 0, -0.96], [-0.012, 0.97, 0.8]]) * (1 + 0.2 * rng.normal(0, 1, (3, 3))) + rng.normal(0, 2e-6, (3, 3))).astype(np.float32)
            G = Fm.astype(np.float64)
            a = x[i] * G[0, 0] + y[i] * G[1, 0] + G[2, 0]; b = x[i] * G[0, 1] + y[i] * G[1, 1] + G[2, 1]
            num = 0.0 if open_line else rng.choice([-1.0, 1.0]) * np.sqrt(3.84 * sig2[k["octave"][i]] * (a * a + b * b))
            f22 = np.array([num - (a * x[i] + b * y[i]) - (x[i] * G[0, 2] + y[i] * G[1, 2])], np.float32)
            if not open_line:
                f22 = (f22.view(np.int32) + np.int32(rng.integers(-3, 4))).view(np.float32)
            Fm[2, 2] = f22[0]
            has2 = (rng.random(n) < 0.05).astype(np.uint8); has2[targets] = 0
            calls.append(dict(kind=kind, i=i, kf1=kf1, kf2=kf2, fv1=fv1, fv2=fv(targets, [others2 if h == g else 6 for h in range(len(targets))], full), has1=has1, has2=has2,
                              F12=Fm, t2w=np.asarray(t2w, np.float32), only_stereo=only_stereo, check_ori=check_ori))

    far = lambda: np.array([rng.choice([-1, 1]) * rng.uniform(8, 15), rng.choice([-1, 1]) * rng.uniform(8, 15), 1.0])     # the epipole far outside the image
    fars = lambda m: [far() for _ in range(m)]
    mono, ster = np.nonzero(~stereo)[0], np.nonzero(stereo)[0]
    for j in range(25):                                            # (a call with every feature in a node costs the emulation 50 ms: a few only)
        group("line", rng.choice(n, 4, replace=False), "f1", "f1b", fars(4), check_ori=j % 4 == 0, full=j % 10 == 0)
    for j in range(8):
        group("long", rng.choice(n, 4, replace=False), "f1", "f1b", fars(4), others2=int(rng.integers(280, 420)))
    for j in range(6):
        group("stereo", rng.choice(n, 4, replace=False), "f1", "st", fars(4), check_ori=j % 3 == 0)
    for j in range(10):
        group("only_stereo", rng.choice(ster, 4, replace=False), "st", "stb", fars(4), only_stereo=True)
    for j in range(10):                                            # the epipole gate: mono-mono pairs (key frame 2 mono, or the mono features of the stereo one) ...
        i = rng.choice(mono)
        ts, t = _epipole_t2w(rng, k["x"][i], k["y"][i], k["octave"][i])
        tried += t
        group("epi", [i], "f1", "f1b" if j % 2 else "st", ts[:2], open_line=True)
    i = rng.choice(ster)                                           # ... and one stereo feature of key frame 2, which the gate must leave alone whatever the sum is
    ts, t = _epipole_t2w(rng, k["x"][i], k["y"][i], k["octave"][i])
    group("epi_stereo", [i], "f1", "st", ts[:1], open_line=True)
    return dict(calls=calls, epipoles_tried=tried + t)


def run(S, L, F, cases, which=ALL_MEMBERS):
    """every member on its cases through library L (frames F made by L) -> {member: output array}; "tri_calls": the outputs of "tri" call by call"""
    A, s12 = cases["A"], cases["s12"]
    S.set_test_poses(A, A, s12, None, None, library=L)
    try:
        res = {}
        for m in which:
            c = cases[m]
            if m == "tri":
                res["tri_calls"] = []
                for t in c["calls"]:
                    n, m12 = S.search_for_triangulation(F[t["kf1"]], t["has1"], t["fv1"], F[t["kf2"]], t["has2"], t["fv2"], t["F12"], t["t2w"], only_stereo=t["only_stereo"], check_ori=t["check_ori"])
                    res["tri_calls"].append(np.append(m12, np.int32(n)))
                res[m] = np.concatenate(res["tri_calls"]) if res["tri_calls"] else np.zeros(0, np.int32)
                continue
            if m == "sim3":
                S.set_test_poses(A, c["B"], s12, c["R12"], c["t12"], library=L)
                n, out = S.search_by_sim3(F["f0"], c["has1"], *c["P1"], c["level1"], c["desc1"], F["f1"], c["has2"], *c["P2"], c["level2"], c["desc2"], th=c["th"])
                S.set_test_poses(A, A, s12, None, None, library=L)
                res[m] = np.append(np.asarray(out, np.int32), np.int32(n))
                continue
            nq = len(c["X"])
            z8 = np.zeros(nq, np.uint8)
            if m == "reloc":
                n, out = S.search_by_projection_reloc(F["f1"], F["f0"], np.ones(nq, np.uint8), c["X"], c["Y"], c["Z"], c["level"], z8, z8, c["desc"], np.zeros(F["f1"].N, np.uint8),
                                                      th=c["th"], orb_dist=100, nnratio=0.9, check_ori=False)
            elif m in ("fuse", "fuse_stereo"):
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
    # SearchForTriangulation: the calls whose outputs differ, and two on which the builds agree (an aimed pair that stayed on one side of the line gate, and the
    # epipole aimed at a stereo feature); reloc / sim3 keep every point, like LAST_FRAME (one per feature: their claims interact)
    tri = cases["tri"]
    differ = [not np.array_equal(a, b) for a, b in zip(rn["tri_calls"], rc["tri_calls"])]
    agree = [[j for j, (d, t) in enumerate(zip(differ, tri["calls"])) if not d and t["kind"] == kind][:1] for kind in ("line", "epi_stereo")]
    assert agree[0] and agree[1], "no agreeing line call, or the model found no epipole at the gate of the stereo feature"
    cases["tri"] = dict(tri, calls=[t for j, t in enumerate(tri["calls"]) if differ[j] or j in agree[0] + agree[1]], candidates=len(tri["calls"]))
    return cases


def moved_new(cases, rn, rc):
    """outputs of the members added later that differ between the two reference builds: per member; SearchForTriangulation's by kind of call (match12 entries
    only: the return value moves with them and is not a gate decision of its own); SearchBySim3's by the pass that was aimed at the window's edge"""
    new = {m: int((rn[m] != rc[m]).sum()) for m in NEW_MEMBERS}
    kinds = {t["kind"]: 0 for t in cases["tri"]["calls"]}
    for t, a, b in zip(cases["tri"]["calls"], rn["tri_calls"], rc["tri_calls"]):
        kinds[t["kind"]] += int((a[:-1] != b[:-1]).sum())
    new["tri"] = sum(kinds.values())
    c = cases["sim3"]
    d = rn["sim3"][c["i1"]] != rc["sim3"][c["i1"]]
    new["sim3_pass1"], new["sim3_pass2"] = int((d & c["first"]).sum()), int((d & ~c["first"]).sum())
    return new, kinds


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
        new, tri_kind = moved_new(cases, rn, rc)
        with capsys.disabled():
            print("\nboundary cases: points " + ", ".join(f"{m} {len(cases[m]['X'])}" for m in MEMBERS) + f", reloc {len(cases['reloc']['X'])}, sim3 pairs {len(cases['sim3']['i1'])}" +
                  f", tri calls {len(cases['tri']['calls'])} of {cases['tri']['candidates']} ({cases['tri']['epipoles_tried']} epipoles modelled)" +
                  "; member outputs that differ between the native-flags and the canonical reference: " + ", ".join(f"{m} {moved[m]}" for m in MEMBERS) +
                  ", " + ", ".join(f"{m} {new[m]}" for m in NEW_MEMBERS) + f" (sim3 by aimed pass: {new['sim3_pass1']} / {new['sim3_pass2']}; tri = match12 entries, by kind of call: " + ", ".join(f"{k} {v}" for k, v in sorted(tri_kind.items())) + ")")
        assert sum(moved.values()) >= 20, moved                # the cases straddle gates: the two reference builds answer differently
        assert sum(moved[m] > 0 for m in MEMBERS) >= 3, moved
        assert new["tri"] >= 20 and tri_kind.get("long", 0) >= 1 and new["reloc"] >= 5 and new["sim3"] >= 5, (new, tri_kind)
        assert tri_kind.get("only_stereo", 0) >= 1 and tri_kind.get("stereo", 0) >= 1, tri_kind          # bOnlyStereo and a stereo key frame 2 are among the kept calls
        assert new["sim3_pass1"] >= 1 and new["sim3_pass2"] >= 1, new          # both projections of SearchBySim3's batch entry decide a moved output
        assert "epi_stereo" in tri_kind, tri_kind             # the epipole at the gate of a stereo feature is among the calls: `!bStereo1 && !bStereo2` seen from both sides
        assert tri_kind.get("epi", 0) >= 1, tri_kind           # the line gate of these calls is wide open: the epipole's distance gate moved them
        for m in ALL_MEMBERS:
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

