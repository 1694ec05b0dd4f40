"""What the entry points of the projection-guided search and of the best-in-window search promise about each other and about their arguments
(include/orbhip.h).  By the letters used below:
  projection search   sb orbhip_search_by_projection_bounds   pb orbhip_project_search_bounds   sf orbhip_search_by_projection_frame   pf orbhip_project_search_frame
                      sB orbhip_search_by_projection_batch
  window search       wb orbhip_search_best_in_window_bounds  pw orbhip_project_best_in_window_bounds   wf orbhip_search_best_in_window_frame
                      wB orbhip_search_best_in_window_batch   pB orbhip_project_best_in_window_batch    pS ..._shared   pH ..._held

  test_invalid_arguments / test_invalid_slot_of_a_batch / test_held_without_its_slot
                              ORBHIP_ERR_INVALID, and which outputs (handed in full of garbage) are reset: none by a one-frame call, those of the slots before the bad
                              one by a batch
  test_nothing_to_do_*        n == 0, nq == 0, no slots, only empty slots: ORBHIP_OK, outputs reset; the shared form without a live slot, then the held one
  test_single_is_a_batch_of_one_*   byte for byte
  test_slot_shapes_*          batches whose slots differ in nq (1, 4, 5, 257), in n (63, 64, 65, all), with empty slots, with different bounds, with the select kernel's
                              tables in device memory: every slot equals its own one-frame call
  test_resident_frame         the _frame entries equal the _bounds entries on the fetched arrays: frames 0 and 1 of a pair, and the frame of a single-image extraction
                              before and after its grid is built behind the extraction
  test_interleaved            shared, held, one-frame projection search, held (ORBHIP_ERR_INVALID), shared, held on one thread: every answer equals the call made alone
  test_records                emulation only: which entry points write ORBHIP_TEST_RECORD records, and their bytes"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_slam2_amd  # noqa: E402
from orb_slam2_amd import orbhip as H  # noqa: E402
from orb_slam2_amd import synth  # noqa: E402
from test_parity_projection import _queries  # noqa: E402

W, HT, FX, FY, CX, CY = 320, 240, 300.0, 300.0, 160.0, 120.0
GARBAGE = 0x5a5a5a5a
FULL, SHIFTED = (0.0, 0.0, float(W), float(HT)), (-7.5, 3.25, W + 11.0, HT + 2.5)
PROJ_KINDS, WIN_KINDS = (H.PROJ_LAST_FRAME, H.PROJ_FRAME_KF, H.PROJ_KF_SIM3), (H.PROJ_FUSE, H.PROJ_FUSE_SIM3, H.PROJ_SIM3)      # what the members of each family use
PROJ, WIN = ("sb", "pb", "sf", "pf", "sB"), ("wb", "pw", "wf", "wB", "pB", "pS", "pH")
FAMILY = {**{e: "proj" for e in PROJ}, **{e: "win" for e in WIN}}
POINTS = ("pb", "pf", "pw", "pB", "pS", "pH")                        # the entry points that project map points on the device


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(oracle):
    """two oracle-extracted frames; the queries and map points play the last frame's key points seen from the current one.  Read-only: the tests share it."""
    S = Scene()
    S.images = synth.sequence(W, HT, 2, seed=41)
    ora = oracle.OracleExtractor(500, 1.2, 8, 20, 7)
    (S.kl, S.dl), (S.kc, S.dc) = ora.extract(S.images[0]), ora.extract(S.images[1])
    S.sf = ora.params()["scale_factors"]
    assert 300 <= len(S.kl) <= 600 and 300 <= len(S.kc) <= 600
    rng = np.random.default_rng(5)
    tup = (W, HT, S.sf, (S.kl, S.dl), (S.kc, S.dc))
    S.q = {mode: _queries(oracle, tup, mode, th, rng, rule) for mode, th, rule in ((0, 4.0, "local_map"), (1, 7.0, "window"))}
    S.inv = (1.0 / (S.sf * S.sf)).astype(np.float32)
    S.ur = np.where(rng.random(len(S.kc)) < 0.6, S.kc["x"] - rng.uniform(8, 10, len(S.kc)), -1).astype(np.float32)
    S.bl = (rng.random(len(S.kc)) < 0.15).astype(np.uint8)
    nq = len(S.kl)
    bq = np.zeros(nq, H.BEST_QUERY_DTYPE)
    bq["x"] = S.kl["x"] - 3.0 + rng.normal(0, 1.2, nq).astype(np.float32); bq["y"] = S.kl["y"] - 1.0 + rng.normal(0, 1.2, nq).astype(np.float32)
    bq["level"] = np.clip(S.kl["octave"] + rng.integers(0, 2, nq), 0, 7); bq["radius"] = (np.float32(5.0) * S.sf[bq["level"]]).astype(np.float32); bq["ur"] = bq["x"] - np.float32(9.0)
    S.bq = bq
    # map points: the last frame's key points moved by the image motion, at depths of 2..8 in a camera at the origin (R = I, t = 0: every kind projects them alike)
    z = rng.uniform(2, 8, nq); u = S.kl["x"] - 3.0 + rng.normal(0, 1.0, nq); v = S.kl["y"] - 1.0 + rng.normal(0, 1.0, nq)
    z[:4] *= -1.0                                                     # behind the camera
    pts = np.zeros(nq, H.MAP_POINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = (u - CX) / FX * z, (v - CY) / FY * z, z
    p = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(np.float64); d = np.linalg.norm(p, axis=1)
    pts["cam_x"], pts["cam_y"], pts["cam_z"] = pts["x"], pts["y"], pts["z"]
    pts["nx"], pts["ny"], pts["nz"] = (p / d[:, None]).T
    pts["scale_dist"] = (d * S.sf[S.kl["octave"]]).astype(np.float32) * np.float32(0.97); pts["min_dist"] = 0.0; pts["max_dist"] = 1e30
    pts["level"] = -1; pts["blocks"] = rng.random(nq) < 0.9; pts["angle"] = S.kl["angle"]
    S.pts = pts
    S.lr = None                                                      # PredictScale's thresholds: derived once, by the library under test
    return S


def _lr(S, lib):
    if S.lr is None:
        S.lr = H.predict_scale_table(np.float32(np.log(np.float32(1.2))), 8, library=lib)
    return S.lr


def _proj(S, lib, kind, bounds=FULL, gemm=0, fc=0, th=5.0):
    eye = np.eye(3, dtype=np.float32)
    return H.make_projection(kind, eye, np.zeros(3), FX, FY, CX, CY, bounds, th, S.sf, _lr(S, lib), bf=40.0, R2=eye, t2=np.zeros(3), gemm_mode=gemm, fp_contract=fc)


def _pts(S, kind):
    pts = S.pts.copy()
    if kind == H.PROJ_LAST_FRAME:
        pts["level"] = S.kl["octave"]
    return pts


def _c(v):
    return H._p(v) if isinstance(v, np.ndarray) else (C.byref(v) if isinstance(v, C.Structure) else v)


def _addr(v):
    return None if v is None else (H._p(v).value if isinstance(v, np.ndarray) and len(v) else None)


def _garbage(n, dtype=np.int32):
    a = np.empty(max(n, 1), dtype)
    a.view(np.uint8)[:] = 0x5a
    return a


def args(S, lib, e, **over):
    """the arguments of one frame / slot of entry point e by name, every one replaceable (`n=-1`, `fq=None`, ...); outputs handed in full of garbage"""
    fam, points = FAMILY[e], e in POINTS
    a = dict(kps=S.kc, desc=S.dc, ur=None, bl=None, n=len(S.kc), bounds=H.Bounds.of(FULL), mode=0, nnratio=0.8, th=100, ori=1, chi2=0, inv=S.inv, nlev=len(S.inv),
             frame=0, use_ur=0, kind=H.PROJ_KF_SIM3 if fam == "proj" else H.PROJ_FUSE, gemm=0, fc=0)
    a.update({k: over.pop(k) for k in list(over) if k in ("kind", "gemm", "fc", "mode")})
    if points:
        a.update(proj=_proj(S, lib, a["kind"], gemm=a["gemm"], fc=a["fc"]), pts=_pts(S, a["kind"]), qd=S.dl)
    elif fam == "proj":
        a.update(pts=S.q.get(a["mode"], S.q[0])[0], qd=S.q.get(a["mode"], S.q[0])[1])
    else:
        a.update(pts=S.bq, qd=S.dl)
    a.update(over)
    a.setdefault("nq", len(a["pts"]) if a["pts"] is not None else 0)
    if fam == "proj":
        a.setdefault("fq", _garbage(a["n"])); a.setdefault("nm", C.c_int(GARBAGE)); a.setdefault("qo", _garbage(a["nq"], H.PROJ_QUERY_DTYPE) if e in ("pb", "pf") else None)
    else:
        a.setdefault("bi", _garbage(a["nq"])); a.setdefault("bd", _garbage(a["nq"])); a.setdefault("qo", _garbage(a["nq"], H.BEST_QUERY_DTYPE) if e == "pw" else None)
    return a


def call(L, e, a, ctx=None, slots=None, nslots=None, skip=None, slot=0, device=0):
    """one entry point on the arguments of args() (the batch forms: on a list of them) -> status"""
    g = lambda k: _c(a[k])
    if e == "sb":
        return L.orbhip_search_by_projection_bounds(device, g("kps"), g("desc"), g("ur"), g("bl"), a["n"], g("bounds"), g("pts"), g("qd"), a["nq"], a["mode"], a["nnratio"], a["th"], a["ori"], g("fq"), g("nm"))
    if e == "pb":
        return L.orbhip_project_search_bounds(device, g("kps"), g("desc"), g("ur"), g("bl"), a["n"], g("bounds"), g("proj"), g("pts"), g("qd"), a["nq"], a["nnratio"], a["th"], a["ori"], g("fq"), g("nm"), g("qo"))
    if e == "sf":
        return L.orbhip_search_by_projection_frame(ctx, a["frame"], a["n"], a["use_ur"], g("bl"), g("pts"), g("qd"), a["nq"], a["mode"], a["nnratio"], a["th"], a["ori"], g("fq"), g("nm"))
    if e == "pf":
        return L.orbhip_project_search_frame(ctx, a["frame"], a["n"], a["use_ur"], g("bl"), g("proj"), g("pts"), g("qd"), a["nq"], a["nnratio"], a["th"], a["ori"], g("fq"), g("nm"), g("qo"))
    if e == "wb":
        return L.orbhip_search_best_in_window_bounds(device, g("kps"), g("desc"), g("ur"), a["n"], g("bounds"), g("inv"), a["nlev"], g("pts"), g("qd"), a["nq"], a["chi2"], g("bi"), g("bd"))
    if e == "pw":
        return L.orbhip_project_best_in_window_bounds(device, g("kps"), g("desc"), g("ur"), a["n"], g("bounds"), g("inv"), a["nlev"], g("proj"), g("pts"), g("qd"), a["nq"], a["chi2"], g("bi"), g("bd"), g("qo"))
    if e == "wf":
        return L.orbhip_search_best_in_window_frame(ctx, a["frame"], a["n"], a["use_ur"], g("pts"), g("qd"), a["nq"], a["chi2"], g("bi"), g("bd"))
    if e == "pH":
        return L.orbhip_project_best_in_window_held(device, slot, g("proj"), g("pts"), g("qd"), a["nq"], a["chi2"], g("bi"), g("bd"))
    slots = [a] if slots is None else slots
    nslots = len(slots) if nslots is None else nslots
    a0 = slots[0] if slots else a
    if e == "sB":
        arr = (H.ProjSlot * max(len(slots), 1))()
        for k, s in enumerate(slots):
            arr[k] = H.ProjSlot(_addr(s["kps"]), _addr(s["desc"]), _addr(s["ur"]), _addr(s["bl"]), s["n"], _addr(s["pts"]), _addr(s["qd"]), s["nq"], _addr(s["fq"]), GARBAGE)
        st = L.orbhip_search_by_projection_batch(device, nslots, arr if slots else None, _c(a0["bounds"]), a0["mode"], a0["nnratio"], a0["th"], a0["ori"])
        for k, s in enumerate(slots):
            s["nm"] = C.c_int(arr[k].nmatches)
        return st
    if e == "wB":
        arr = (H.BestSlot * max(len(slots), 1))()
        for k, s in enumerate(slots):
            arr[k] = H.BestSlot(_addr(s["kps"]), _addr(s["desc"]), _addr(s["ur"]), s["n"], s["bounds"], _addr(s["inv"]), s["nlev"], _addr(s["pts"]), _addr(s["qd"]), s["nq"], _addr(s["bi"]), _addr(s["bd"]))
        return L.orbhip_search_best_in_window_batch(device, nslots, arr if slots else None, a0["chi2"])
    arr = (H.ProjectBestSlot * max(len(slots), 1))()
    for k, s in enumerate(slots):
        arr[k] = H.ProjectBestSlot(_addr(s["kps"]), _addr(s["desc"]), _addr(s["ur"]), s["n"], s["bounds"], _addr(s["inv"]), s["nlev"], C.pointer(s["proj"]) if s.get("proj") is not None else None,
                                   _addr(s["pts"]), _addr(s["qd"]), s["nq"], _addr(s["bi"]), _addr(s["bd"]))
    if e == "pB":
        return L.orbhip_project_best_in_window_batch(device, nslots, arr if slots else None, a0["chi2"])
    assert e == "pS"
    return L.orbhip_project_best_in_window_shared(device, nslots, arr if slots else None, _c(skip), a0["chi2"])


def untouched(a):
    return all(np.all(a[k].view(np.uint8) == 0x5a) for k in ("fq", "bi", "bd", "qo") if a.get(k) is not None) and ("nm" not in a or a["nm"] is None or a["nm"].value == GARBAGE)


def was_reset(a):
    """the state a call leaves its outputs in before it searches: no match anywhere, every derived query gated out"""
    ok = True
    if a.get("fq") is not None:
        ok = ok and np.all(a["fq"][:a["n"]] == -1) and a["nm"].value == 0
    if a.get("bi") is not None:
        ok = ok and np.all(a["bi"][:a["nq"]] == -1) and np.all(a["bd"][:a["nq"]] == 256)
    if a.get("qo") is not None and a["nq"] > 0:
        qo = a["qo"][:a["nq"]]
        ok = ok and np.all(qo["radius"] == -1.0) and np.all(qo["x"] == 0.0) and all(np.all(qo[f] == 0) for f in qo.dtype.names if f != "radius")
    return bool(ok)


@pytest.fixture(scope="module")
def contexts(scene):
    """contexts(lib) -> the handle of a context whose last extraction was the scene's two frames (no stereo columns): one per library, closed behind the module"""
    made = {}

    def get(lib):
        if lib not in made:
            made[lib] = H.ORBextractor(500, 1.2, 8, 20, 7, W, HT, max_batch=2, library=lib)
            made[lib].extract_batch(scene.images)
        return made[lib].h
    yield get
    for ext in made.values():
        ext.close()


def _bad_proj(S, lib, **f):
    P = _proj(S, lib, H.PROJ_FUSE)
    for k, v in f.items():
        setattr(P, k, v)
    return P


# name -> (arguments replaced, the entry points it applies to)
INVALID = {
    "null fq": (dict(fq=None), PROJ), "null nmatches": (dict(nm=None), ("sb", "pb", "sf", "pf")), "null best_idx": (dict(bi=None), WIN), "null best_dist": (dict(bd=None), WIN),
    "null query_desc": (dict(qd=None), PROJ + WIN), "null queries": (dict(pts=None, nq=7), PROJ + WIN), "null kps": (dict(kps=None), ("sb", "pb", "sB", "wb", "pw", "wB", "pB", "pS")),
    "null bounds": (dict(bounds=None), ("sb", "pb", "sB", "wb", "pw")),
    "n<0": (dict(n=-1), ("sb", "pb", "sf", "pf", "sB", "wb", "pw", "wf", "wB", "pB", "pS")), "nq<0": (dict(nq=-1), PROJ + WIN),
    "inverted x": (dict(bounds=H.Bounds(10.0, 0.0, 10.0, 240.0)), ("sb", "pb", "sB", "wb", "pw", "wB", "pB", "pS")),
    "inverted y": (dict(bounds=H.Bounds(0.0, 240.0, 320.0, 0.0)), ("sb", "pb", "sB", "wb", "pw", "wB", "pB", "pS")),
    "mode 2": (dict(mode=2), ("sb", "sf", "sB")),
    "kind 6": (dict(P=dict(kind=6)), POINTS), "kind bit": (dict(P=dict(kind=H.PROJ_FUSE | 0x200)), POINTS), "gemm_mode 3": (dict(P=dict(gemm_mode=3)), POINTS),
    "nlevels 0": (dict(P=dict(nlevels=0)), POINTS), "nlevels 17": (dict(P=dict(nlevels=17)), POINTS), "null proj": (dict(proj=None), POINTS),
    "chi2 without sigma": (dict(chi2=1, inv=None), ("wb", "pw", "wB", "pB", "pS")), "chi2 without levels": (dict(chi2=1, nlev=0), ("wb", "pw", "wB", "pB", "pS")),
    "frame 2": (dict(frame=2), ("sf", "pf", "wf")), "frame -1": (dict(frame=-1), ("sf", "pf", "wf")), "n beyond capacity": (dict(n=1 << 20), ("sf", "pf", "wf")),
    "no stereo columns": (dict(use_ur=1), ("sf", "pf", "wf")), "null context": (dict(), ("sf", "pf", "wf")),
}
CASES = [(name, e) for name, (_, es) in INVALID.items() for e in es]


@pytest.mark.parametrize("name,e", CASES, ids=[f"{n}-{e}" for n, e in CASES])
def test_invalid_arguments(backend, scene, contexts, name, e):
    L = H.lib(backend)
    over = dict(INVALID[name][0])
    if "P" in over:
        over = dict(proj=_bad_proj(scene, backend, **over["P"]))
    a = args(scene, backend, e, **over)
    if e == "pH":                                                    # a valid shared call first: the held call's own arguments are what is wrong
        assert call(L, "pS", args(scene, backend, "pS", **_cut(args(scene, backend, "pS"), n=64, nq=40))) == H.OK
    st = call(L, e, a, ctx=None if name == "null context" or e not in ("sf", "pf", "wf") else contexts(backend))
    assert st == H.ERR_INVALID and L.orbhip_last_error() and untouched(a)


# what is wrong with slot 1 of three -> the entry points after which slot 0 has been reset (the others refuse the call before they reset anything: the window
# batches look for a slot's queries / points before the slots are walked, the shared form for slot 0's points and descriptors in every slot)
BAD_SLOT = {"n<0": (dict(n=-1), ("sB", "wB", "pB", "pS")), "null queries": (dict(pts=None), ("sB",)), "null query_desc": (dict(qd=None), ("sB", "wB", "pB"))}


@pytest.mark.parametrize("bad", list(BAD_SLOT))
@pytest.mark.parametrize("e", ["sB", "wB", "pB", "pS"])
def test_invalid_slot_of_a_batch(backend, scene, e, bad):
    """the slots before the bad one are reset where the walk over the slots found it, the bad one and those behind it are left alone"""
    L = H.lib(backend)
    pts = args(scene, backend, e)
    same = dict(pts=pts["pts"], qd=pts["qd"], nq=pts["nq"])          # (the shared form: every slot names slot 0's points)
    s = [args(scene, backend, e, **same), args(scene, backend, e, **{**same, **BAD_SLOT[bad][0]}), args(scene, backend, e, **same)]
    assert call(L, e, None, slots=s) == H.ERR_INVALID and L.orbhip_last_error()
    assert (was_reset(s[0]) if e in BAD_SLOT[bad][1] else untouched(s[0])) and untouched(s[1]) and untouched(s[2])
    assert call(L, e, s[0], slots=[], nslots=-1) == H.ERR_INVALID
    assert call(L, e, s[0], slots=[], nslots=1) == H.ERR_INVALID    # slots without an array


def test_shared_slot_rules(backend, scene):
    """65 slots; a slot naming other points; ORBHIP_FP_CONTRACT in one slot only (batch and shared)"""
    L = H.lib(backend)
    a = args(scene, backend, "pS")
    same = dict(pts=a["pts"], qd=a["qd"])
    many = [args(scene, backend, "pS", **same) for _ in range(65)]
    assert call(L, "pS", None, slots=many) == H.ERR_INVALID and all(untouched(s) for s in many)
    other = [args(scene, backend, "pS", **same), args(scene, backend, "pS", pts=a["pts"].copy(), qd=a["qd"])]
    assert call(L, "pS", None, slots=other) == H.ERR_INVALID and all(untouched(s) for s in other)
    for e in ("pB", "pS"):
        mixed = [args(scene, backend, "pS", **same), args(scene, backend, "pS", fc=1, **same)]
        assert call(L, e, None, slots=mixed) == H.ERR_INVALID and b"ORBHIP_FP_CONTRACT" in L.orbhip_last_error()
        assert was_reset(mixed[0]) and untouched(mixed[1])


def test_held_without_its_slot(backend, scene):
    L = H.lib(backend)
    mk = lambda **o: args(scene, backend, "pH", **o)
    assert call(L, "wb", args(scene, backend, "wb")) == H.OK            # the thread's last scratch-using call is not a shared one
    a = mk()
    assert call(L, "pH", a) == H.ERR_INVALID and untouched(a)
    s = mk()
    assert call(L, "pS", None, slots=[s]) == H.OK
    for kw in (dict(device=1), dict(slot=1), dict(slot=-1)):        # another device number, a slot the shared call did not have
        a = mk()
        assert call(L, "pH", a, **kw) == H.ERR_INVALID and untouched(a)
    a = mk()
    assert call(L, "pH", a) == H.OK and np.array_equal(a["bi"], s["bi"]) and np.array_equal(a["bd"], s["bd"])
    # a shared call that offered no points: a slot with key points never travelled (-2, outputs reset first), a slot without answers -1 / 256
    none = dict(pts=scene.pts[:0], qd=scene.dl[:0], nq=0)
    s = [mk(**none), mk(n=0, **none)]
    assert call(L, "pS", None, slots=s) == H.OK
    a = mk()
    assert call(L, "pH", a, slot=0) == H.ERR_INVALID and was_reset(a)
    a = mk()
    assert call(L, "pH", a, slot=1) == H.OK and was_reset(a)


@pytest.mark.parametrize("empty", ["n", "nq"])
@pytest.mark.parametrize("e", PROJ + WIN)
def test_nothing_to_do_in_one_frame(backend, scene, contexts, e, empty):
    L = H.lib(backend)
    over = dict(n=0) if empty == "n" else dict(nq=0)
    if e not in ("sf", "pf", "wf"):
        over.update(dict(kps=None, desc=None) if empty == "n" else dict(pts=None, qd=None))
    a = args(scene, backend, e, **over)
    if e == "pH":                                                    # (a held call names no key frame: the shared call's slot is the empty one)
        assert call(L, "pS", args(scene, backend, "pS", **(dict(n=0) if empty == "n" else {}))) == H.OK
    assert call(L, e, a, ctx=contexts(backend) if e in ("sf", "pf", "wf") else None) == H.OK and was_reset(a)
    if a.get("fq") is not None:
        assert np.all(a["fq"][a["n"]:] == GARBAGE)                   # nothing beyond n is written


@pytest.mark.parametrize("e", ["sB", "wB", "pB", "pS"])
def test_nothing_to_do_in_a_batch(backend, scene, e):
    L = H.lib(backend)
    a = args(scene, backend, e)
    assert call(L, e, a, slots=[], nslots=0) == H.OK                 # no slots
    none = dict(pts=a["pts"][:0], qd=a["qd"][:0], nq=0)
    s = [args(scene, backend, e, n=0, **(none if e == "pS" else {})), args(scene, backend, e, **none)]
    assert call(L, e, None, slots=s) == H.OK and was_reset(s[0]) and was_reset(s[1])


def _same(a, b, keys):
    return all((a[k].value == b[k].value) if k == "nm" else (a[k].tobytes() == b[k].tobytes()) for k in keys)


@pytest.mark.parametrize("stereo,blocked", [(False, False), (True, True)])
@pytest.mark.parametrize("ori", [1, 0])
@pytest.mark.parametrize("mode", [0, 1])
def test_single_is_a_batch_of_one_projection(backend, scene, select_tables, mode, ori, stereo, blocked):
    L = H.lib(backend)
    mk = lambda: args(scene, backend, "sb", mode=mode, ori=ori, ur=scene.ur if stereo else None, bl=scene.bl if blocked else None, nnratio=0.8 if mode == 0 else 0.9)
    one, b = mk(), mk()
    assert call(L, "sb", one) == H.OK and call(L, "sB", b) == H.OK
    assert one["nm"].value > 50 and _same(one, b, ("fq", "nm"))


@pytest.mark.parametrize("bounds", [FULL, SHIFTED])
@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("chi2", [0, 1])
def test_single_is_a_batch_of_one_window(backend, scene, chi2, stereo, bounds):
    L = H.lib(backend)
    mk = lambda: args(scene, backend, "wb", chi2=chi2, ur=scene.ur if stereo else None, bounds=H.Bounds.of(bounds))
    one, b = mk(), mk()
    assert call(L, "wb", one) == H.OK and call(L, "wB", b) == H.OK
    assert int((one["bd"] <= 50).sum()) > 100 and _same(one, b, ("bi", "bd"))


@pytest.mark.parametrize("gemm", [0, 1])
@pytest.mark.parametrize("fc", [0, 1])
@pytest.mark.parametrize("kind", WIN_KINDS)
def test_single_is_a_batch_of_one_projected_window(backend, scene, kind, fc, gemm):
    L = H.lib(backend)
    mk = lambda: args(scene, backend, "pw", kind=kind, fc=fc, gemm=gemm, chi2=int(kind == H.PROJ_FUSE), ur=scene.ur)
    one, b, sh = mk(), mk(), mk()
    assert call(L, "pw", one) == H.OK and call(L, "pB", b) == H.OK and call(L, "pS", sh, skip=np.zeros(sh["nq"], np.uint64)) == H.OK
    assert int((one["bd"] <= 50).sum()) > 100 and np.all(one["qo"]["radius"][:4] == -1.0) and np.any(one["qo"]["radius"] > 0)
    assert _same(one, b, ("bi", "bd")) and _same(one, sh, ("bi", "bd"))


def _cut(a, n=None, nq=None):
    """the slot's arguments with the first n key points / nq queries only"""
    o = {}
    if n is not None:
        o.update(kps=a["kps"][:n].copy(), desc=a["desc"][:n].copy(), n=n, ur=None if a["ur"] is None else a["ur"][:n].copy(), bl=None if a["bl"] is None else a["bl"][:n].copy())
    if nq is not None:
        o.update(pts=a["pts"][:nq].copy(), qd=a["qd"][:nq].copy(), nq=nq)
    return o


def _slots_equal_their_own_calls(L, S, lib, single, batch, shapes, keys, **common):
    mk = lambda e, shape: args(S, lib, e, **{**common, **_cut(args(S, lib, e, **common), **shape)})
    slots, alone = [mk(batch, s) for s in shapes], [mk(single, s) for s in shapes]
    assert call(L, batch, None, slots=slots) == H.OK
    for s, a in zip(slots, alone):
        assert call(L, single, a) == H.OK and _same(s, a, keys), (s["n"], s["nq"])
        if s["n"] == 0 or s["nq"] == 0:
            assert was_reset(s)
    return slots


NQ_SHAPES = [dict(nq=1), dict(nq=4), dict(nq=5), dict(nq=257)]
N_SHAPES = [dict(n=63), dict(n=64), dict(n=65), dict()]
EMPTY_SHAPES = [dict(n=0), dict(nq=200), dict(nq=0), dict(n=100), dict(n=0)]


@pytest.mark.parametrize("shapes", [NQ_SHAPES, N_SHAPES, EMPTY_SHAPES], ids=["nq", "n", "empty"])
def test_slot_shapes_projection(backend, scene, select_tables, shapes):
    L = H.lib(backend)
    s = _slots_equal_their_own_calls(L, scene, backend, "sb", "sB", shapes, ("fq", "nm"), mode=1, nnratio=0.9, ur=scene.ur, bl=scene.bl)
    assert sum(x["nm"].value for x in s) > 20


@pytest.mark.parametrize("shapes", [NQ_SHAPES, N_SHAPES, EMPTY_SHAPES], ids=["nq", "n", "empty"])
@pytest.mark.parametrize("form", ["wB", "pB"])
def test_slot_shapes_window(backend, scene, form, shapes):
    L = H.lib(backend)
    s = _slots_equal_their_own_calls(L, scene, backend, "wb" if form == "wB" else "pw", form, shapes, ("bi", "bd"), chi2=1, ur=scene.ur)
    assert sum(int((x["bd"][:x["nq"]] <= 50).sum()) for x in s) > 20


@pytest.mark.parametrize("equal", [True, False])
def test_slot_shapes_window_bounds(backend, scene, equal):
    """five slots: one k_match_grid launch for equal bounds, one per slot for pairwise different ones"""
    L = H.lib(backend)
    mk = lambda k: args(scene, backend, "wb", bounds=H.Bounds.of(SHIFTED if equal else (-2.0 * k, -1.0 * k, W + 3.0 * k, HT + 1.5 * k)), **_cut(args(scene, backend, "wb"), n=len(scene.kc) - 37 * k))
    slots, alone = [mk(k) for k in range(5)], [mk(k) for k in range(5)]
    assert call(L, "wB", None, slots=slots) == H.OK
    for s, a in zip(slots, alone):
        assert call(L, "wb", a) == H.OK and _same(s, a, ("bi", "bd")) and int((a["bd"] <= 50).sum()) > 100


def test_resident_frame(backend, scene):
    """the _frame entries on frames 0 and 1 of a pair, then on the frame of single-image extractions: the first search there asks for the grid, the extraction after it
    builds the grid behind itself and the searches after that take it"""
    L = H.lib(backend)
    ext = H.ORBextractor(500, 1.2, 8, 20, 7, W, HT, max_batch=2, library=backend)
    b = H.Bounds.of(ext.bounds())
    inv = ext.GetInverseScaleSigmaSquares()
    q, qd = scene.q[1]

    def check(frame, kps, desc):
        n = len(kps)
        ur, bl = np.resize(scene.ur, n), np.resize(scene.bl, n)
        ext.set_stereo_columns(ur, frame=frame)
        for use_ur in (False, True):
            nm, fq = ext.search_by_projection(frame, n, q, qd, 1, nnratio=0.9, use_u_right=use_ur, blocked=bl)
            nm0, fq0 = orb_slam2_amd.search_by_projection(kps, desc, W, HT, q, qd, 1, nnratio=0.9, u_right=ur if use_ur else None, blocked=bl, library=backend, bounds=b)
            assert nm == nm0 and nm > 50 and np.array_equal(fq, fq0)
        bi, bd = ext.search_best_in_window(frame, n, scene.bq, scene.dl, True, use_u_right=True)
        bi0, bd0 = orb_slam2_amd.search_best_in_window(kps, desc, W, HT, inv, scene.bq, scene.dl, True, u_right=ur, library=backend, bounds=b)
        assert np.array_equal(bi, bi0) and np.array_equal(bd, bd0) and int((bd <= 50).sum()) > 100
        a, a0 = (args(scene, backend, e, kps=kps, desc=desc, n=n, frame=frame, kind=H.PROJ_LAST_FRAME, bounds=b, mode=1) for e in ("pf", "pb"))
        assert call(L, "pf", a, ctx=ext.h) == H.OK and call(L, "pb", a0) == H.OK and a["nm"].value > 50 and _same(a, a0, ("fq", "nm", "qo"))

    k, d = ext.extract_batch(scene.images)
    check(0, k[0], d[0]); check(1, k[1], d[1])
    k, d = ext.extract_batch(scene.images[1:])
    check(0, k[0], d[0])                                             # asks for the grid
    k, d = ext.extract_batch(scene.images[1:])
    check(0, k[0], d[0]); check(0, k[0], d[0])                       # finds it, and again
    ext.close()


def test_interleaved(backend, scene):
    L = H.lib(backend)
    same = dict(pts=_pts(scene, H.PROJ_FUSE), qd=scene.dl)
    shared = lambda e: [args(scene, backend, e, chi2=1, **same, **_cut(args(scene, backend, e), n=n)) for n in (len(scene.kc), 200, 0)]
    other = lambda: args(scene, backend, "pH", chi2=1, pts=_pts(scene, H.PROJ_FUSE)[50:180].copy(), qd=scene.dl[50:180].copy())
    alone = []
    for n in (len(scene.kc), 200):                                   # the held calls made alone: the one-frame entry on that slot's key frame
        a = args(scene, backend, "pw", chi2=1, pts=other()["pts"], qd=other()["qd"], **_cut(args(scene, backend, "pw"), n=n))
        assert call(L, "pw", a) == H.OK
        alone.append(a)
    s_alone = shared("pw")
    for s in s_alone:
        assert call(L, "pw", s) == H.OK
    p_alone = args(scene, backend, "sb", mode=1, nnratio=0.9)
    assert call(L, "sb", p_alone) == H.OK and p_alone["nm"].value > 50

    s1, h1, p, h2, s2, h3, h4 = shared("pS"), other(), args(scene, backend, "sb", mode=1, nnratio=0.9), other(), shared("pS"), other(), other()
    skip = np.zeros(s1[0]["nq"], np.uint64)
    assert call(L, "pS", None, slots=s1, skip=skip) == H.OK
    assert call(L, "pH", h1, slot=1) == H.OK
    assert call(L, "sb", p) == H.OK
    assert call(L, "pH", h2, slot=1) == H.ERR_INVALID and untouched(h2)
    assert call(L, "pS", None, slots=s2, skip=skip) == H.OK
    assert call(L, "pH", h3, slot=0) == H.OK and call(L, "pH", h4, slot=2) == H.OK
    for s, t, a in zip(s1, s2, s_alone):
        assert _same(s, a, ("bi", "bd")) and _same(t, a, ("bi", "bd"))
    assert int((s_alone[0]["bd"] <= 50).sum()) > 100 and was_reset(s1[2])
    assert _same(h1, alone[1], ("bi", "bd")) and _same(h3, alone[0], ("bi", "bd")) and int((h3["bd"] <= 50).sum()) > 30
    assert was_reset(h4)                              # the slot without key points
    assert _same(p, p_alone, ("fq", "nm"))


def _rec(tag, *arrays):
    out = [np.int32(tag).tobytes()]
    for a in arrays:
        raw = b"" if a is None else (bytes(a) if isinstance(a, C.Structure) else np.ascontiguousarray(a).tobytes())
        out.append(np.int64(-1 if a is None else len(raw)).tobytes() + raw)
    return b"".join(out)


def test_records(emu_lib, scene, tmp_path, monkeypatch):
    L = H.lib(emu_lib)
    ext = H.ORBextractor(500, 1.2, 8, 20, 7, W, HT, max_batch=2, library=emu_lib)
    k, d = ext.extract_batch(scene.images)
    f = tmp_path / "rec.bin"

    def recorded(e, a, **kw):
        f.write_bytes(b"")
        monkeypatch.setenv("ORBHIP_TEST_RECORD", str(f))
        st = call(L, e, a, **kw)
        monkeypatch.delenv("ORBHIP_TEST_RECORD")
        assert st == H.OK
        return f.read_bytes()

    a = args(scene, emu_lib, "pb", kind=H.PROJ_LAST_FRAME, ur=scene.ur, bl=scene.bl, nnratio=0.9, th=90, ori=1)
    got = recorded("pb", a)
    assert a["nm"].value > 50
    assert got == _rec(1, a["kps"], a["desc"], a["ur"], a["bl"], a["bounds"], a["proj"], a["pts"], a["qd"], np.array([0.9, 0.0], np.float32), np.array([90, 1, a["nm"].value], np.int32), a["fq"][:a["n"]])
    mk = lambda **o: args(scene, emu_lib, "pB", chi2=1, **o)
    s = [mk(ur=scene.ur), mk(n=0), mk(fc=0, kind=H.PROJ_FUSE_SIM3, **_cut(mk(), n=200, nq=90))]
    got = recorded("pB", None, slots=s)
    assert got == b"".join(_rec(2, x["kps"], x["desc"], x["ur"], x["bounds"], x["inv"], x["proj"], x["pts"], x["qd"], np.array([1], np.int32), x["bi"][:x["nq"]], x["bd"][:x["nq"]]) for x in (s[0], s[2]))
    # the resident form of the projected search: one tag-1 record too, of the arrays where the extraction left them
    n = len(k[0])
    a = args(scene, emu_lib, "pf", kind=H.PROJ_LAST_FRAME, n=n, bounds=H.Bounds.of(ext.bounds()), nnratio=0.9)
    got = recorded("pf", a, ctx=ext.h)
    assert got == _rec(1, k[0], d[0], None, None, a["bounds"], a["proj"], a["pts"], a["qd"], np.array([0.9, 0.0], np.float32), np.array([100, 1, a["nm"].value], np.int32), a["fq"][:n])
    # every other entry point: nothing
    for e in ("sb", "sf", "sB", "wb", "pw", "wf", "wB", "pS", "pH"):
        assert recorded(e, args(scene, emu_lib, e, n=n if e in ("sf", "wf") else len(scene.kc)), ctx=ext.h) == b"", e
    ext.close()
