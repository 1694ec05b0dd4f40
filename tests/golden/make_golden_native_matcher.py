"""Freezes the boundary-straddling matcher cases of tests/test_native_flags_matcher_exact.py - map points within a few ulps of a gate of Fuse (chi-square, mono and
stereo), SearchByProjection(KF, Scw), Fuse(KF, Scw), SearchByProjection(Current, Last), SearchByProjection(Current, KF) of relocalisation and SearchBySim3 (both
passes), and SearchForTriangulation calls whose aimed pair sits on the epipolar-line gate or whose epipole sits on its distance gate - as the device calls the
drop-in classes make for them.

Both drop-in builds run the cases on the CPU emulation of the kernels, which records every projected search and every triangulation search as the C ABI receives
it (ORBHIP_TEST_RECORD, an emulation-only hook of orb_slam2_amd/csrc/orbhip_internal.h): the build with the reference's OWN flags (-O3 -march=native: its
ORBmatcher.cc asks for the fused forms, ORBHIP_FP_CONTRACT) and the canonical one (-ffp-contract=off).  Before anything is written, each drop-in's member outputs
must equal those of the reference built the same way (`make -C oracle ref_native_slam`), so the recorded answers are the ones behind the native and the canonical
reference's results.  The fixtures travel to the GPU box, where neither reference build exists; tests/test_native_flags_matcher_gpu.py replays the recorded calls
through liborbhip.so.  Two files: native_flags_matcher_calls.npz (the projected searches) and native_flags_triangulation_calls.npz (tag 3; the key frames' arrays
repeat from call to call, so every distinct array is stored once as pool.<k> and named by <tag>.<field>@[call] = k; the per-call arrays of all calls lie
end to end in <tag>.<field>, call i at bytes <tag>.<field>.off[i : i + 2]).
Run from the repo root where the reference sources are mounted: python tests/golden/make_golden_native_matcher.py"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import orbslam_ref as S  # noqa: E402
import test_native_flags_matcher_exact as E  # noqa: E402

# the arrays of a record, in the order orbhip_search.hip writes them
FIELDS = {1: ("kps", "desc", "u_right", "blocked", "bounds", "proj", "points", "pdesc", "fpar", "ipar", "feature_query"),
          2: ("kps", "desc", "u_right", "bounds", "inv_level_sigma2", "proj", "points", "pdesc", "ipar", "best_idx", "best_dist"),
          3: ("desc1", "kp1", "has_mp1", "stereo1", "fv1_node", "fv1_off", "fv1_feat", "desc2", "kp2", "has_mp2", "stereo2", "fv2_node", "fv2_off", "fv2_feat",
              "F12", "epipole", "scale_factors2", "level_sigma2_2", "ipar", "match12")}
POOLED = ("desc1", "kp1", "stereo1", "desc2", "kp2", "stereo2", "scale_factors2", "level_sigma2_2")      # of a triangulation record: the same from call to call


def read_records(path):
    out = []
    with open(path, "rb") as f:
        buf = f.read()
    o = 0
    while o < len(buf):
        tag = int(np.frombuffer(buf, np.int32, 1, o)[0]); o += 4
        rec = {"tag": tag}
        for name in FIELDS[tag]:
            b = int(np.frombuffer(buf, np.int64, 1, o)[0]); o += 8
            rec[name] = None if b < 0 else np.frombuffer(buf, np.uint8, b, o).copy()
            o += max(b, 0)
        out.append(rec)
    return out


def recorded_run(lib, F, cases):
    """every member by itself, so that the records can be counted per member -> (outputs, records, {member: record count})"""
    res, recs, count = {}, [], {}
    for m in E.ALL_MEMBERS:
        fd, path = tempfile.mkstemp(suffix=".rec"); os.close(fd)
        os.environ["ORBHIP_TEST_RECORD"] = path
        try:
            res.update(E.run(S, lib, F, cases, which=(m,)))
            r = read_records(path)
        finally:
            del os.environ["ORBHIP_TEST_RECORD"]
            os.unlink(path)
        assert all((x["tag"] == 3) == (m == "tri") for x in r), m
        recs += r; count[m] = len(r)
    return res, recs, count


assert S.build() and S.build_native() and S.build_dropin() and S.build_dropin_native(), "needs the reference sources"
nat, can = S.native_lib(), S.lib()
Fn, Fc = E.frames(S, nat), E.frames(S, can)
cases = E.straddling_cases(S, nat, can, Fn, Fc)
rn, rc = E.run(S, nat, Fn, cases), E.run(S, can, Fc, cases)
out, tri, pool = {}, {}, {}
for tag, ref, lib in (("native", rn, S.dropin_native_lib()), ("canonical", rc, S.dropin_full_lib())):
    res, recs, count = recorded_run(lib, E.frames(S, lib), cases)
    for m in E.ALL_MEMBERS:
        assert np.array_equal(res[m], ref[m]), (tag, m)          # the recorded calls are the ones behind the reference's own answers
    mine = [r for r in recs if r["tag"] != 3]
    out[f"{tag}.n"] = np.int32(len(mine))
    for i, r in enumerate(mine):
        out[f"{tag}.{i}.tag"] = np.int32(r["tag"])
        for name in FIELDS[r["tag"]]:
            if r[name] is not None:
                out[f"{tag}.{i}.{name}"] = r[name]
    mine = [r for r in recs if r["tag"] == 3]                      # (an archive member per record and field would cost more than the data: one per field)
    tri[f"{tag}.n"] = np.int32(len(mine))
    for name in FIELDS[3]:
        if name in POOLED:
            tri[f"{tag}.{name}@"] = np.array([pool.setdefault(r[name].tobytes(), len(pool)) for r in mine], np.int32)
        else:
            tri[f"{tag}.{name}"] = np.concatenate([r[name] for r in mine])
            tri[f"{tag}.{name}.off"] = np.cumsum([0] + [len(r[name]) for r in mine]).astype(np.int64)
    for m in E.ALL_MEMBERS:
        (tri if m == "tri" else out)[f"{tag}.n.{m}"] = np.int32(count[m])
    assert int(tri[f"{tag}.n"]) == len(cases["tri"]["calls"]), "one device call per SearchForTriangulation"
for b, k in pool.items():
    tri[f"pool.{k}"] = np.frombuffer(b, np.uint8)
moved = {m: int((rn[m] != rc[m]).sum()) for m in E.MEMBERS}
new, tri_kind = E.moved_new(cases, rn, rc)
out["moved"] = np.int32(sum(moved.values()))
for m in ("reloc", "sim3", "sim3_pass1", "sim3_pass2"):
    out[f"moved.{m}"] = np.int32(new[m])
tri["moved"] = np.int32(new["tri"])
tri["kinds"] = np.array([t["kind"] for t in cases["tri"]["calls"]])
path, tpath = os.path.join(HERE, "native_flags_matcher_calls.npz"), os.path.join(HERE, "native_flags_triangulation_calls.npz")
np.savez_compressed(path, **out)
np.savez_compressed(tpath, **tri)
per = lambda d, tag: ", ".join(f"{m} {int(d[f'{tag}.n.{m}'])}" for m in E.ALL_MEMBERS if f"{tag}.n.{m}" in d)
print(f"golden: {path} ({os.path.getsize(path)} bytes): {int(out['native.n'])} / {int(out['canonical.n'])} recorded device calls (native: {per(out, 'native')}; canonical: {per(out, 'canonical')}); "
      f"{tpath} ({os.path.getsize(tpath)} bytes): {int(tri['native.n'])} / {int(tri['canonical.n'])} triangulation calls, {len(pool)} pooled arrays; "
      f"member outputs that differ between the native and the canonical reference: " + ", ".join(f"{m} {v}" for m, v in {**moved, **new}.items()) +
      " (tri = match12 entries, by kind of call: " + ", ".join(f"{k} {v}" for k, v in sorted(tri_kind.items())) + ")")
