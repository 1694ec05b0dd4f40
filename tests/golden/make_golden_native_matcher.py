"""Freezes the boundary-straddling matcher cases of tests/test_native_flags_matcher_exact.py - map points within a few ulps of a gate of Fuse (chi-square, mono and
stereo), SearchByProjection(KF, Scw), Fuse(KF, Scw) and SearchByProjection(Current, Last) - as the device calls the drop-in classes make for them.

Both drop-in builds run the cases on the CPU emulation of the kernels, which records every projected search as the C ABI receives it (ORBHIP_TEST_RECORD, an
emulation-only hook of orb_slam2_amd/csrc/orbhip_api.hip): the build with the reference's OWN flags (-O3 -march=native: its ORBmatcher.cc asks for the fused
forms, ORBHIP_FP_CONTRACT) and the canonical one (-ffp-contract=off).  Before anything is written, each drop-in's member outputs must equal those of the reference
built the same way (`make -C oracle ref_native_slam`), so the recorded answers are the ones behind the native and the canonical reference's results.  The fixture
travels to the GPU box, where neither reference build exists; tests/test_native_flags_matcher_gpu.py replays the recorded calls through liborbhip.so.
Run from the repo root where /root/reference is mounted: python tests/golden/make_golden_native_matcher.py"""
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

# the arrays of a record, in the order orbhip_api.hip writes them
FIELDS = {1: ("kps", "desc", "u_right", "blocked", "bounds", "proj", "points", "pdesc", "fpar", "ipar", "feature_query"),
          2: ("kps", "desc", "u_right", "bounds", "inv_level_sigma2", "proj", "points", "pdesc", "ipar", "best_idx", "best_dist")}


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
    fd, path = tempfile.mkstemp(suffix=".rec"); os.close(fd)
    os.environ["ORBHIP_TEST_RECORD"] = path
    try:
        res = E.run(S, lib, F, cases)
        return res, read_records(path)
    finally:
        del os.environ["ORBHIP_TEST_RECORD"]
        os.unlink(path)


assert S.build() and S.build_native() and S.build_dropin() and S.build_dropin_native(), "needs /root/reference"
nat, can = S.native_lib(), S.lib()
Fn, Fc = E.frames(S, nat), E.frames(S, can)
cases = E.straddling_cases(S, nat, can, Fn, Fc)
rn, rc = E.run(S, nat, Fn, cases), E.run(S, can, Fc, cases)
out = {}
for tag, ref, lib in (("native", rn, S.dropin_native_lib()), ("canonical", rc, S.dropin_full_lib())):
    res, recs = recorded_run(lib, E.frames(S, lib), cases)
    for m in E.MEMBERS:
        assert np.array_equal(res[m], ref[m]), (tag, m)          # the recorded calls are the ones behind the reference's own answers
    out[f"{tag}.n"] = np.int32(len(recs))
    for i, r in enumerate(recs):
        out[f"{tag}.{i}.tag"] = np.int32(r["tag"])
        for name in FIELDS[r["tag"]]:
            if r[name] is not None:
                out[f"{tag}.{i}.{name}"] = r[name]
moved = sum(int((rn[m] != rc[m]).sum()) for m in E.MEMBERS)
out["moved"] = np.int32(moved)
path = os.path.join(HERE, "native_flags_matcher_calls.npz")
np.savez_compressed(path, **out)
print(f"golden: {path}: {int(out['native.n'])} / {int(out['canonical.n'])} recorded device calls; {moved} member outputs differ between the native and the canonical reference")
