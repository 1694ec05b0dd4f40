"""orb_slam2_amd/cpp/MapPointBatch.cc (ComputeDistinctiveDescriptorsBatch of include/ORBmatcherBatch.h) on the emulation build.  The points of
tests/golden/distinct_ref.npz are rebuilt from the test-owned stand-ins of tests/distinct/ and run through the batch form: every point must end with the
mDescriptor the reference's own member left (the golden), the untouched ones included.  Where the reference is mounted its src/MapPoint.cc is built beside
the batch form: member per point on one copy of the points, the batch on another, equal descriptors; and the installer's src/MapPointBatch.cc compiles
(syntax only) against the checkout's own headers.  Everything is compiled into the test's temporary directory."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import distinct_harness as H
import distinct_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = os.path.join(ROOT, "tests", "golden", "distinct_ref.npz")
SCRIPT = os.path.join(ROOT, "integration", "apply_dropin.py")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference sources not mounted")


def test_batch_form_replays_the_golden(emu_lib, tmp_path):
    g = M.load_golden(GOLDEN)
    w = H.world_of_golden(H.build(tmp_path, reference=None, batch_lib=emu_lib), g)
    npts = len(g["initial"])
    assert np.array_equal(w.descriptors(), g["before"])
    w.batch([-1] + list(range(npts)) + [-1])                                 # NULL elements are skipped
    got = w.descriptors()
    w.close()
    bad = [p for p in range(npts) if not np.array_equal(got[p], g["after"][p])]
    assert not bad, bad
    assert (g["after"] != g["before"]).any(axis=1).sum() >= 20 and (g["after"] == g["before"]).all(axis=1).sum() >= 3


@needs_reference
def test_batch_form_equals_the_member(emu_lib, tmp_path):
    g = M.load_golden(GOLDEN)
    lib = H.build(tmp_path, reference=REF, batch_lib=emu_lib)
    one, all_ = H.world_of_golden(lib, g), H.world_of_golden(lib, g)
    pts = np.arange(len(g["initial"]))
    one.member(pts)
    all_.batch(pts)
    a, b = one.descriptors(), all_.descriptors()
    one.close(); all_.close()
    assert np.array_equal(a, g["after"]) and np.array_equal(a, b)


@needs_reference
def test_installer_writes_the_batch_file(tmp_path):
    from test_apply_dropin import _flags
    out = tmp_path / "out"
    subprocess.run([sys.executable, SCRIPT, REF, str(out)], capture_output=True, text=True, check=True)
    assert (out / "src/MapPointBatch.cc").read_text() == open(os.path.join(ROOT, "orb_slam2_amd/cpp/MapPointBatch.cc")).read()
    assert "void ComputeDistinctiveDescriptorsBatch(" in (out / "include/ORBmatcherBatch.h").read_text() and "struct DistinctAccess;" in (out / "include/ORBmatcher.h").read_text()
    assert "+++ b/src/MapPointBatch.cc" in subprocess.run([sys.executable, SCRIPT, "--patch", REF], capture_output=True, text=True, check=True).stdout
    co = tmp_path / "co"
    shutil.copytree(os.path.join(REF, "include"), co / "include")
    os.remove(co / "include/Converter.h")
    for rel in ("include/ORBextractor.h", "include/ORBmatcher.h", "include/orbhip.h", "include/ORBmatcherBatch.h", "include/MapPoint.h"):
        shutil.copyfile(out / rel, co / rel)
    r = subprocess.run(["g++"] + _flags(co) + [str(out / "src/MapPointBatch.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # without the friend line the file refuses to compile, and says why
    shutil.copyfile(os.path.join(REF, "include/MapPoint.h"), co / "include/MapPoint.h")
    r = subprocess.run(["g++"] + _flags(co) + [str(out / "src/MapPointBatch.cc")], capture_output=True, text=True)
    assert r.returncode != 0 and "friend class ORBmatcher" in r.stderr
