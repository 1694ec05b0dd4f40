"""Builds and drives tests/distinct/mp_stub.cpp: a world of key frames and map points behind a C interface, compiled into a directory the caller names
(a temporary one: never into this repository).  Three users: tests/golden/make_golden_distinct.py (the reference's own src/MapPoint.cc), 
tests/test_distinctive_dropin_cpp.py (orb_slam2_amd/cpp/MapPointBatch.cc, with and without the reference beside it) and tools/distinct_rate.py (the reference's
member timed on the host)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "distinct")


def build(tmp, reference=None, batch_lib=None, name="libdistinct.so"):
    """reference: a checkout of ORB_SLAM2 whose src/MapPoint.cc is compiled where it lies (its include/MapPoint.h is copied to tmp with the installer's one
    friend line); None: the stand-in tests/distinct/own/MapPoint.h.  batch_lib: the liborbhip build ComputeDistinctiveDescriptorsBatch links (None: no batch)."""
    tmp = str(tmp)
    flags = ["-std=c++14", "-w", "-O1", "-fPIC", "-pthread", "-ffp-contract=off", "-fno-fast-math", "-DCVLITE_ALGEBRA", "-DORBHIP_USE_OPENCV"]
    srcs = [os.path.join(STUB, "mp_stub.cpp")]
    if reference:
        sys.path.insert(0, os.path.join(ROOT, "integration"))
        from apply_dropin import patch_mappoint_header
        hdr = os.path.join(tmp, "mappoint_h")
        os.makedirs(hdr, exist_ok=True)
        open(os.path.join(hdr, "MapPoint.h"), "w").write(patch_mappoint_header(open(os.path.join(reference, "include", "MapPoint.h")).read()))
        inc = [hdr]
        srcs.append(os.path.join(reference, "src", "MapPoint.cc"))
    else:
        flags.append("-DDISTINCT_STUB_OWN_MAPPOINT")
        inc = [os.path.join(STUB, "own")]
    inc += [os.path.join(STUB, "stub"), os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "cvlite")]
    link = []
    if batch_lib:
        flags.append("-DDISTINCT_WITH_BATCH")
        srcs.append(os.path.join(ROOT, "orb_slam2_amd", "cpp", "MapPointBatch.cc"))
        d, f = os.path.split(os.path.abspath(batch_lib))
        link = ["-L" + d, "-l" + f[3:-3], "-Wl,-rpath," + d]
    lib = os.path.join(tmp, name)
    r = subprocess.run(["g++", "-shared"] + flags + ["-I" + i for i in inc] + srcs + ["-o", lib] + link, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class World:
    """kf_rows[k] descriptors in key frame k (desc: all of them, key frame after key frame); kf_bad[k] != 0: KeyFrame::isBad()"""

    def __init__(self, lib, kf_rows, desc, kf_bad):
        L = self.L = C.CDLL(lib)
        vp = C.c_void_p
        L.dst_world.restype = vp; L.dst_world.argtypes = [C.c_int, vp, vp]
        L.dst_free.argtypes = [vp]; L.dst_free.restype = None
        L.dst_kf_bad.argtypes = [vp, C.c_int, C.c_int]
        L.dst_point.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int]
        L.dst_descriptor.argtypes = [vp, C.c_int, vp]
        if hasattr(L, "dst_member"):
            L.dst_member.argtypes = [vp, C.c_int, vp]; L.dst_member.restype = C.c_double
        if hasattr(L, "dst_batch"):
            L.dst_batch.argtypes = [vp, C.c_int, vp, C.c_char_p, C.c_int]
        kf_rows = np.ascontiguousarray(kf_rows, np.int32)
        desc = np.ascontiguousarray(desc, np.uint8)
        self.w = L.dst_world(len(kf_rows), _p(kf_rows), _p(desc))
        for k, b in enumerate(kf_bad):
            if b:
                L.dst_kf_bad(self.w, k, 1)
        self.npoints = 0

    def close(self):
        self.L.dst_free(self.w)
        self.w = None

    def point(self, initial, obs_kf, obs_row, bad=False):
        initial = np.ascontiguousarray(initial, np.uint8)
        kf, row = np.ascontiguousarray(obs_kf, np.int32), np.ascontiguousarray(obs_row, np.int32)
        self.npoints += 1
        return self.L.dst_point(self.w, _p(initial), len(kf), _p(kf), _p(row), int(bad))

    def descriptors(self):
        out = np.zeros((self.npoints, 32), np.uint8)
        for p in range(self.npoints):
            self.L.dst_descriptor(self.w, p, _p(out[p]))
        return out

    def member(self, points):
        """the reference's member on every listed point, in order -> milliseconds of the loop"""
        pts = np.ascontiguousarray(points, np.int32)
        return float(self.L.dst_member(self.w, len(pts), _p(pts)))

    def batch(self, points):
        pts = np.ascontiguousarray(points, np.int32)
        err = C.create_string_buffer(512)
        assert self.L.dst_batch(self.w, len(pts), _p(pts), err, 512) == 0, err.value.decode()


def world_of_golden(lib, g):
    """the golden's key frames and points, not yet computed"""
    w = World(lib, g["kf_rows"], g["desc"], g["kf_bad"])
    for p in range(len(g["obs_off"]) - 1):
        a, b = int(g["obs_off"][p]), int(g["obs_off"][p + 1])
        w.point(g["initial"][p], g["obs_kf"][a:b], g["obs_row"][a:b], bool(g["point_bad"][p]))
    return w
