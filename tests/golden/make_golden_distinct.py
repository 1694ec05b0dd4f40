"""Freezes what ORB_SLAM2's own MapPoint::ComputeDistinctiveDescriptors does with a list of map points -> tests/golden/distinct_ref.npz (data only).

Runs only where the reference checkout is mounted (/root/reference, or $ORBSLAM_REF).  The reference's src/MapPoint.cc is compiled where it lies, into a
temporary directory (never into this repository), against the test-owned stand-ins of tests/distinct/ (stub/KeyFrame.h, stub/Frame.h, stub/Map.h, mp_stub.cpp);
its include/MapPoint.h is the reference's own.  The key frames lie in one array, so a point's std::map<KeyFrame*,size_t> walks them in index order.  Every
point's mDescriptor is recorded before and after the member ran.  The same groups go through tests/distinct_model.py: the generator refuses to write a
golden that lacks one of the situations the tests are about, or that the model does not reproduce.

    python tests/golden/make_golden_distinct.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("ORBSLAM_REF", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "distinct_ref.npz")
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 300, 1000)      # 1000: about 4 MB of the member's stack array; no higher
NKF = 1010
BAD_KFS = (3, 7, 500)


def make_points(seed=4242):
    """-> kf_rows, desc (key-frame major), points = list of (obs_kf, obs_row, bad, initial)"""
    rng = np.random.default_rng(seed)
    good = np.array([k for k in range(NKF) if k not in BAD_KFS])
    rows = [[] for _ in range(NKF)]                                           # descriptors of every key frame
    points = []

    def near(base, n, p=0.12):
        flip = rng.random((n, 256)) < p
        return np.packbits(np.unpackbits(np.repeat(base[None], n, 0), axis=1) ^ flip, axis=1)

    def point(kfs, descs, bad=False):
        obs_row = []
        for k, d in zip(kfs, descs):
            obs_row.append(len(rows[k]))
            rows[k].append(np.asarray(d, np.uint8))
        order = rng.permutation(len(kfs))                                     # AddObservation in any order: the map sorts
        points.append((np.asarray(kfs, np.int32)[order], np.asarray(obs_row, np.int32)[order], bad, rng.integers(0, 256, 32, dtype=np.uint8)))

    rnd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)
    for n in SIZES:                                                           # the sizes, in good key frames only
        point(np.sort(rng.choice(good, n, replace=False)), near(rnd(), n))
    three = [rnd() for _ in range(3)]                                         # drawn from three descriptors: nearly every median ties, many duplicates
    for n in (6, 17, 64, 70):
        point(np.sort(rng.choice(good, n, replace=False)), [three[i] for i in rng.integers(0, 3, n)])
    d = rnd()
    point(good[:5], [near(d, 1)[0], d, ~d, near(d, 1)[0], near(d, 1)[0]])     # a complementary pair: distance 256
    point(good[10:12], [d, ~d])                                               # ... alone: N = 2, median 0 all the same
    point(good[20:29], [d] * 9)                                               # identical descriptors
    point(good[30:33], [d, d, near(d, 1)[0]])                                 # duplicates beside another
    # an observation in a bad key frame in front of the others: it is skipped, the chosen row lies behind it.  The tight cluster sits in the last three rows.
    c = rnd()
    point([1, 3, 5, 9, 11, 13], [rnd(), rnd(), rnd(), near(c, 1, 0.02)[0], c, near(c, 1, 0.02)[0]])
    point([2, 7, 8, 500, 501], near(rnd(), 5))                                # two bad key frames among good ones
    point([3, 7], near(rnd(), 2))                                             # all key frames bad: untouched
    point([3], near(rnd(), 1))
    point(good[40:46], near(rnd(), 6), bad=True)                              # a bad point: untouched
    point([], [])                                                             # no observations: untouched
    kf_rows = np.array([len(r) for r in rows], np.int32)
    desc = np.array([d for r in rows for d in r], np.uint8).reshape(-1, 32)
    return kf_rows, desc, points


def check_situations(g):
    import distinct_model as M
    groups = M.golden_groups(g)
    seen = {"tie": False, "duplicates": False, "complementary": False, "identical": False, "bad key frame skipped": False, "all key frames bad": False,
            "bad point": False, "no observations": False}
    sizes = set()
    for p, (d, untouched) in enumerate(groups):
        a, b = int(g["obs_off"][p]), int(g["obs_off"][p + 1])
        kf = np.sort(g["obs_kf"][a:b])
        if g["point_bad"][p]:
            seen["bad point"] = True
            continue
        if a == b:
            seen["no observations"] = True
            continue
        if len(d) == 0:
            seen["all key frames bad"] = True
            continue
        n = len(d)
        sizes.add(n)
        t = M.distances(d).astype(np.int32)
        med = np.sort(t, axis=1)[:, int(0.5 * (n - 1))]
        first = int(np.argmin(med))
        seen["tie"] |= int((med == med.min()).sum()) >= 2 and first != n - 1
        nu = len(np.unique(d, axis=0))
        seen["duplicates"] |= 1 < nu < n
        seen["identical"] |= n >= 2 and nu == 1
        seen["complementary"] |= bool((t == 256).any())
        bad_at = [i for i, k in enumerate(kf) if g["kf_bad"][k]]
        if bad_at and bad_at[0] < len(kf) - 1 and first >= bad_at[0]:        # the winner's index among ALL observations is behind a skipped one
            seen["bad key frame skipped"] = True
    missing = [k for k, v in seen.items() if not v] + [f"group size {n}" for n in SIZES if n not in sizes]
    assert not missing, f"the golden lacks: {missing}"


def main():
    if not os.path.isdir(os.path.join(REF, "src")):
        sys.exit(f"{REF} is not mounted: the golden is made where the reference is")
    import distinct_harness as H
    import distinct_model as M
    kf_rows, desc, points = make_points()
    kf_bad = np.zeros(NKF, np.uint8); kf_bad[list(BAD_KFS)] = 1
    g = {"kf_rows": kf_rows, "desc": desc, "kf_bad": kf_bad,
         "obs_off": np.concatenate([[0], np.cumsum([len(p[0]) for p in points])]).astype(np.int32),
         "obs_kf": np.concatenate([p[0] for p in points]).astype(np.int32), "obs_row": np.concatenate([p[1] for p in points]).astype(np.int32),
         "point_bad": np.array([p[2] for p in points], np.uint8), "initial": np.array([p[3] for p in points], np.uint8)}
    check_situations(g)
    with tempfile.TemporaryDirectory() as tmp:
        w = H.world_of_golden(H.build(tmp, reference=REF), g)
        g["before"] = w.descriptors()
        w.member(np.arange(len(points)))
        g["after"] = w.descriptors()
        w.close()
    assert np.array_equal(g["before"], g["initial"])
    agree = 0
    for p, (d, untouched) in enumerate(M.golden_groups(g)):
        want = g["before"][p] if untouched else d[M.best(d)[0]]
        assert np.array_equal(g["after"][p], want), f"the model does not reproduce the reference at point {p}"
        agree += 1
    np.savez_compressed(OUT, **g)
    print(f"{OUT}: {len(points)} points, {len(desc)} descriptors in {NKF} key frames, {os.path.getsize(OUT)} bytes; the model reproduces all {agree}")


if __name__ == "__main__":
    main()
