"""A literal restatement of MapPoint::ComputeDistinctiveDescriptors' selection rule (MapPoint.cc:272-301) in numpy: the float N x N table of
ORBmatcher::DescriptorDistance, every row sorted, element int(0.5*(N-1)) of the sorted row as its median, and the first row whose median is strictly below
the best so far (starting from INT_MAX).  tests/test_distinctive.py pins it to the reference's own output (tests/golden/distinct_ref.npz) and compares the
product with it."""
import numpy as np

INT_MAX = 2**31 - 1


def distances(desc):
    """Distances[N][N] of MapPoint.cc:275-285 (float, as there)"""
    bits = np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    n = len(bits)
    out = np.zeros((n, n), np.float32)
    for i0 in range(0, n, 256):                                               # (blocks of rows: the table of bit differences of a large group stays small)
        out[i0:i0 + 256] = (bits[i0:i0 + 256, None, :] != bits[None, :, :]).sum(-1)
    return out


def best(desc):
    """-> (BestIdx, BestMedian) of one group of descriptors; (-1, -1) for an empty group (the member returns before it gets here)"""
    n = len(desc)
    if n == 0:
        return -1, -1
    table = distances(desc)
    best_median, best_idx = INT_MAX, 0
    for i in range(n):
        v = np.sort(table[i].astype(np.int32))
        median = int(v[int(0.5 * (n - 1))])
        if median < best_median:
            best_median, best_idx = median, i
    return best_idx, best_median


def best_all(desc, offsets):
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    r = [best(desc[offsets[g]:offsets[g + 1]]) for g in range(len(offsets) - 1)]
    return np.array([a for a, _ in r], np.int32), np.array([b for _, b in r], np.int32)


def load_golden(path):
    """-> dict of the arrays of tests/golden/distinct_ref.npz (see tests/golden/make_golden_distinct.py)"""
    z = np.load(path)
    return {k: z[k] for k in z.files}


def golden_groups(g):
    """per point: (the descriptors the member gathers, in the order it gathers them: ascending key frame, bad key frames skipped; untouched?)"""
    out = []
    kf_first = np.concatenate([[0], np.cumsum(g["kf_rows"])])
    for p in range(len(g["obs_off"]) - 1):
        kf, row = g["obs_kf"][g["obs_off"][p]:g["obs_off"][p + 1]], g["obs_row"][g["obs_off"][p]:g["obs_off"][p + 1]]
        order = np.argsort(kf, kind="stable")
        rows = [int(kf_first[kf[i]] + row[i]) for i in order if not g["kf_bad"][kf[i]]]
        untouched = bool(g["point_bad"][p]) or len(rows) == 0
        out.append((g["desc"][rows] if rows else np.zeros((0, 32), np.uint8), untouched))
    return out
