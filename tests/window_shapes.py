"""Synthetic frames and queries for the windowed searches (k_best_in_window over the table of k_match_grid / k_match_grid_big), and a numpy restatement of what the
table and the kernel's scan look like for them, so that a test can ASSERT the shape it claims to test - the cell populations, the run position (lane, chunk) of
the winner, the side of a literal a float product falls on - before it calls the library.  No tests here.

The table: the cell of a key point is px = round((x - min_x) * gw), py = round((y - min_y) * gh) in float32 (roundf: halves away from zero), gw = 64 / (max_x - min_x),
gh = 48 / (max_y - min_y); a key point with px outside 0..63 or py outside 0..47 is not in the table; the others stand in it by (px * 48 + py, index).
The scan: a query reads the table from start[col_lo * 48] to start[col_hi * 48] (column_run), 64 entries (one per lane) a step ("chunk")."""
import numpy as np

import orb_slam2_amd

COLS, ROWS, CELLS = 64, 48, 64 * 48
KD = orb_slam2_amd.KEYPOINT_DTYPE
QD = orb_slam2_amd.BEST_QUERY_DTYPE
f32 = np.float32
GRID_LDS_MAX = 150 * 1024                              # orbhip_launch_match_grid: a table that needs more LDS is built in device memory (k_match_grid_big)


def grid_lds_bytes(cap):
    """orbhip_match_grid_lds: counters, the table and the u16 cell of every key point, for a frame capacity (the searches round it up to 64)"""
    return 4 * (CELLS + 1 + cap) + 2 * (cap + 2)


def keypoints(x, y, octave=0):
    k = np.zeros(len(x), KD)
    k["x"], k["y"], k["octave"], k["size"] = np.asarray(x, f32), np.asarray(y, f32), octave, 31.0
    return k


def queries(x, y, radius, level=0, ur=0.0):
    q = np.zeros(len(np.atleast_1d(x)), QD)
    q["x"], q["y"], q["radius"], q["level"], q["ur"] = np.asarray(x, f32), np.asarray(y, f32), radius, level, ur
    return q


def descriptor(seed):
    return np.random.default_rng(1000 + seed).integers(0, 256, 32, dtype=np.uint8)


def at_distance(d, dist):
    """a copy of descriptor d with its first `dist` bits flipped (256: the complement)"""
    out = d.copy()
    for b in range(dist):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def inv_cell(bounds):
    b = [f32(v) for v in bounds]
    return f32(COLS) / f32(b[2] - b[0]), f32(ROWS) / f32(b[3] - b[1])


def _roundf(v):
    """roundf on float32 values: halves away from zero (in float64, where v +- 0.5 is exact)"""
    v = np.asarray(v, np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5))


def grid_coords(x, y, bounds):
    """(px, py) of Frame::AssignFeaturesToGrid, as integers (not yet tested against the table's 64 x 48)"""
    gw, gh = inv_cell(bounds)
    vx = (np.asarray(x, f32) - f32(bounds[0])) * gw
    vy = (np.asarray(y, f32) - f32(bounds[1])) * gh
    assert vx.dtype == f32 and vy.dtype == f32
    return np.clip(_roundf(vx), -1e9, 1e9).astype(np.int64), np.clip(_roundf(vy), -1e9, 1e9).astype(np.int64)


class Table:
    """cell[i]: px * 48 + py of key point i, -1 if the grid drops it; order: the key point indices in table order; start[c]: first table position of cell c
    (start[3072] = entries in the table)"""

    def __init__(self, kps, bounds):
        self.kps, self.bounds = kps, tuple(float(v) for v in bounds)
        px, py = grid_coords(kps["x"], kps["y"], bounds)
        inside = (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)
        self.px, self.py = px, py
        self.cell = np.where(inside, px * ROWS + py, -1)
        kept = np.flatnonzero(inside)
        self.order = kept[np.argsort(self.cell[kept], kind="stable")]              # by (cell, index)
        self.start = np.concatenate([[0], np.cumsum(np.bincount(self.cell[kept], minlength=CELLS))]).astype(np.int64)

    def dropped(self):
        return np.flatnonzero(self.cell < 0)

    def population(self, px, py):
        c = px * ROWS + py
        return int(self.start[c + 1] - self.start[c])

    def column_ends(self, x, radius):
        """cl, ch: the float32 column coordinates of the window's left and right edge, as the kernel forms them"""
        gw, _ = inv_cell(self.bounds)
        d = f32(x) - f32(self.bounds[0])
        return f32(f32(d - f32(radius)) * gw), f32(f32(d + f32(radius)) * gw)

    def column_run(self, x, radius):
        """(t_lo, t_hi): the table positions the kernel scans for a query at column coordinate x with this radius"""
        cl, ch = self.column_ends(x, radius)
        col_lo = int(min(np.floor(cl) - 1, COLS)) if cl >= 1 else 0
        col_hi = int(max(np.ceil(ch) + 2, 0)) if ch < COLS - 2 else COLS
        return int(self.start[min(col_lo, col_hi) * ROWS]), int(self.start[col_hi * ROWS])

    def in_window(self, q):
        """(run positions, key point indices) of the scanned entries inside the query's square, in scan order; positions are relative to the run's start,
        so that position p is lane p % 64 of chunk p // 64"""
        t_lo, t_hi = self.column_run(q["x"], q["radius"])
        idx = self.order[t_lo:max(t_hi, t_lo)]
        k = self.kps[idx]
        ok = (np.abs(k["x"] - f32(q["x"])) < f32(q["radius"])) & (np.abs(k["y"] - f32(q["y"])) < f32(q["radius"]))
        return np.flatnonzero(ok), idx[ok]

    def level_window(self, q):
        """in_window, then the level filter level-1 .. level"""
        pos, idx = self.in_window(q)
        lv = self.kps["octave"][idx]
        ok = (lv >= q["level"] - 1) & (lv <= q["level"])
        return pos[ok], idx[ok]


def chi2_product(qx, qy, qur, kx, ky, ur, inv_sigma2):
    """the float the kernel compares with 5.99 (ur is None: the monocular branch) or 7.8, in its canonical rounding sequence:
    ex*ex, ey*ey, their sum, (+ er*er,) times the level's inverse sigma^2 - every step rounded to float32"""
    ex, ey = f32(f32(qx) - f32(kx)), f32(f32(qy) - f32(ky))
    e2 = f32(f32(ex * ex) + f32(ey * ey))
    if ur is not None:
        er = f32(f32(qur) - f32(ur))
        e2 = f32(e2 + f32(er * er))
    return f32(e2 * f32(inv_sigma2))


def float_steps(a, b):
    """how many float32 values lie between two positive floats (0: equal, 1: neighbours)"""
    return abs(int(np.array(a, f32).view(np.int32)) - int(np.array(b, f32).view(np.int32)))


def neighbours(v, k):
    """the 2k + 1 float32 values around a positive v, ascending"""
    b = int(np.array(v, f32).view(np.int32))
    return np.arange(b - k, b + k + 1, dtype=np.int32).view(f32)


def one_cell_frame(rng, n, bounds, px, py, nlevels=4):
    """n key points, all in cell (px, py): jittered inside it (away from its rounding edges), mixed levels"""
    gw, gh = inv_cell(bounds)
    x = f32(bounds[0]) + (f32(px) + rng.uniform(-0.45, 0.45, n).astype(f32)) / gw
    y = f32(bounds[1]) + (f32(py) + rng.uniform(-0.45, 0.45, n).astype(f32)) / gh
    return keypoints(x, y, rng.integers(0, nlevels, n))
