"""Synthetic two-view scenes for the Sim3Solver tests: n map-point pairs seen from two key frames related by a similarity (X1 = s R X2 + t), 1 px of
noise at level 0 growing with the level, a share of wrong matches, levels 0-7, K1 != K2.  Everything is a pure function of the case's parameters and its
seed.  Graded triples are drawn only where the largest eigenvalue of Horn's N is separated from the next by more than GAP of its size (the eigenvector is
then well conditioned: DESIGN.md H17); the generator asserts that it rejects fewer than 5 % of its draws."""
import numpy as np

import sim3_model as M

f32 = np.float32
K1 = np.array([520.9, 521.0, 325.1, 249.7], f32)
K2 = np.array([517.3, 516.5, 318.6, 255.3], f32)
GAP = 1e-3

#           name                    n   n_hyp  fix    scale mode
GRADED = [("n3_h5_fix_m0",          3,    5, True,  1.0, 0),
          ("n4_h5_free13_m1",       4,    5, False, 1.3, 1),
          ("n20_h300_free13_m0",   20,  300, False, 1.3, 0),
          ("n20_h5_fix13_m0",      20,    5, True,  1.3, 0),
          ("n63_h5_fix_m1",        63,    5, True,  1.0, 1),
          ("n64_h5_free_m0",       64,    5, False, 1.0, 0),
          ("n64_h300_free13_m1",   64,  300, False, 1.3, 1),
          ("n65_h1_free13_m1",     65,    1, False, 1.3, 1),
          ("n65_h5_fix_m0",        65,    5, True,  1.0, 0),
          ("n129_h5_fix_m0",      129,    5, True,  1.0, 0),
          ("n129_h1_free_m1",     129,    1, False, 1.0, 1),
          ("n300_h300_free13_m1", 300,  300, False, 1.3, 1),
          ("n300_h300_fix_m0",    300,  300, True,  1.0, 0),
          ("n300_h5_fix13_m0",    300,    5, True,  1.3, 0),
          ("n1000_h5_free13_m0", 1000,    5, False, 1.3, 0),
          ("n1000_h300_fix_m1",  1000,  300, True,  1.0, 1)]
PARAMS = {g[0]: g[1:] for g in GRADED}
ALL_NAMES = [g[0] for g in GRADED]


def level_sigma2(nlevels=8, factor=1.2):
    """mvLevelSigma2 as ORBextractor computes it"""
    sf = np.ones(nlevels, f32)
    for l in range(1, nlevels):
        sf[l] = f32(sf[l - 1] * f32(factor))
    return (sf * sf).astype(f32)


def rotation(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    X = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.cos(angle) * np.eye(3) + (1 - np.cos(angle)) * np.outer(axis, axis) + np.sin(angle) * X


def scene(n, scale, seed, wrong=0.2, noise_px=1.0):
    """corr (n x 8 float32) and the true (R, t, s) of X1 = s R X2 + t"""
    rng = np.random.default_rng([n, int(scale * 10), seed])
    R = rotation(rng.normal(size=3), rng.uniform(0.05, 0.6))
    t = rng.uniform(-0.5, 0.5, 3)
    u, v, z = rng.uniform(30, 610, n), rng.uniform(30, 450, n), rng.uniform(2, 12, n)
    X1 = np.stack([(u - K1[2]) / K1[0] * z, (v - K1[3]) / K1[1] * z, z], 1)
    X2 = (X1 - t) @ R / scale                                                   # R^T (X1 - t) / s
    lev1, lev2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    sig = level_sigma2()
    for X, lev, K in ((X1, lev1, K1), (X2, lev2, K2)):                            # a lateral shift worth noise_px * sigma pixels
        X[:, 0] += rng.normal(0, noise_px, n) * np.sqrt(sig[lev]) * X[:, 2] / K[0] * 0.5
        X[:, 1] += rng.normal(0, noise_px, n) * np.sqrt(sig[lev]) * X[:, 2] / K[1] * 0.5
    bad = rng.random(n) < wrong
    X2[bad] += rng.normal(0, 1.0, (int(bad.sum()), 3))
    corr = np.concatenate([X1, X2, sig[lev1][:, None], sig[lev2][:, None]], 1).astype(f32)
    return corr, (R, t, scale)


def n_of_triple(corr, tri):
    Pr1, _ = M.centroid(corr[tri, 0:3].T)
    Pr2, _ = M.centroid(corr[tri, 3:6].T)
    return M.n_matrix(M.m_matrix(Pr1, Pr2))


def draw_triples(corr, n_hyp, seed, gate=True):
    """n_hyp triples by the solver's swap-remove draw; with gate only triples whose eigenvalue gap exceeds GAP (fewer than 5 % may be rejected)"""
    rng = np.random.default_rng([len(corr), n_hyp, seed, 77])
    n, out, rejected = len(corr), [], 0
    while len(out) < n_hyp:
        avail, tri = list(range(n)), []
        for _ in range(3):
            r = int(rng.integers(0, len(avail)))
            tri.append(avail[r]); avail[r] = avail[-1]; avail.pop()
        if gate and M.eigen_gap(n_of_triple(corr, tri)) <= GAP:
            rejected += 1
            assert rejected < 40, "the scene is degenerate"
            continue
        out.append(tri)
    TALLY[0] += rejected + n_hyp; TALLY[1] += rejected
    assert rejected + n_hyp < 100 or rejected < 0.05 * (rejected + n_hyp), (rejected, n_hyp)     # (a short call is judged with the others: rejected_share)
    return np.array(out, np.int32)


TALLY = [0, 0]                                                                  # gated draws made, draws rejected, over every call so far


def rejected_share():
    return TALLY[1] / max(TALLY[0], 1)


def case(name, seed=0):
    """(corr, triples, fix_scale, mode, min_inliers)"""
    n, n_hyp, fix, scale, mode = PARAMS[name]
    corr, _ = scene(n, scale, seed)
    tri = draw_triples(corr, n_hyp, seed)
    return corr, tri, fix, mode, max(6, n // 2)
