"""tests/init_model.py alone (no library): its stated replacements of OpenCV's primitives against numpy.linalg; every hypothesis of the graded scenes
against an independent restatement (numpy.linalg.svd of A in float64, tests/init_cases.py) with the recorded spread (tests/golden/init_spread.npz) -
a minimal set of 8 gives a system with a one-dimensional null space, so a hypothesis does not hang on a basis; the whole call against the independent
restatement and the ground truth; the draws and Normalize."""
import os

import numpy as np
import pytest

import init_cases as Cs
import init_model as M
import sim3_model as S3
from pnp_model import jacobi_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_spread.npz")
f32 = np.float32
ULP = float(np.spacing(f32(1.0)))
GATE = 1e-10
COMPARED = [nm for nm in Cs.GRADED if nm != "fronto_300"]                       # identical frames: F is degenerate in any arithmetic
_models = {}


def answer(name):
    if name not in _models:
        tr = {}
        _models[name] = (M.reconstruct(trace=tr, **Cs.arguments(Cs.case(name))), tr)
    return _models[name]


@pytest.mark.parametrize("n", [4, 9])
def test_jacobi_against_eigh(n):
    rng = np.random.default_rng(n)
    mats = [B.T @ B for B in (rng.normal(size=(n + 3, n)) for _ in range(4))] + [B.T @ B for B in (rng.normal(size=(n - 1, n)) for _ in range(2))]
    w, V = jacobi_batch(np.array(mats))
    for k, A in enumerate(mats):
        ws, Vs = S3.jacobi(A)                                                   # the one-matrix statement
        assert np.array(ws).tobytes() == w[k].tobytes() and np.array(Vs).tobytes() == V[k].tobytes()
        ew, ev = np.linalg.eigh(A)
        assert np.allclose(np.sort(w[k]), ew, atol=1e-12 * ew[-1])
        b = int(M.smallest(w[k:k + 1])[0])
        assert w[k, b] == w[k].min() and abs(abs(V[k][:, b] @ ev[:, 0]) - 1.0) <= 1e-9
    # the first index strictly smaller than every earlier one: of two equal smallest values the first
    assert M.smallest(np.array([[3.0, 1.0, 2.0, 1.0], [0.5, 0.5, 0.7, 0.9]])).tolist() == [1, 0]


def test_svd3_against_numpy():
    rng = np.random.default_rng(5)
    for rank in (3, 3, 3, 2, 2):
        A = rng.normal(size=(3, 3)).astype(f32)
        if rank == 2:
            U, s, Vt = np.linalg.svd(A.astype(float))
            A = (U @ np.diag([s[0], s[1], 0.0]) @ Vt).astype(f32)
        tr = {}
        U, w, V = M.svd3(A, tr)
        sn = np.linalg.svd(A.astype(float), compute_uv=False)
        assert U.dtype == f32 and np.abs(w - sn).max() <= 4 * ULP * sn[0] and (w[0] >= w[1] >= w[2])
        assert np.abs((U.astype(float) * w.astype(float)) @ V.astype(float).T - A).max() <= 8 * ULP * sn[0]
        assert np.abs(U.astype(float).T @ U.astype(float) - np.eye(3)).max() <= 8 * ULP
    exact = np.diag([2.0, 1.0, 0.0]).astype(f32)                                # exactly rank 2: the cross-product arm
    tr = {}
    with np.errstate(all="ignore"):
        U, w, V = M.svd3(exact, tr)
    assert tr.get("rank2_finite") == 1 and w.tolist() == [2.0, 1.0, 0.0] and abs(np.linalg.det(U.astype(float)) * np.linalg.det(V.astype(float)) - 1.0) <= 1e-6


def test_inverse_and_determinant_against_numpy():
    rng = np.random.default_rng(6)
    for _ in range(6):
        A = rng.normal(size=(3, 3)).astype(f32)
        want = np.linalg.inv(A.astype(float))
        assert np.abs(M.inv3(A) - want).max() <= 2 * ULP * np.abs(want).max()
        assert abs(M.det3(A) - np.linalg.det(A.astype(float))) <= 1e-12 * np.abs(A).max() ** 3
    with np.errstate(all="ignore"):
        assert not np.isfinite(M.inv3(np.array([[1, 2, 3], [2, 4, 6], [1, 0, 1]], f32))).any()     # singular: non-finite, and every comparison false


def test_products_in_both_gemm_modes():
    a, b = np.array([1.0, 2.0 ** -24, -1.0], f32), np.array([1.0, 1.0, 1.0], f32)
    assert M.mul(0, a, b) == f32(2.0 ** -24) and M.mul(1, a, b) == f32(0.0)     # the double sum keeps what the float sum loses
    R, x, t = np.eye(3, dtype=f32), np.array([1.0, 0.0, 0.0], f32), np.array([2.0 ** -24, 0, 0], f32)
    assert M.affine(0, R[0], x, t[0]) == M.affine(1, R[0], x, t[0]) == f32(1.0)


@pytest.mark.parametrize("name", COMPARED)
def test_every_hypothesis_against_the_independent_null_vector(name):
    g = np.load(GOLDEN)
    args = Cs.arguments(Cs.case(name))
    worst = {}
    for is_f, tag in ((False, "H"), (True, "F")):
        v = M.null_vectors(args["matches"], args["sets"], args["norm1"], args["norm2"], is_f)
        vi, ratio = Cs.independent_null_vectors(args["matches"], args["sets"], args["norm1"], args["norm2"], is_f)
        keep = ratio > GATE
        vi = np.where((np.sum(vi * v, 1) < 0)[:, None], -vi, vi)                # sign alignment: the sign of a null vector is free
        dev = np.abs(v.astype(float) - vi).max(axis=1)
        worst[tag] = float(dev[keep].max())
        print(f"{name} {tag}: {int(keep.sum())} of {len(keep)} compared, largest deviation {worst[tag]:.3e}, recorded spread {g[name + '/' + tag][0]:.3e}")
        assert abs((~keep).mean() - g[name + "/" + tag][1]) < 1e-12, "the gate no longer leaves out the recorded share - rerun tests/golden/make_golden_init_spread.py"
        assert worst[tag] <= 4.0 * g[name + "/" + tag][0] + ULP


def test_the_gate_leaves_out_less_than_five_percent():
    out = total = 0
    for name in COMPARED:
        args = Cs.arguments(Cs.case(name))
        for is_f in (False, True):
            ratio = Cs.independent_null_vectors(args["matches"], args["sets"], args["norm1"], args["norm2"], is_f)[1]
            out += int((~(ratio > GATE)).sum()); total += len(ratio)
    print(f"{out} of {total} hypotheses left out")
    assert out < 0.05 * total


@pytest.mark.parametrize("name", [nm for nm in COMPARED if answer(nm)[0]["best_mot"] >= 0])
def test_triangulation_against_the_independent_null_vector(name):
    g = np.load(GOLDEN)
    args = Cs.arguments(Cs.case(name))
    m, _ = answer(name)
    R, t = m["mot_R"][m["best_mot"]], m["mot_t"][m["best_mot"]]
    mask = m["mask_h"] if m["model"] == 0 else m["mask_f"]
    fx, fy, cx, cy = Cs.K
    P1 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], f32)
    with np.errstate(all="ignore"):
        x, A, AtA = M.triangulate(args["matches"][mask], P1, M.projection(Cs.K, R, t, args["gemm_mode"])[0], with_system=True)
    dev = []
    for k in range(len(A)):
        sv = np.linalg.svd(A[k], compute_uv=False) ** 2
        if not sv[2] > GATE * sv[0]:
            continue
        vi = np.linalg.svd(A[k])[2][3]
        vi = vi if vi @ x[k] >= 0 else -vi
        dev.append(np.abs(x[k].astype(float) - vi).max())
    print(f"{name}: {len(dev)} of {len(A)} triangulations compared, largest deviation {max(dev):.3e}, recorded spread {g[name + '/T'][0]:.3e}")
    assert len(dev) > 0.95 * len(A) and max(dev) <= 4.0 * g[name + "/T"][0] + ULP


def angle(Ra, Rb):
    return float(np.rad2deg(np.arccos(np.clip((np.trace(np.asarray(Ra, float).T @ np.asarray(Rb, float)) - 1) / 2, -1, 1))))


def direction(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.rad2deg(np.arccos(np.clip(a @ b / np.linalg.norm(a) / np.linalg.norm(b), -1, 1))))


@pytest.mark.parametrize("name", Cs.GRADED)
def test_whole_call_against_the_independent_restatement_and_the_truth(name):
    c = Cs.case(name)
    m, tr = answer(name)
    like = (tr["motion_svd"][0], tr["motion_svd"][2], m["H21"], m["F21"]) if "motion_svd" in tr else None
    ind = Cs.independent(c, like)
    print(f"{name}: independent RH {ind['RH']:.3f}, model chosen {m['model']}, returned {m['returned']}, ends on {m['best_mot']} (independent {ind['best_mot']})")
    assert not 0.35 <= ind["RH"] <= 0.45, "the scene does not decide between H and F clearly"
    assert (m["returned"], m["model"], m["best_mot"]) == (ind["returned"], ind["model"], ind["best_mot"])
    if m["returned"]:
        R, t = c["truth"]["R"], c["truth"]["t"]
        eR, et = angle(m["R21"], R), direction(m["t21"], t)
        iR, it = angle(ind["R21"], R), direction(ind["t21"], t)
        nm, ni = int(m["triangulated"].sum()), int(ind["triangulated"].sum())
        print(f"{name}: against the truth: R {eR:.4f} deg (independent {iR:.4f}), t {et:.4f} deg (independent {it:.4f}), triangulated {nm} (independent {ni} of {len(c['matches'])})")
        assert eR <= 4.0 * iR + 1e-3 and et <= 4.0 * it + 1e-3
        assert abs(nm - ni) <= 4 * max(1, len(c["matches"]) - ni) and nm >= 50


def test_generator_conditions():
    import init_checks as K
    K.check_conditions()


def test_normalize_is_the_serial_float_sum():
    rng = np.random.default_rng(3)
    pts = np.stack([rng.uniform(0, 640, 2000), rng.uniform(0, 480, 2000)], 1).astype(f32)
    mx = my = f32(0)
    for x, y in pts:
        mx = mx + x; my = my + y
    mx, my = mx / f32(2000), my / f32(2000)
    dx = dy = f32(0)
    for x, y in pts:
        dx = dx + abs(x - mx); dy = dy + abs(y - my)
    want = [mx, my, f32(1.0 / float(dx / f32(2000))), f32(1.0 / float(dy / f32(2000)))]
    assert M.normalize(pts).tolist() == [float(v) for v in want]
    assert M.normalize(pts).tolist() != M.normalize(pts[::-1]).tolist()         # the order matters: a sum that reorders would not give these bits


def test_draws_are_a_swap_remove_over_fresh_indices():
    calls = []

    def rand(lo, hi):
        calls.append((lo, hi))
        return hi if len(calls) % 2 else lo
    sets = M.draw_sets(10, 3, rand)
    assert calls == [(0, 9 - j) for j in range(8)] * 3 and all(len(set(s)) == 8 for s in sets.tolist())
    assert sets[0].tolist() == sets[1].tolist() == [9, 0, 7, 8, 5, 6, 3, 4]
    a, b = M.draw_sets(20, 4, M.LibcRand(0)), M.draw_sets(20, 4, M.LibcRand(0))
    assert np.array_equal(a, b) and a.min() >= 0 and a.max() < 20


def test_parallax_is_the_float_acos_in_degrees():
    assert M.parallax(0, f32(0.5)) == 0 and abs(float(M.parallax(3, f32(0.5))) - 60.0) < 1e-4 and M.parallax(1, f32(1.0)) == 0
    assert np.isnan(M.parallax(1, f32(1.0000001)))
    c = [f32(x) for x in np.linspace(-1, 1, 2001)]
    p = [float(M.parallax(1, x)) for x in c]
    assert all(a >= b for a, b in zip(p, p[1:]))                                # falls as the cosine rises: the device compares cosines (orbhip_init.hip)
    # ... and float by float around the cosine of Initialize's own threshold, 1 degree (the precondition include/orbhip.h states for the host's acosf)
    x, near = f32(np.cos(np.deg2rad(1.0))), []
    for _ in range(2500):                                                       # (the cosine of 1 degree lies 2555 floats below 1.0)
        x = np.nextafter(x, f32(-1))
    for _ in range(5000):
        near.append(float(M.parallax(1, x)))
        x = np.nextafter(x, f32(2))
    assert all(a >= b for a, b in zip(near, near[1:])) and near[0] > 1.0 > near[-1]
