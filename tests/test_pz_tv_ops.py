"""The ground a per-lane test of the time-vectorised polynomial-zonotope operators (armour_amd/csrc/pz_tv.h) stands on -- CPU only.

pz_tv.h rests on one claim: with lane = time step, ONE sorted key list for all steps and coefficient 0 where a step lacks a monomial, every lane
computes exactly what the per-step operator computes for its step.  Holding the device operators to that claim one at a time needs a hook that
runs one operator of the time-vectorised chain on operands in union form; what is here is everything of that comparison that needs no device:

  * the oracle's own side of the claim: monomials with coefficient 0 change nothing in any operator's result, for every op code 0-17 of
    armour_debug_pz_op (12-17, the chain's compound operators, as the compositions tests/test_pz_ops.py oracle_op writes down);
  * operands in union form (keys[U], coef[U, sz, nl], per-step centre / radii) and the helpers that split one into per-lane operands -- the rows
    with a non-zero coefficient in the lane -- and back;
  * the compound op codes' compositions against their definition on a hand-written case;
  * with the 128-bit oracle, in a child process: a key carry across bit 63 and a product whose keys differ only above bit 63."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_pz_ops import OP_SHAPES, ROOT, THR, oracle_op, rand_keys


# ------------------------------------------------------------------ operands in union form, and their per-lane slices
def rand_tpz(rng, sz, count, nl, scale=1.0, small_frac=0.3, present=0.85, keys=None, n_f=7):
    """A PZ of nl time steps in union form.  Coefficients vary smoothly with the lane (neighbouring time steps are nearly alike), three lanes are
    independent draws, a per-lane presence mask removes monomials from single lanes, and `small_frac` of the rows have a norm that runs through
    THR along the lanes: the same key is kept in some lanes and pruned in others."""
    keys = rand_keys(rng, count, n_f=n_f) if keys is None else keys
    count = len(keys)
    t = np.linspace(-1.0, 1.0, nl) if nl > 1 else np.zeros(1)
    coef = rng.normal(size=(count, sz, 1)) * scale + rng.normal(size=(count, sz, 1)) * (0.2 * scale) * t
    lanes = rng.choice(nl, size=min(3, nl), replace=False)
    coef[:, :, lanes] = rng.normal(size=(count, sz, len(lanes))) * scale
    small = rng.random(count) < small_frac
    if small.any():
        u = rng.normal(size=(int(small.sum()), sz, 1))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        f = rng.uniform(0.2, 1.2, (int(small.sum()), 1, 1)) + rng.uniform(0.0, 2.0, (int(small.sum()), 1, 1)) * (t + 1.0) / 2.0
        coef[small] = u * THR * f
    coef = coef * (rng.random((count, 1, nl)) < present)
    cen = rng.normal(size=(sz, 1)) + 0.1 * rng.normal(size=(sz, 1)) * t
    ind = np.abs(rng.normal(size=(sz, nl))) * 0.01
    return dict(sz=sz, keys=keys, coef=coef, cen=cen, ind=ind, ind2=ind * 1.5 + 1e-3)


def lane_operand(u, t, radius="ind"):
    """Lane t's own operand of a union-form PZ: the monomials with a non-zero coefficient there."""
    keep = np.any(u["coef"][:, :, t] != 0.0, axis=1) if len(u["keys"]) else np.zeros(0, bool)
    return dict(sz=u["sz"], keys=u["keys"][keep], coef=u["coef"][keep][:, :, t].reshape(-1, u["sz"]), cen=u["cen"][:, t].copy(), ind=u[radius][:, t].copy())


def union_operand(lanes):
    """Per-lane operands (dicts of pz_op's kind) -> union form; the inverse of lane_operand on every lane."""
    sz, nl = lanes[0]["sz"], len(lanes)
    allk = sorted({int(k) for l in lanes for k in l["keys"]})
    keys = np.array(allk, dtype=lanes[0]["keys"].dtype if len(allk) else np.uint64)
    row = {k: i for i, k in enumerate(allk)}
    coef = np.zeros((len(allk), sz, nl))
    for t, l in enumerate(lanes):
        for m, k in enumerate(l["keys"]):
            coef[row[int(k)], :, t] = l["coef"][m]
    return dict(sz=sz, keys=keys, coef=coef, cen=np.stack([l["cen"] for l in lanes], axis=1), ind=np.stack([l["ind"] for l in lanes], axis=1))


# ------------------------------------------------------------------ CPU
ZERO_MEMBER_OPS = list(range(18))


@pytest.mark.parametrize("op", ZERO_MEMBER_OPS)
def test_zero_coefficient_members_change_nothing_in_the_oracle(op):
    """The ground of the per-lane comparison: an operand's monomials with coefficient 0 leave the keys of every operator's result identical and
    its coefficients, centre, radii and min_margin identical up to the order of a sum -- bit for bit in all but one of these 54 draws: the
    oracle's simplify() orders its raw terms with std::sort (oracle/pz.hpp), which is not stable, so extra members may permute the equal keys of
    a run and with them a sum of three or more terms, by an ulp.  Hence the bounds of the device comparison, which allow for the order of the
    sums: 1e-13 / 1e-12.  (17, which copies its operand's key list, keeps the zero rows: they are removed before the comparison.)"""
    rng = np.random.default_rng(100 + op)
    shapes = OP_SHAPES[op]
    for trial in range(3):
        r = int(rng.integers(3)) if op in (6, 15) else (-1 if trial == 0 else int(rng.integers(3))) if op == 12 else 0
        consts = rng.normal(size=4)
        plain, padded = [], []
        for i, sz in enumerate(shapes):
            if op == 12 and i == 2 and r >= 0:
                sz = 1
            cnt = int(rng.integers(0, 8)) if sz == 9 and i == 1 else int(rng.integers(0, 40))
            u = rand_tpz(rng, sz, cnt + 12, 1, scale=float(rng.choice([1.0, 0.05])), present=1.0)
            zero = np.zeros(cnt + 12, bool)
            zero[rng.choice(cnt + 12, size=12, replace=False)] = True
            u["coef"][zero] = 0.0
            padded.append(dict(sz=sz, keys=u["keys"], coef=u["coef"][:, :, 0], cen=u["cen"][:, 0], ind=u["ind"][:, 0]))
            plain.append(lane_operand(u, 0))
            assert len(plain[-1]["keys"]) <= cnt and len(padded[-1]["keys"]) == cnt + 12
        a, b = oracle_op(op, plain, consts=consts, r=r), oracle_op(op, padded, consts=consts, r=r)
        if op == 17:
            keep = np.any(b["coef"] != 0.0, axis=1)
            b = dict(b, keys=b["keys"][keep], coef=b["coef"][keep])
        assert np.array_equal(a["keys"], b["keys"])
        if len(a["keys"]):
            assert np.abs(a["coef"] - b["coef"]).max() <= 1e-13 * max(1.0, np.abs(a["coef"]).max())
        assert np.abs(a["cen"] - b["cen"]).max() <= 1e-13 * max(1.0, np.abs(a["cen"]).max())
        assert np.abs(a["ind"] - b["ind"]).max() <= 1e-12 * max(1.0, np.abs(a["ind"]).max())
        assert a["min_margin"] == b["min_margin"] or abs(a["min_margin"] - b["min_margin"]) <= 1e-12


def test_union_and_lane_operands_are_inverse():
    rng = np.random.default_rng(7)
    nl = 9
    u = rand_tpz(rng, 3, 25, nl, present=0.6)
    u["coef"][4] = 0.0                                       # a key no lane has: the round trip drops it
    lanes = [lane_operand(u, t) for t in range(nl)]
    for t, l in enumerate(lanes):
        assert np.all(np.any(l["coef"] != 0.0, axis=1)) and np.array_equal(l["cen"], u["cen"][:, t])
        assert set(map(int, l["keys"])) == {int(k) for k, row in zip(u["keys"], u["coef"]) if np.any(row[:, t] != 0.0)}
    back = union_operand(lanes)
    held = np.any(u["coef"] != 0.0, axis=(1, 2))
    assert not held[4] and np.array_equal(back["keys"], u["keys"][held]) and np.array_equal(back["coef"], u["coef"][held])
    assert np.array_equal(back["cen"], u["cen"]) and np.array_equal(back["ind"], u["ind"])
    for t in range(nl):
        again = lane_operand(back, t)
        assert np.array_equal(again["keys"], lanes[t]["keys"]) and np.array_equal(again["coef"], lanes[t]["coef"])


def test_compound_op_codes_are_the_compositions_they_name():
    """12-17 on a tiny hand-written case, against their definitions worked out by hand (nothing is near the threshold: simplify() only merges)."""
    k1, k2, k3 = 1, 4, 1 << 14
    K = lambda *ks: np.array(ks, dtype=np.uint64)
    a = dict(sz=3, keys=K(k1, k2), coef=np.array([[1.0, 2.0, 3.0], [0.5, 0.0, -1.0]]), cen=np.array([1.0, 0.0, -1.0]), ind=np.array([0.1, 0.2, 0.3]))
    b = dict(sz=3, keys=K(k2, k3), coef=np.array([[1.5, 1.0, 1.0], [2.0, 2.0, 2.0]]), cen=np.array([0.0, 1.0, 0.0]), ind=np.array([0.0, 0.1, 0.0]))
    c = dict(sz=3, keys=K(k1), coef=np.array([[-1.0, 1.0, 0.0]]), cen=np.array([2.0, 2.0, 2.0]), ind=np.array([0.5, 0.0, 0.0]))
    d = dict(sz=3, keys=K(k3), coef=np.array([[1.0, 0.0, 0.0]]), cen=np.array([0.0, 0.0, 1.0]), ind=np.array([0.0, 0.0, 0.25]))
    s = dict(sz=1, keys=K(k2), coef=np.array([[4.0]]), cen=np.array([3.0]), ind=np.array([0.5]))
    o = oracle_op(12, [a, b, c], r=-1)
    assert list(o["keys"]) == [k1, k2, k3] and np.array_equal(o["coef"], [[0.0, 3.0, 3.0], [2.0, 1.0, 0.0], [2.0, 2.0, 2.0]])
    assert np.array_equal(o["cen"], [3.0, 3.0, 1.0]) and np.allclose(o["ind"], [0.6, 0.3, 0.3], rtol=0, atol=1e-15)
    o = oracle_op(12, [a, b, s], r=1)
    assert list(o["keys"]) == [k1, k2, k3] and np.array_equal(o["coef"], [[1.0, 2.0, 3.0], [2.0, 5.0, 0.0], [2.0, 2.0, 2.0]])
    assert np.array_equal(o["cen"], [1.0, 4.0, -1.0]) and np.allclose(o["ind"], [0.1, 0.8, 0.3], rtol=0, atol=1e-15)
    o = oracle_op(13, [a, b, c, d])
    assert list(o["keys"]) == [k1, k2, k3] and np.array_equal(o["coef"], [[0.0, 3.0, 3.0], [2.0, 1.0, 0.0], [3.0, 2.0, 2.0]]) and np.array_equal(o["cen"], [3.0, 3.0, 2.0])
    s2 = dict(sz=1, keys=K(k1, k2), coef=np.array([[1.0], [1.0]]), cen=np.array([1.0]), ind=np.array([0.25]))
    s3 = dict(sz=1, keys=K(k3), coef=np.array([[2.0]]), cen=np.array([-1.0]), ind=np.array([1.0]))
    o = oracle_op(14, [s, s2, s3], consts=[2.0, -1.0, 0.5])
    assert list(o["keys"]) == [k1, k2, k3] and np.array_equal(o["coef"], [[-1.0], [7.0], [1.0]]) and np.array_equal(o["cen"], [4.5]) and np.array_equal(o["ind"], [1.75])
    o = oracle_op(15, [s], r=2)
    assert list(o["keys"]) == [k2] and np.array_equal(o["coef"], [[0.0, 0.0, 4.0]]) and np.array_equal(o["cen"], [0.0, 0.0, 3.0]) and np.array_equal(o["ind"], [0.0, 0.0, 0.5])
    w = dict(sz=3, keys=K(k1), coef=np.array([[1.0, 0.0, 0.0]]), cen=np.array([0.0, 1.0, 0.0]), ind=np.zeros(3))
    o = oracle_op(16, [a, w, c], consts=[0.0, 0.0, 2.0])     # cross(w, (0, 0, 2)): e_x x 2 e_z = -2 e_y on k1, e_y x 2 e_z = 2 e_x in the centre
    assert list(o["keys"]) == [k1, k2] and np.array_equal(o["coef"], [[0.0, 1.0, 3.0], [0.5, 0.0, -1.0]]) and np.array_equal(o["cen"], [5.0, 2.0, 1.0])
    m = dict(sz=9, keys=K(k1), coef=np.arange(9.0).reshape(1, 9), cen=np.arange(9.0) * 2, ind=np.arange(9.0) * 0.5)
    o = oracle_op(17, [m])
    assert np.array_equal(o["coef"], [[0, 3, 6, 1, 4, 7, 2, 5, 8]]) and np.array_equal(o["cen"][[1, 3]], [6.0, 2.0]) and np.array_equal(o["ind"][[2, 6]], [3.0, 1.0])


def _run_k128(body):
    env = dict(os.environ, ARMOUR_KEY128="1")
    env.pop("ARMOUR_HIP_LIB", None)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_pz_tv_ops as t; t.%s()" % (ROOT, os.path.join(ROOT, "tests"), body)
    return subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)


def _body_k128_oracle():
    """(runs with ARMOUR_KEY128=1)"""
    from oracle import cpu_oracle as orc
    assert orc.KEY_WORDS == 2
    n = 8
    sin3 = 1 << (7 * n + 2 * 3)                              # bits 62-63: sin_3^3 * sin_3 carries into bit 64, the next field
    a = dict(sz=1, keys=[3 * sin3], coef=np.array([[2.0]]), cen=np.zeros(1), ind=np.zeros(1))
    b = dict(sz=1, keys=[sin3], coef=np.array([[3.0]]), cen=np.zeros(1), ind=np.zeros(1))
    p = oracle_op(2, [a, b])
    assert list(p["keys"]) == [3 * sin3 + sin3] == [1 << 64] and p["coef"][0, 0] == 6.0
    # two operands whose keys differ only above bit 63: the raw terms come out sorted by the high word, equal sums merged
    lo = 5
    x = dict(sz=1, keys=[lo + (1 << 64), lo + (2 << 64)], coef=np.array([[1.0], [2.0]]), cen=np.zeros(1), ind=np.zeros(1))
    y = dict(sz=1, keys=[lo + (1 << 64), lo + (2 << 64)], coef=np.array([[3.0], [5.0]]), cen=np.zeros(1), ind=np.zeros(1))
    p = oracle_op(2, [x, y])
    assert list(p["keys"]) == [2 * lo + (2 << 64), 2 * lo + (3 << 64), 2 * lo + (4 << 64)] and np.array_equal(p["coef"][:, 0], [3.0, 11.0, 10.0])
    print("k128 oracle ok", flush=True)


def test_k128_oracle_carries_across_bit_63_and_sorts_by_the_high_word():
    r = _run_k128("_body_k128_oracle")
    assert r.returncode == 0 and "k128 oracle ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
