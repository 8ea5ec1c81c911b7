"""Polynomial-zonotope operators one at a time (RT/PZsparse.cu).

CPU part: algebraic identities of the oracle's operators (the reference has no unit tests for them).
GPU part: the wave-level device operators (armour_amd/csrc/pz_wave.h, through the armour_debug_pz_op hook) against
the oracle on the same random operands -- identical key lists, |d coeff| <= 1e-13 (summation order of equal keys is
the only difference), independent radii <= 1e-12 -- over the three sorting regimes of the device code (<= 64 raw
terms in registers, merge of sorted runs, LDS bitonic) and the reference's corner cases: empty polynomials, the
1-bit tracking-error fields carrying into their neighbours when squared (RT/PZsparse.cu:938-940), coefficients that
straddle SIMPLIFY_THRESHOLD."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_F = 7
THR = 5e-4


def rand_keys(rng, count, kinds=("k", "qde", "cos", "sin", "qdae", "qddae"), n_f=N_F):
    """sorted unique monomial keys in the layout of RT/PZsparse.h:23-40 (n_f = 8: the 128-bit ABI's, fields up to bit 71, as Python integers)"""
    keys = set()
    while len(keys) < count:
        key = 0
        for _ in range(int(rng.integers(1, 4))):
            kind = kinds[int(rng.integers(len(kinds)))]
            j = int(rng.integers(n_f))
            shift = {"k": 2 * j, "qde": 2 * n_f + j, "qdae": 3 * n_f + j, "qddae": 4 * n_f + j, "cos": 5 * n_f + 2 * j, "sin": 7 * n_f + 2 * j}[kind]
            key += 1 << shift                      # plain integer add: repeated 1-bit variables carry, as in the reference
        keys.add(key)
    return np.array(sorted(keys), dtype=np.uint64 if n_f <= 7 else object)


def rand_pz(rng, sz, count, scale=1.0, small_frac=0.3, n_f=N_F):
    coef = rng.normal(size=(count, sz)) * scale
    small = rng.random(count) < small_frac
    coef[small] *= THR / max(scale, 1e-12) * rng.uniform(0.2, 3.0, (small.sum(), 1))   # straddle the prune threshold
    return dict(sz=sz, keys=rand_keys(rng, count, n_f=n_f), coef=coef, cen=rng.normal(size=sz), ind=np.abs(rng.normal(size=sz)) * 0.01)


def label_seed(label):
    """a seed that is the same in every process (hash() of a string is not)"""
    return zlib.crc32(label.encode()) % (2**31)


# Operand shapes of every op code of armour_debug_pz_op (entries per coefficient); 12 with r >= 0 takes its third operand 1x1
OP_SHAPES = {0: (9, 3), 1: (9, 9), 2: (1, 1), 3: (1, 3), 4: (3, 3), 5: (3, 3), 6: (3, 1), 7: (1, 1, 1), 8: (3,), 9: (3,), 10: (3, 3), 11: (1, 1),
             12: (3, 3, 3), 13: (3, 3, 3, 3), 14: (1, 1, 1), 15: (1,), 16: (3, 3, 3), 17: (9,)}
OUT_SZ = {0: 3, 1: 9, 2: 1, 3: 3, 4: 3, 5: 3, 6: 3, 7: 3, 8: 3, 9: 3, 10: 3, 11: 1, 12: 3, 13: 3, 14: 1, 15: 3, 16: 3, 17: 9}


def oracle_op(op, ops, consts=None, r=0):
    """Op codes 0-11: the oracle's operator.  12-17, the chain's compound operators, are compositions of those -- each step with its own
    simplify(), as the reference's chain writes them (RT/Dynamics.cu) -- and min_margin is the smallest of the steps'."""
    from oracle.cpu_oracle import pz_op
    if op <= 11:
        return pz_op(op, ops, consts=consts, r=r)
    consts = np.zeros(4) if consts is None else np.asarray(consts, dtype=np.float64)
    steps = []

    def step(code, operands, sz, **kw):
        out = pz_op(code, operands, **kw)
        steps.append(out["min_margin"])
        return dict(out, sz=sz)
    if op == 12:      # sum3: (a + b) + c, c a 3x1 (r < 0) or a 1x1 into entry r
        ab = step(4, [ops[0], ops[1]], 3)
        out = step(4, [ab, ops[2]], 3) if r < 0 else step(6, [ab, ops[2]], 3, r=r)
    elif op == 13:    # sum4: ((a + b) + c) + d
        out = step(4, [step(4, [step(4, [ops[0], ops[1]], 3), ops[2]], 3), ops[3]], 3)
    elif op == 14:    # comb3: (sa a + sb b) + sc c
        out = step(11, [step(11, [ops[0], ops[1]], 1, consts=[consts[0], consts[1]]), ops[2]], 1, consts=[1.0, consts[2]])
    elif op == 15:    # embedOneDim: addOneDimPZ(PZsparse(0, 0, 0), a, r)
        zero = dict(sz=3, keys=ops[0]["keys"][:0], coef=np.zeros((0, 3)), cen=np.zeros(3), ind=np.zeros(3))
        out = step(6, [zero, ops[0]], 3, r=r)
    elif op == 16:    # (a + cross(w, consts)) + c
        out = step(4, [step(4, [ops[0], step(8, [ops[1]], 3, consts=consts)], 3), ops[2]], 3)
    elif op == 17:    # transpose of a 3x3: keys unchanged, no simplify()
        tr = lambda v: np.asarray(v).reshape(-1, 3, 3).transpose(0, 2, 1).reshape(np.shape(v))
        return dict(keys=ops[0]["keys"], coef=tr(ops[0]["coef"]) if len(ops[0]["keys"]) else np.zeros((0, 9)), cen=tr(ops[0]["cen"]), ind=tr(ops[0]["ind"]), min_margin=1e300)
    else:
        raise ValueError(op)
    out["min_margin"] = min(steps)
    return out


# ------------------------------------------------------------------ CPU: oracle identities
def test_oracle_simplify_invariants_and_identities():
    rng = np.random.default_rng(0)
    a, b = rand_pz(rng, 3, 40), rand_pz(rng, 3, 55)
    s = oracle_op(4, [a, b])
    assert np.all(np.diff(s["keys"].astype(np.int64)) > 0)                          # sorted, unique
    assert np.all(np.linalg.norm(s["coef"], axis=1) > THR)                          # nothing below the threshold survives
    assert np.allclose(s["cen"], a["cen"] + b["cen"])
    # a - a: every monomial cancels, the radius is 2*ind (the reference adds the independents, RT/PZsparse.cu:829)
    z = oracle_op(5, [a, a])
    assert len(z["keys"]) == 0 and np.allclose(z["cen"], 0) and np.allclose(z["ind"], 2 * a["ind"])
    # interval hull of a product contains the product of sampled values
    x, y = rand_pz(rng, 1, 12, small_frac=0), rand_pz(rng, 1, 9, small_frac=0)
    p = oracle_op(2, [x, y])
    hull = lambda q: (q["cen"][0] - q["ind"][0] - np.abs(q["coef"]).sum(), q["cen"][0] + q["ind"][0] + np.abs(q["coef"]).sum())
    lo, hi = hull(p)
    for _ in range(200):
        # evaluate both factors at a random point of the unit box (one value per distinct variable field is not needed:
        # every monomial is an independent generator in [-1,1] for containment purposes only if keys differ; use +-1 corners)
        sx = rng.choice([-1.0, 1.0], len(x["keys"])); sy = rng.choice([-1.0, 1.0], len(y["keys"]))
        vx = x["cen"][0] + (x["coef"][:, 0] * sx).sum() * 0  # centre-only sample keeps the check exact
        vy = y["cen"][0] + (y["coef"][:, 0] * sy).sum() * 0
        assert lo - 1e-12 <= vx * vy <= hi + 1e-12
    # cross(a, c) = -cross(c, a) for a constant c (centre and coefficients; the radii are equal)
    c = rng.normal(size=3)
    u, v = oracle_op(8, [a], consts=c), oracle_op(9, [a], consts=c)
    assert np.array_equal(u["keys"], v["keys"]) and np.allclose(u["coef"], -v["coef"]) and np.allclose(u["cen"], -v["cen"]) and np.allclose(u["ind"], v["ind"])


def test_oracle_key_carry_is_plain_integer_addition():
    """qde_0 * qde_0: the 1-bit field overflows into qde_1's bit, exactly as u64 addition does (RT/PZsparse.cu:938-940)."""
    k = np.array([1 << (2 * N_F)], dtype=np.uint64)
    a = dict(sz=1, keys=k, coef=np.array([[2.0]]), cen=np.array([0.0]), ind=np.array([0.0]))
    p = oracle_op(2, [a, a])
    assert list(p["keys"]) == [1 << (2 * N_F + 1)] and p["coef"][0, 0] == 4.0


# ------------------------------------------------------------------ GPU: device operators vs oracle
def _compare(dev, ref, ctol=1e-13, itol=1e-12):
    assert dev["flags"] == 0
    assert np.array_equal(dev["keys"], ref["keys"]), (len(dev["keys"]), len(ref["keys"]))
    if len(ref["keys"]):
        assert np.abs(dev["coef"] - ref["coef"]).max() <= ctol * max(1.0, np.abs(ref["coef"]).max())
    assert np.abs(dev["cen"] - ref["cen"]).max() <= ctol * max(1.0, np.abs(ref["cen"]).max())
    assert np.abs(dev["ind"] - ref["ind"]).max() <= itol * max(1.0, np.abs(ref["ind"]).max())


def _device_margin(out):
    """|norm - threshold| / threshold of the operator's nearest verdict, from the squared-domain distance armour_debug_pz_op hands back, as
    armour_get_prune_margin converts it (the kept side's figure); 1e300: no verdict."""
    if not np.isfinite(out["margin_sq"]):
        return 1e300
    return abs(np.sqrt(out["thr_sq"] + out["margin_sq"]) - THR) / THR


def margin_agrees(dev_margin, ref, tol=2e-10):
    """The device's margin against the oracle's min_margin.  Equal when the nearest verdict kept its monomial; when it pruned it the device
    reports the kept side's figure, sqrt(1 + 2r - r^2) - 1 = r - r^2 + ..., and a zero norm -- which the oracle leaves out -- counts as r = 1."""
    r = min(ref, 1.0)
    return np.sqrt(1.0 + 2.0 * r - r * r) - 1.0 - tol <= dev_margin <= ref + tol


@pytest.fixture(scope="module")
def dev():
    from armour_amd.planner import ArmourNLP
    return ArmourNLP(T=100)


CASES = [
    # (op, operand (sz, count) list, label)
    (0, [(9, 3), (3, 120)], "MV merge (4 runs)"), (0, [(9, 0), (3, 200)], "MV constant matrix"), (0, [(9, 3), (3, 5)], "MV small"),
    (1, [(9, 150), (9, 3)], "MM merge (short second operand)"), (1, [(9, 6), (9, 3)], "MM small"),
    (2, [(1, 25), (1, 35)], "SS bitonic 0.9k raw"), (2, [(1, 7), (1, 8)], "SS <= 64 raw"), (2, [(1, 5), (1, 150)], "SS merge"),
    (2, [(1, 0), (1, 0)], "SS both empty"), (3, [(1, 0), (3, 180)], "SV mass times vector"),
    (4, [(3, 300), (3, 280)], "add merge"), (4, [(3, 20), (3, 30)], "add small"), (4, [(3, 0), (3, 77)], "add empty + x"),
    (5, [(3, 250), (3, 250)], "sub merge"), (6, [(3, 140), (1, 2)], "addOneDim"), (7, [(1, 90), (1, 70), (1, 110)], "stack 3-way merge"),
    (7, [(1, 10), (1, 0), (1, 12)], "stack with an empty entry"), (8, [(3, 333)], "cross(a, const)"), (9, [(3, 64)], "cross(const, a)"),
    (10, [(3, 30), (3, 25)], "cross(a, b) bitonic"), (10, [(3, 6), (3, 90)], "cross(a, b) merge"),
    # round 6: 2 049 .. ~3 000 raw terms in more than eight runs -- the two halves of the tree's last level sorted apart, then one bitonic merge (MulEval::split_merge)
    (10, [(3, 36), (3, 59)], "cross(a, b) split merge 2219 raw"), (10, [(3, 46), (3, 45)], "cross(a, b) split merge, runs along b"), (2, [(1, 40), (1, 60)], "SS split merge 2500 raw"),
    (0, [(9, 10), (3, 230)], "MV split merge 2540 raw"), (2, [(1, 55), (1, 62)], "SS 3527 raw: no split fits, the whole network"),
    (10, [(3, 6), (3, 7)], "cross(a, b) <= 64 raw"), (10, [(3, 0), (3, 40)], "cross(constant a, b)"), (10, [(3, 25), (3, 0)], "cross(a, constant b)"), (11, [(1, 200), (1, 190)], "s1*a + s2*b"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("op,shapes,label", CASES, ids=[c[2] for c in CASES])
def test_device_operator_matches_oracle(dev, op, shapes, label):
    rng = np.random.default_rng(abs(hash(label)) % (2**31))
    for trial in range(3):
        ops = [rand_pz(rng, sz, cnt, scale=float(rng.choice([1.0, 0.05]))) for sz, cnt in shapes]
        if "split merge" in label or "no split fits" in label:   # thousands of raw terms: coefficients small enough that most products are pruned and the result fits a work slot (1024 monomials)
            ops = [rand_pz(rng, sz, cnt, scale=0.008 if op == 0 else 0.02) for sz, cnt in shapes]
        if op in (5, 11) and trial == 0:
            ops[1]["keys"] = ops[0]["keys"][:len(ops[1]["keys"])].copy() if len(ops[0]["keys"]) >= len(ops[1]["keys"]) else ops[1]["keys"]
        consts = rng.normal(size=4)
        if op in (8, 9) and trial == 1:
            consts[0] = 0.0                          # a zero component (the Kinova link offsets have them)
        r = int(rng.integers(3))
        ref = oracle_op(op, ops, consts=consts, r=r)
        if ref["min_margin"] < 1e-9:
            continue                                 # a coefficient within 1e-9 of the threshold: either verdict is legitimate
        out = dev.debug_pz_op(op, ops, consts=consts, r=r, out_cap=max(4096, len(ref["keys"]) + 8))
        _compare(out, ref)
        # the prune margin the device recorded for this operator (armour_get_prune_margin is the minimum of these over a build) equals the
        # oracle's: the same verdicts on the same sums, the one nearest to the threshold found by both
        assert margin_agrees(_device_margin(out), ref["min_margin"]), (label, trial, _device_margin(out), ref["min_margin"])
        # second independent radius: same rule with ind2 in place of ind (fused nominal / interval RNEA)
        ops2 = [dict(o, ind2=o["ind"] * (1.5 + i)) for i, o in enumerate(ops)]
        ref2 = oracle_op(op, [dict(o, ind=o["ind2"]) for o in ops2], consts=consts, r=r)
        out2 = dev.debug_pz_op(op, ops2, consts=consts, r=r, out_cap=max(4096, len(ref["keys"]) + 8))
        assert np.array_equal(out2["keys"], ref["keys"]) and np.abs(out2["ind"] - ref["ind"]).max() <= 1e-12 * max(1.0, np.abs(ref["ind"]).max())
        assert np.abs(out2["ind2"] - ref2["ind"]).max() <= 1e-12 * max(1.0, np.abs(ref2["ind"]).max())


@pytest.mark.gpu
def test_device_key_carry_and_capacity_flags(dev):
    k = np.array([1 << (2 * N_F)], dtype=np.uint64)
    a = dict(sz=1, keys=k, coef=np.array([[2.0]]), cen=np.array([0.0]), ind=np.array([0.0]))
    p = dev.debug_pz_op(2, [a, a])
    assert list(p["keys"]) == [1 << (2 * N_F + 1)] and p["coef"][0, 0] == 4.0 and p["flags"] == 0
    # more raw terms than the LDS sort buffer holds: flagged (the planner then retries with larger buffers), never silent
    rng = np.random.default_rng(5)
    big = [rand_pz(rng, 1, 90, small_frac=0), rand_pz(rng, 1, 90, small_frac=0)]
    out = dev.debug_pz_op(2, big)
    assert out["flags"] & 1


# ------------------------------------------------------------------ which sorter an operator takes (restated from pz_wave.h sort_terms; used to
# choose sizes on both sides of every boundary -- the kernel's raw-term count is checked against raw_terms())
PRODUCTS = (0, 1, 2, 3, 10)


def raw_terms(op, counts):
    return (counts[0] + 1) * (counts[1] + 1) - 1 if op in PRODUCTS else counts[0] if op in (8, 9, 15, 17) else sum(counts)


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def sorter_of(op, counts, cap_key, cap_raw):
    """'none' (one ordered pass), 'count', 'tree', 'rank', 'split', 'network', 'merge' (sums: pairwise merge), 'search' (sums: binary searches), 'overflow'"""
    if op in (8, 9, 15, 17):
        return "none"
    N = raw_terms(op, counts)
    if op in PRODUCTS:
        na1, nb1 = counts[0] + 1, counts[1] + 1
        can_tree = 2 * N <= cap_key and 2 * N <= cap_raw
        can_rank = min(na1, nb1) <= 8 and na1 + nb1 <= cap_key
        if N > cap_raw or (N > 64 and not (can_tree or can_rank) and next_pow2(N) > cap_key):
            return "overflow"
        if N <= 64:
            return "count"
        if can_tree:
            return "tree"
        if can_rank:
            return "rank"
        nr, d1 = min(na1, nb1), max(na1, nb1)
        levels = 0
        while (1 << levels) < nr:
            levels += 1
        P, C = next_pow2(N), min(cap_key, cap_raw)
        N1 = (d1 << (levels - 1)) - 1 if levels >= 1 else 0
        N2 = N - N1
        ok = levels >= 1 and N2 > 0 and P <= C and N1 <= P // 2 and N2 <= P // 2 and 2 * N1 <= C and N1 + 2 * N2 <= P
        return "split" if ok else "network"
    if N > cap_raw or (N > 8 and N > cap_key):
        return "overflow"
    return "count" if N <= 8 else "merge" if 2 * N <= cap_key and 2 * N <= cap_raw else "search"


# ------------------------------------------------------------------ the compound operators of the chain, and the builds' sort-buffer shapes
COMPOUND_CASES = [
    # (op, operand (sz, count) list, r, label)
    (12, [(3, 3), (3, 2), (3, 2)], -1, "sum3 <= 8 raw"), (12, [(3, 120), (3, 100), (3, 90)], -1, "sum3 merge"), (12, [(3, 120), (3, 100), (1, 30)], 1, "sum3 with a 1x1 into entry 1"),
    (12, [(3, 0), (3, 40), (1, 0)], 2, "sum3 with empty operands"), (13, [(3, 90), (3, 70), (3, 110), (3, 60)], 0, "sum4 merge"), (13, [(3, 2), (3, 2), (3, 1), (3, 2)], 0, "sum4 <= 8 raw"),
    (14, [(1, 90), (1, 70), (1, 110)], 0, "comb3"), (14, [(1, 3), (1, 0), (1, 4)], 0, "comb3 <= 8 raw"), (15, [(1, 2)], 0, "embedOneDim entry 0"), (15, [(1, 200)], 2, "embedOneDim entry 2"),
    (16, [(3, 120), (3, 100), (3, 90)], 0, "sum3 of a, cross(w, const), c"), (16, [(3, 30), (3, 0), (3, 20)], 0, "sum3 of a, cross(constant w, const), c"),
    (17, [(9, 8)], 0, "transpose33"), (17, [(9, 0)], 0, "transpose33 of a constant"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("op,shapes,r,label", COMPOUND_CASES, ids=[c[3] for c in COMPOUND_CASES])
def test_device_compound_operator_matches_the_composition(dev, op, shapes, r, label):
    """Op codes 12-17 of the hook -- the per-step chain's sum3 / sum4 / comb3 / embedOneDim / transpose33, which no test reached one at a time --
    against the oracle's composition of the operators they fuse, at the tolerances above; no trial is skipped (the seeds leave every margin >= 1e-9)."""
    rng = np.random.default_rng(label_seed(label))
    for trial in range(3):
        ops = [rand_pz(rng, sz, cnt, scale=float(rng.choice([1.0, 0.05]))) for sz, cnt in shapes]
        if trial == 0 and len(ops) > 1 and ops[0]["sz"] == ops[1]["sz"] and len(ops[0]["keys"]) >= len(ops[1]["keys"]):
            ops[1]["keys"] = ops[0]["keys"][:len(ops[1]["keys"])].copy()     # shared keys: runs of equal keys, cancellations
        consts = rng.normal(size=4)
        ref = oracle_op(op, ops, consts=consts, r=r)
        assert ref["min_margin"] >= 1e-9, (label, trial)
        ops2 = [dict(o, ind2=o["ind"] * (1.5 + i)) for i, o in enumerate(ops)]
        ref2 = oracle_op(op, [dict(o, ind=o["ind2"]) for o in ops2], consts=consts, r=r)
        out = dev.debug_pz_op(op, ops2, consts=consts, r=r)
        _compare(out, ref)
        assert np.abs(out["ind2"] - ref2["ind"]).max() <= 1e-12 * max(1.0, np.abs(ref2["ind"]).max())
        assert margin_agrees(_device_margin(out), ref["min_margin"]), (label, trial, _device_margin(out), ref["min_margin"])


# (op, counts, scale): products of 503 | 524 raw terms around 2N = 1 024 and 1 023 | 1 055 around next_pow2(N) = 1 024 -- 1 007 | 1 055 and 2 057 | 2 115 for
# the same two at 2 048, 2 024 for the whole network there --; a product with two runs over 1 021 keys, nl + ns = 1 024 exactly, and four runs over
# 1 019 and 600; sums of 510 | 522 terms around 2N = 1 024, 1 024 around N = 1 024 and 2N = 2 048, 2 000 around N = 2 048 and 2N = 4 096
SHAPE_SIZES = [(2, (20, 23), 0.2), (2, (20, 24), 0.2), (2, (31, 31), 0.05), (2, (31, 32), 0.05), (2, (41, 48), 0.02), (2, (45, 45), 0.02), (2, (44, 44), 0.02),
               (0, (1, 1021), 1e-4), (0, (3, 1019), 1e-4), (0, (3, 600), 0.008),
               (4, (250, 260), 1.0), (4, (260, 262), 1.0), (4, (512, 512), 1.0), (4, (1000, 1000), 1.0)]
SHAPES = [(0, 0), (1024, 2048), (2048, 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("caps", SHAPES, ids=["full width", "1024/2048", "2048/4096"])
def test_device_operator_at_the_builds_sort_buffer_shapes(dev, caps):
    """The builds do not run with full-width key buffers: the fourth wave of a four-wave block has 1 024 keys / 2 048 raw terms, every wave of the
    128-bit ABI cap / 2 keys, and sort_terms picks the sorter from the two separately.  Sizes on both sides of 2N <= cap_key, nl + ns <= cap_key and
    next_pow2(N) <= cap_key, at every shape that holds them; beyond the last the buffers overflow, which must be flagged."""
    ck, cr = caps if caps != (0, 0) else (4096, 4096)
    taken = set()
    for op, counts, scale in SHAPE_SIZES:
        rng = np.random.default_rng(label_seed(f"shape {op} {counts}"))
        ops = [rand_pz(rng, sz, cnt, scale=scale) for sz, cnt in zip(OP_SHAPES[op], counts)]
        if op == 4 and sum(counts) > 1024:
            ops[1]["keys"] = ops[0]["keys"].copy()           # (so that the sum fits a 1 024-monomial slot)
        consts, r = rng.normal(size=4), 0
        sorter = sorter_of(op, counts, ck, cr)
        out = dev.debug_pz_op(op, ops, consts=consts, r=r, cap_key=caps[0], cap_raw=caps[1])
        if sorter == "overflow":
            assert out["flags"] & 1, (op, counts, caps, out["flags"])
            continue
        ref = oracle_op(op, ops, consts=consts, r=r)
        assert ref["min_margin"] >= 1e-9 and len(ref["keys"]) <= 1024, (op, counts)
        _compare(out, ref)
        assert out["raw_terms"] == raw_terms(op, counts)
        assert margin_agrees(_device_margin(out), ref["min_margin"]), (op, counts, caps)
        taken.add(sorter)
    assert taken >= ({"tree", "rank", "split", "network", "merge", "search"} if caps != (0, 0) else {"tree", "rank", "split", "merge"}), taken


# ------------------------------------------------------------------ 128-bit keys (the second ABI: libarmour_hip_k128.so, oracle/liboracle_k128.so)
def _body_k128_device():
    """(runs with ARMOUR_KEY128=1)  The operator table above and the compound operators through the hook with 8-factor keys (fields up to bit 71,
    keys equal in the low word), at the build's own sort-buffer shape (key_cap(cap) = cap / 2 keys) and at full width, against the 128-bit oracle."""
    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP
    assert _lib.KEY_WORDS == 2
    dev = ArmourNLP(T=100)
    worst = {"coef": 0.0, "cen": 0.0, "ind": 0.0}
    table = [(op, shapes, None, label) for op, shapes, label in CASES] + list(COMPOUND_CASES)
    for op, shapes, r_fixed, label in table:
        rng = np.random.default_rng(label_seed("k128 " + label))
        counts = tuple(cnt for _, cnt in shapes)
        scale = (0.008 if op == 0 else 0.02) if ("split merge" in label or "no split fits" in label) else 1.0
        # the build's shapes: 4 096 raw terms with 2 048 keys, and -- what a launch that overflowed those is repeated with -- 8 192 with 4 096
        build_caps = (2048, 4096) if sorter_of(op if op != 7 else 4, counts, 2048, 4096) != "overflow" else (4096, 8192)
        consts, r = rng.normal(size=4), int(rng.integers(3)) if r_fixed is None else r_fixed
        ops = [rand_pz(rng, sz, cnt, scale=scale, n_f=8) for sz, cnt in shapes]
        assert sum(len(o["keys"]) for o in ops) < 8 or any(int(k) >> 64 for o in ops for k in o["keys"])
        ref = oracle_op(op, ops, consts=consts, r=r)
        assert ref["min_margin"] >= 1e-9, label
        for caps in (build_caps, (4096, 4096)):
            out = dev.debug_pz_op(op, ops, consts=consts, r=r, cap_key=caps[0], cap_raw=caps[1])
            _compare(out, ref)
            assert margin_agrees(_device_margin(out), ref["min_margin"]), (label, caps)
            if len(ref["keys"]):
                worst["coef"] = max(worst["coef"], np.abs(out["coef"] - ref["coef"]).max() / max(1.0, np.abs(ref["coef"]).max()))
            worst["cen"] = max(worst["cen"], np.abs(out["cen"] - ref["cen"]).max() / max(1.0, np.abs(ref["cen"]).max()))
            worst["ind"] = max(worst["ind"], np.abs(out["ind"] - ref["ind"]).max() / max(1.0, np.abs(ref["ind"]).max()))
    # the carry across the word boundary: with 8 factors sin_3 is bits 62-63, and sin_3^3 * sin_3 carries into bit 64, the next field
    sin3 = 1 << (7 * 8 + 2 * 3)
    a = dict(sz=1, keys=[3 * sin3], coef=np.array([[2.0]]), cen=np.zeros(1), ind=np.zeros(1))
    b = dict(sz=1, keys=[sin3], coef=np.array([[3.0]]), cen=np.zeros(1), ind=np.zeros(1))
    p = dev.debug_pz_op(2, [a, b])
    assert list(p["keys"]) == [1 << 64] and p["coef"][0, 0] == 6.0 and p["flags"] == 0
    # <= 64 raw terms, ranked by counting on keys broadcast with pzkey_readlane, and a tree merge: keys that differ only in the high word
    rng = np.random.default_rng(64)
    lo = 5 + (1 << 20)
    for na, nb in ((7, 6), (30, 25)):
        his = [sorted(rng.choice(200, n, replace=False).tolist()) for n in (na, nb)]
        ops = [dict(rand_pz(rng, 3, len(h), small_frac=0.0), keys=np.array([lo + (int(v) << 64) for v in h], dtype=object)) for h in his]
        ref = oracle_op(10, ops)
        assert ref["min_margin"] >= 1e-9 and len(ref["keys"]) > 8 and all((int(k) & ((1 << 64) - 1)) == 2 * lo for k in ref["keys"][-3:])
        _compare(dev.debug_pz_op(10, ops), ref)
        _compare(dev.debug_pz_op(10, ops, cap_key=2048, cap_raw=4096), ref)
    print("k128 worst", {k: "%.3g" % v for k, v in worst.items()}, flush=True)
    print("k128 device ok", flush=True)


@pytest.mark.gpu
def test_k128_operators_match_the_128_bit_oracle():
    """No operator had been run on keys whose distinguishing bits lie above bit 63: the hook handed back the low word of a key and the oracle's
    took 64-bit keys.  Both now pass a key in the library's own width."""
    env = dict(os.environ, ARMOUR_KEY128="1")
    env.pop("ARMOUR_HIP_LIB", None)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_pz_ops as t; t._body_k128_device()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "k128 device ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout[-400:])
