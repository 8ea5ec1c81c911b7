"""The exact-layout (EX) kernels against the six-slot kernels they replace, bit for bit, at the shapes where a collision block's loading can go wrong.

An EX launch loads a block's slicing tables and planes by a fixed plan: one or two rounds of (monomial, axis) tasks per thread -- the launch
picks the one-round kernel where max_pairs * 3 * max_link <= 256 -- and six planes per wave from addresses of the launch plan.  The reference is
the SAME problems on a second handle with ARMOUR_OPT_P2_EX = 0: the six-slot kernel with predicated loads and its own address arithmetic, which
shares none of that.  Every double of g and jac must be the same on the uint64 view, through the asynchronous device entry and a prepared
3-step graph, at a random k, at +1, at -1 and from rest at k = 0 (the points of tests/golden/make_p2_ex_rows.py, whose helpers this file uses).

Shapes: Kinova, box obstacles.  O = 8 puts eight (link, time step) records under every 64-row block (a block starts at a multiple of 64, which
is a multiple of O: never the nine that the plan's bound max_pairs = 63 / O + 2 allows for); O = 13 has the record boundaries off the block boundaries and a partial
last block; O = 20 is the headline's; O = 64 and O = 100 have a block inside one record and across two; B = 3 is the pointer path with the shared
mask and per-problem bases, B = 8 recomputes d.  T = 2 keeps Q at a few hundred rows.

Round counts.  A block has npairs * 3 * max_link slicing tasks, npairs the records it really touches; the launch decides by the plan's bound,
max_pairs * 3 * max_link <= 256 -> one round, which is safe only because npairs <= max_pairs.  At T = 2 the link PZs of the problems that build
have at most 9 monomials: no block there has a task beyond thread 255.  The case `o8_t8` (O = 8, T = 8, Q = 448: link PZs of up to 12
monomials, 8 * 3 * 12 = 288 tasks in every block) is the one whose blocks have LIVE second-round tasks -- the test asserts that from the
tables -- so a launch that dropped the second round there would lose terms of the eighth record's link PZ and miss the reference's bits.
The seeds are the first, counting up from the case's base, whose two problem sets build and take the EX kernel (searched once with the parent
commit's library; a problem's reach sets can outgrow the build's capacity at steps this long).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_p2_ex_rows as gen  # noqa: E402

P2_BLOCK = 256
N = 7
# name: (O, T, seeds of the B problems, d recomputed)
CASES = {
    "o8": (8, 2, (2001,), False),
    "o8_t8": (8, 8, (2026,), False),
    "o13": (13, 2, (2100,), False),
    "o20": (20, 2, (2203,), False),
    "o64": (64, 2, (2308,), False),
    "o100": (100, 2, (2400,), False),
    "o20_b3": (20, 2, (2203, 2205, 2206), False),
    "o20_b8": (20, 2, (2203, 2205, 2206, 2208, 2212, 2221, 2224, 2227), True),
}
ENTRIES = ("device", "steps")


def expected_rounds(O, max_link):
    """The rule of armour_p2_launch: one round where the (63 / O + 2) records a block can touch, three axes and max_link monomials fit P2_BLOCK threads."""
    return 1 if ((P2_BLOCK // 4 - 1) // O + 2) * 3 * max_link <= P2_BLOCK else 2


def inputs_of(name, s):
    O, _, seeds, _ = CASES[name]
    ps = [gen._variants(seed, O)[s] for seed in seeds]
    inputs = {key: np.stack([p[key] for p in ps]) for key in gen.INPUT_KEYS}
    from armour_amd.worlds import random_k
    B = len(seeds)
    ks = np.stack([random_k(seeds[0], B), np.ones((B, N)), -np.ones((B, N))]) if s == "a" else np.zeros((1, B, N))
    return inputs, ks


@pytest.fixture(scope="module")
def handles():
    """(EX handle, reference handle with ARMOUR_OPT_P2_EX = 0, evaluation points) per (case, problem set), shared by the tests."""
    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP
    made = {}

    def get(name, s):
        if (name, s) not in made:
            inputs, ks = inputs_of(name, s)
            pair = []
            for ex in (1, 0):
                nlp = ArmourNLP(T=CASES[name][1])
                nlp.set_option(_lib.OPT_P2_EX, ex)
                pair.append(nlp.set_parameters(inputs["q0"], inputs["qd0"], inputs["qdd0"], inputs["q_des"], inputs["obstacles"]))
            made[(name, s)] = (pair[0], pair[1], ks)
        return made[(name, s)]

    yield get
    for ex, ref, _ in made.values():
        ex.close(); ref.close()


@pytest.fixture(scope="module")
def reference_rows(handles):
    """g, jac of the six-slot kernels per (case, problem set, entry): computed once."""
    rows = {}

    def get(name, s, entry):
        if (name, s, entry) not in rows:
            _, ref, ks = handles(name, s)
            rows[(name, s, entry)] = gen.role.evaluate(ref, ks, entry)
        return rows[(name, s, entry)]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_the_cases_are_ex_launches_and_the_references_are_not(handles, name):
    O, T, seeds, dfc = CASES[name]
    for s in gen.SETS:
        ex, ref, _ = handles(name, s)
        v, f = gen.plan_verdict(ex)
        assert v["exact"] == 1 and v["six"] == 1 and v["shared"] == 1 and v["by_value"] == 1 and v["dfc"] == int(dfc), (name, s, v)
        assert f[0] > 0 and f[4] > 0 and f[5] > 0
        w, _ = gen.plan_verdict(ref)
        assert w["exact"] == 0 and w["six"] == 1 and w["dfc"] == int(dfc), (name, s, w)
        assert ex.m == N * T + 7 * T * O + 4 * N and ex.B == len(seeds)


def live_second_round_tasks(nlp, O, T):
    """Slicing tasks with index >= P2_BLOCK that are live (monomial index below the record's count), over all collision blocks of problem 0:
    task = (pi * max_link + mo) * 3 + axis for record pi of the block, as load_pass_uncond numbers them."""
    ml = nlp.table_sizes()["max_link"]
    Q = 7 * T * O
    counts = [len(nlp.pz("link", lt // T, lt % T)[2]) for lt in range(7 * T)]
    live = 0
    for q0 in range(0, Q, P2_BLOCK // 4):
        lt_first, lt_last = q0 // O, (min(Q, q0 + P2_BLOCK // 4) - 1) // O
        for pi in range(lt_last - lt_first + 1):
            live += sum(1 for mo in range(counts[lt_first + pi]) for e in range(3) if (pi * ml + mo) * 3 + e >= P2_BLOCK)
    return live


@pytest.mark.gpu
def test_the_cases_cover_both_round_counts(handles):
    """The launch's rule gives one round for every T = 2 case and two for o8_t8, and o8_t8's blocks really have live tasks beyond thread 255."""
    seen = {}
    for name, (O, _, _, _) in CASES.items():
        for s in gen.SETS:
            seen[(name, s)] = expected_rounds(O, handles(name, s)[0].table_sizes()["max_link"])
    assert all(r == (2 if name == "o8_t8" else 1) for (name, _), r in seen.items()), seen
    O, T, _, _ = CASES["o8_t8"]
    for s in gen.SETS:
        nlp = handles("o8_t8", s)[0]
        assert 8 * 3 * nlp.table_sizes()["max_link"] > P2_BLOCK   # eight records under every block at O = 8
        assert live_second_round_tasks(nlp, O, T) > 0, s
    O, T, _, _ = CASES["o8"]
    assert live_second_round_tasks(handles("o8", "a")[0], O, T) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(CASES))
def test_rows_are_the_six_slot_kernels_bits(handles, reference_rows, name, entry):
    for s in gen.SETS:
        ex, _, ks = handles(name, s)
        g, jac = gen.role.evaluate(ex, ks, entry)
        g_ref, jac_ref = reference_rows(name, s, entry)
        assert not np.isnan(g_ref).any() and not np.isnan(jac_ref).any(), (name, s)
        for what, got, ref in (("g", g, g_ref), ("jac", jac, jac_ref)):
            bad = np.argwhere(np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(ref).view(np.uint64))
            assert got.shape == ref.shape and len(bad) == 0, f"{name}/{s} {entry}: {len(bad)} entries of {what} differ, first at {bad[:4].tolist()}"
