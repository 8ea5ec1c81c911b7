"""The build's zero-normal mask (plane_zero) and the fused evaluation's scan without the zero-normal test, on the device.

The scan of a collision block gives a plane whose normal is zero in a row the -1e8 sentinel there (the reference's A_elt.norm() > 0).  The
reach-set build reports, per problem, which planes have such a row (armour_debug_p2_zero_plan: the masks skip and zero); an exact-layout (EX)
launch none of whose live planes has one takes a kernel in which that test is the constant true (ARMOUR_OPT_P2_NO_ZERO_TEST, default 1).

1. The mask against a restatement from ArmourNLP.hyperplanes(): bit p <=> some row of the problem has A == 0 in all three components of plane
   p, compared on the live planes (bits of skipped planes carry no meaning).  Worlds: three different box worlds in one batch at O = 20, 17 and
   64, where no live plane is ever zero and the verdict is on (and 48 box worlds at T = 100, whose masks come back through
   armour_refresh_table_stats instead of the build's page-locked block); and a world in which ONE obstacle has the zero vector as its third generator --
   the planes pairing that generator are zero in that obstacle's rows only, live and zero somewhere: the premise is asserted, and the verdict
   is off.
2. Rows bit for bit (uint64 view of g and jac), option on against option off, through the entries of tests/golden/make_p2_role_rows.py
   (asynchronous device launch, prepared 3-step graph, two-point launch with either point, synchronous host call) at B = 1, 2 and 8 (d
   recomputed) and O = 20 and 17, T = 2, and at O = 8, T = 8 (seed 2026 of tests/test_p2_ex_staging.py: live slicing tasks beyond thread 255,
   the two-round kernels).  The "on" handle must report the new form, the "off" handle the old one.  In the flat-obstacle world both take the
   old form, agree in every bit, and agree with the CPU oracle to bench.py's tolerances (1e-9 on g, 1e-8 on jac).

Problems: Kinova, seeds counted up from a base until enough of them build at steps this long and take the EX kernel (as make_p2_ex_rows.py
does; searched once per module).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_p2_ex_rows as gen  # noqa: E402

N, J, NPLANES = 7, 7, 36
ALL = (1 << NPLANES) - 1
SEED_BASE = {20: 2203, 17: 3100, 64: 2308, 8: 2026}


def zero_plan(nlp):
    """armour_debug_p2_zero_plan of a handle: (test dropped, skip [B], zero [B])."""
    from armour_amd._lib import check
    v = C.c_int32(-1)
    skip, zero = np.zeros(nlp.B, dtype=np.uint64), np.zeros(nlp.B, dtype=np.uint64)
    u64 = C.POINTER(C.c_uint64)
    check(nlp.L.armour_debug_p2_zero_plan(nlp.h, C.byref(v), skip.ctypes.data_as(u64), zero.ctypes.data_as(u64)))
    return int(v.value), [int(x) for x in skip], [int(x) for x in zero]


def make(inputs, T, option=None):
    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP
    nlp = ArmourNLP(T=T)
    if option is not None:
        nlp.set_option(_lib.OPT_P2_NO_ZERO_TEST, option)
    return nlp.set_parameters(inputs["q0"], inputs["qd0"], inputs["qdd0"], inputs["q_des"], inputs["obstacles"])


def builds(p, T):
    from armour_amd._lib import ArmourError
    try:
        nlp = make({key: p[key][None] for key in gen.INPUT_KEYS}, T)
    except ArmourError:
        return False
    ok = gen.plan_verdict(nlp)[0]["exact"] == 1
    nlp.close()
    return ok


@pytest.fixture(scope="module")
def problems():
    """(O, T, B) -> {set: (inputs, ks)}: the first B seeds from the shape's base whose two variants build and take the EX kernel."""
    from armour_amd.worlds import random_k
    found, sets = {}, {}

    def seeds(O, T, B):
        have = found.setdefault((O, T), [])
        cand = have[-1][0] + 1 if have else SEED_BASE[O]
        while len(have) < B:
            assert cand < SEED_BASE[O] + 400, f"O = {O}: no seed builds"
            v = gen._variants(cand, O)
            if all(builds(v[s], T) for s in gen.SETS):
                have.append((cand, v))
            cand += 1
        return have[:B]

    def get(O, T, B):
        if (O, T, B) not in sets:
            chosen = seeds(O, T, B)
            out = {}
            for s in gen.SETS:
                inputs = {key: np.stack([v[s][key] for _, v in chosen]) for key in gen.INPUT_KEYS}
                ks = np.stack([random_k(chosen[0][0], B), np.ones((B, N)), -np.ones((B, N))]) if s == "a" else np.zeros((1, B, N))
                out[s] = (inputs, ks)
            sets[(O, T, B)] = out
        return sets[(O, T, B)]

    return get


def flat_world(problems, O=20):
    """A box world whose obstacle 1 has lost its third generator (Z = [c g1 g2 g3], 12 doubles: the last three)."""
    inputs, ks = problems(O, 2, 1)["a"]
    inputs = {key: val.copy() for key, val in inputs.items()}
    assert np.all(np.abs(inputs["obstacles"][0, :, 3:].reshape(O, 3, 3)).sum(axis=2) > 0)   # every generator of every box is non-zero
    inputs["obstacles"][0, 1, 9:12] = 0.0
    return inputs, ks


def restated_zero(nlp):
    """[B] masks from the full half-space table: bit p set when some row of the problem has a normal of plane p with three components == 0."""
    A, _, _ = nlp.hyperplanes()                                   # [B, T, J, O, 36, 3]
    z = np.all(A == 0.0, axis=-1).any(axis=(1, 2, 3))             # [B, 36]
    return [sum(1 << p for p in range(NPLANES) if z[b, p]) for b in range(nlp.B)]


@pytest.mark.gpu
@pytest.mark.parametrize("O", [20, 17, 64])
def test_mask_of_box_worlds_is_the_restatement(problems, O):
    for s in gen.SETS:
        inputs, _ = problems(O, 2, 3)[s]
        assert len({inputs["obstacles"][b].tobytes() for b in range(3)}) == 3   # three different worlds
        nlp = make(inputs, 2)
        on, skip, zero = zero_plan(nlp)
        ref = restated_zero(nlp)
        assert skip == [int(x) for x in nlp.plane_skip()]
        for b in range(3):
            live = ~skip[b] & ALL
            assert (zero[b] ^ ref[b]) & live == 0, (O, s, b, hex(zero[b]), hex(ref[b]), hex(live))
            assert ref[b] & live == 0, (O, s, b, hex(ref[b] & live))   # a box world: no live plane is ever zero
        assert gen.plan_verdict(nlp)[0]["exact"] == 1 and on == 1, (O, s, on)
        nlp.close()


@pytest.mark.gpu
def test_mask_of_the_flat_obstacle_world_is_the_restatement(problems):
    inputs, _ = flat_world(problems)
    nlp = make(inputs, 2)
    on, skip, zero = zero_plan(nlp)
    ref = restated_zero(nlp)
    live = ~skip[0] & ALL
    assert (zero[0] ^ ref[0]) & live == 0, (hex(zero[0]), hex(ref[0]), hex(live))
    # the premise: a plane that is live and zero somewhere -- zero in rows of obstacle 1 and in no other row -- and the verdict is off
    assert ref[0] & live != 0 and zero[0] & live != 0 and on == 0, (hex(ref[0]), hex(zero[0]), hex(live), on)
    A, _, _ = nlp.hyperplanes()
    zrow = np.all(A[0] == 0.0, axis=-1)   # [T, J, O, 36]
    for p in range(NPLANES):
        if (ref[0] & live) >> p & 1:
            assert zrow[:, :, 1, p].all() and not np.delete(zrow[..., p], 1, axis=2).any(), p
    nlp.close()


@pytest.mark.gpu
def test_mask_of_a_batch_beyond_the_builds_page_locked_read_back(problems):
    """48 problems at T = 100 keep more than the 4 MiB the build reads back in one block (link generators: B * T * 7 * 18 doubles): the masks then
    come through armour_refresh_table_stats."""
    from armour_amd.worlds import random_problem
    B, T, O = 48, 100, 8
    assert B * T * J * 18 * 8 > (4 << 20)
    ps = [random_problem(4000 + b, O) for b in range(B)]
    inputs = {key: np.stack([p[key] for p in ps]) for key in gen.INPUT_KEYS}
    nlp = make(inputs, T)
    on, skip, zero = zero_plan(nlp)
    ref = restated_zero(nlp)
    assert skip == [int(x) for x in nlp.plane_skip()]
    for b in range(B):
        live = ~skip[b] & ALL
        assert (zero[b] ^ ref[b]) & live == 0 and ref[b] & live == 0, (b, hex(zero[b]), hex(ref[b]), hex(live))
    assert on == gen.plan_verdict(nlp)[0]["exact"]   # (whatever the plan makes of T = 100: the test drops exactly where the launch is an EX one)
    nlp.close()


def same_bits(got, ref):
    return np.argwhere(np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(ref).view(np.uint64))


ROW_CASES = [(20, 2, 1), (17, 2, 1), (20, 2, 2), (17, 2, 2), (20, 2, 8), (17, 2, 8), (8, 8, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("O,T,B", ROW_CASES)
def test_rows_are_the_same_bits_with_and_without_the_test(problems, O, T, B):
    for s in gen.SETS:
        inputs, ks = problems(O, T, B)[s]
        new, old = make(inputs, T, 1), make(inputs, T, 0)
        v = gen.plan_verdict(new)[0]
        assert v["exact"] == 1 and v["dfc"] == int(B >= 8), (O, T, B, s, v)
        assert zero_plan(new)[0] == 1 and zero_plan(old)[0] == 0, (O, T, B, s)
        for entry in gen.ENTRIES:
            g, jac = gen.role.evaluate(new, ks, entry)
            g_ref, jac_ref = gen.role.evaluate(old, ks, entry)
            assert not np.isnan(g_ref).any() and not np.isnan(jac_ref).any(), (O, T, B, s, entry)
            for what, got, ref in (("g", g, g_ref), ("jac", jac, jac_ref)):
                bad = same_bits(got, ref)
                assert got.shape == ref.shape and len(bad) == 0, f"O={O} T={T} B={B}/{s} {entry}: {len(bad)} entries of {what} differ, first at {bad[:4].tolist()}"
        new.close(); old.close()


@pytest.mark.gpu
def test_flat_obstacle_world_keeps_the_test_and_agrees_with_the_oracle(problems):
    from oracle.cpu_oracle import Oracle
    inputs, ks = flat_world(problems)
    new, old = make(inputs, 2, 1), make(inputs, 2, 0)
    assert zero_plan(new)[0] == 0 and zero_plan(old)[0] == 0
    o = Oracle(T=2).set_problem(inputs["q0"][0], inputs["qd0"][0], inputs["qdd0"][0], inputs["q_des"][0], inputs["obstacles"][0])
    for entry in gen.ENTRIES:
        g, jac = gen.role.evaluate(new, ks, entry)
        g_old, jac_old = gen.role.evaluate(old, ks, entry)
        assert len(same_bits(g, g_old)) == 0 and len(same_bits(jac, jac_old)) == 0, entry
        if entry == "device":
            for i in range(ks.shape[0]):
                g_ref, jac_ref = o.eval_g_jac(ks[i, 0])
                dg, dj = float(np.abs(g[i, 0] - g_ref).max()), float(np.abs(jac[i, 0] - jac_ref).max())
                print(f"flat-obstacle world, point {i}: |dg| = {dg:.3e}, |djac| = {dj:.3e}")
                assert dg <= 1e-9 and dj <= 1e-8, (i, dg, dj)
    new.close(); old.close()
