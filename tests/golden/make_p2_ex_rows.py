#!/usr/bin/env python3
"""Recorded rows of the fused evaluation's exact-layout (EX) kernels (GPU box only).

    python3 tests/golden/make_p2_ex_rows.py [OUT]      writes tests/golden/p2_ex_rows.npz (or OUT)

tests/golden/p2_role_rows.npz records O = 1 and O = 3, where a collision block touches more (link, time step) pairs than one slicing
pass holds, so none of its cases runs the EX kernels -- the ones a launch with axis-aligned box obstacles and O >= 7 or so takes, the
headline launch among them.  This file records those, in the same form: for every case of CASES the planning problems (inputs, as
data) and the full g [K,B,m] and jac [K,B,m,n] of armour_eval_g_jac_device of the library in use; the other entries
tests/test_p2_ex_rows.py checks (a prepared 3-step graph, the two-point launch with either point, the synchronous host call) must
agree with those rows in every bit or nothing is written.  Nothing is written either for a case whose one-point launch is not an EX
launch (armour_debug_p2_plan), or whose d column is not handled as the case says.

The committed file was recorded with a library whose kernels are those of the commit before the EX kernels took their plane-table
addressing from the launch plan (select a library with ARMOUR_HIP_LIB; it needs armour_debug_p2_plan).

Shapes: Kinova, box obstacles.  O = 20 and O = 17 put five (link, time step) pairs under a 64-row block, O = 17 with the pair
boundaries off the block boundaries; O = 64 one pair per block; B = 2 is the pointer path with the shared-mask check; B = 8 has no d
column (d is recomputed from the obstacle centres).  T = 2 keeps several full blocks and, where O allows it, a partial last block,
and the file below 1 MB: Q = 280 at O = 20 (four blocks and a 24-row tail), 238 at O = 17 (three and a 46-row tail), 896 at O = 64
(fourteen blocks).  With steps that long a random state's reach sets can outgrow the build's monomial capacity: a problem is taken
from the first seed, counting up from the case's, whose two variants build (the inputs are stored, so the test does not search).
The evaluation points are those of make_p2_role_rows.py: set `a` at a random k, at +1 and at -1, set `z` started at rest and
evaluated at k = 0.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_p2_role_rows as role  # noqa: E402   (evaluate, same_bits: the entries and the comparison are the same)

OUT = os.path.join(HERE, "p2_ex_rows.npz")
# name: (O, B, T, seed, d recomputed)
CASES = {
    "o20_b1": (20, 1, 2, 1000, False),
    "o17_b1": (17, 1, 2, 1010, False),
    "o64_b1": (64, 1, 2, 1020, False),
    "o20_b2": (20, 2, 2, 1030, False),
    "o20_b8": (20, 8, 2, 1040, True),
}
SETS = role.SETS
ENTRIES = role.ENTRIES
INPUT_KEYS = role.INPUT_KEYS["armour"]
N, J = 7, 7


def declared_shapes(name):
    O, B, T, _, _ = CASES[name]
    m = N * T + J * T * O + 4 * N
    out = {}
    for s in SETS:
        K = 3 if s == "a" else 1
        pre = f"{name}__{s}__"
        for key in INPUT_KEYS:
            out[pre + key] = (B, O, 12) if key == "obstacles" else (B, N)
        out[pre + "k"] = (K, B, N)
        out[pre + "g"] = (K, B, m)
        out[pre + "jac"] = (K, B, m, N)
    return out


def _variants(seed, O):
    """The problem of a seed as set `a` has it and as set `z` has it (started at rest)."""
    from armour_amd.worlds import random_problem
    a, z = random_problem(seed, O), random_problem(seed, O)
    z["qd0"] = np.zeros(N); z["qdd0"] = np.zeros(N)
    return {"a": a, "z": z}


def _builds(name, p):
    from armour_amd._lib import ArmourError
    try:
        nlp = make_nlp(name, {key: p[key][None] for key in INPUT_KEYS})
        ok = plan_verdict(nlp)[0]["exact"] == 1   # (few enough monomials per link PZ for one slicing pass)
        nlp.close()
        return ok
    except ArmourError:
        return False


def build_inputs(name):
    """The two problem sets of a case and their evaluation points: {set: (inputs dict, ks [K,B,n])}."""
    from armour_amd.worlds import random_k
    O, B, _, seed, _ = CASES[name]
    chosen, cand = [], seed
    while len(chosen) < B:
        assert cand < seed + 400, f"{name}: no seed builds"
        v = _variants(cand, O)
        if all(_builds(name, v[s]) for s in SETS):
            chosen.append(v)
        cand += 1
    out = {}
    for s in SETS:
        inputs = {key: np.stack([v[s][key] for v in chosen]) for key in INPUT_KEYS}
        ks = np.stack([random_k(seed, B), np.ones((B, N)), -np.ones((B, N))]) if s == "a" else np.zeros((1, B, N))
        out[s] = (inputs, ks)
    return out


def make_nlp(name, inputs):
    from armour_amd.planner import ArmourNLP
    nlp = ArmourNLP(T=CASES[name][2])
    return nlp.set_parameters(inputs["q0"], inputs["qd0"], inputs["qdd0"], inputs["q_des"], inputs["obstacles"])


def plan_verdict(nlp):
    """armour_debug_p2_plan of the handle: dict(dfc, six, exact, arg_bytes, shared, by_value) and the 20 addressing fields."""
    import ctypes as C
    if not hasattr(nlp.L, "armour_debug_p2_plan"):
        raise RuntimeError("the library in use does not export armour_debug_p2_plan")
    from armour_amd._lib import check
    v = np.zeros(6, dtype=np.int32); f = np.zeros(20, dtype=np.uint32)
    check(nlp.L.armour_debug_p2_plan(nlp.h, v.ctypes.data_as(C.POINTER(C.c_int32)), f.ctypes.data_as(C.POINTER(C.c_uint32))))
    return dict(zip(("dfc", "six", "exact", "arg_bytes", "shared", "by_value"), (int(x) for x in v))), f


def main():
    data = {}
    for name, (O, B, T, _, dfc) in CASES.items():
        for s, (inputs, ks) in build_inputs(name).items():
            nlp = make_nlp(name, inputs)
            v, _ = plan_verdict(nlp)
            assert v["exact"] == 1 and v["shared"] == 1, f"{name}/{s}: not an EX launch with one mask ({v}; max_link {nlp.table_sizes()['max_link']}): take the next larger O"
            assert v["dfc"] == int(dfc), f"{name}/{s}: d recomputed = {v['dfc']}"
            g, jac = role.evaluate(nlp, ks, "device")
            assert not np.isnan(g).any() and not np.isnan(jac).any(), (name, s)
            for entry in ENTRIES[1:]:
                g2, j2 = role.evaluate(nlp, ks, entry)
                assert role.same_bits(g, g2) and role.same_bits(jac, j2), f"{name}/{s}: entry {entry} differs from armour_eval_g_jac_device"
            pre = f"{name}__{s}__"
            for key, val in inputs.items():
                data[pre + key] = val
            data[pre + "k"], data[pre + "g"], data[pre + "jac"] = ks, g, jac
            nlp.close()
            print(f"{name}/{s}: m = {g.shape[-1]}, {ks.shape[0]} point(s), plan {v}")
    for name in CASES:
        for key, shape in declared_shapes(name).items():
            assert data[key].shape == shape, (key, data[key].shape, shape)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(out, **data)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()
