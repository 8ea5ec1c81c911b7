#!/usr/bin/env python3
"""Recorded rows of the fused evaluation's three block roles (GPU box only).

    python3 tests/golden/make_p2_role_rows.py [OUT]      writes tests/golden/p2_role_rows.npz (or OUT)

For every case of CASES the file holds the planning problems (inputs, as data) and the full g [K,B,m] and jac [K,B,m,n] that
armour_eval_g_jac_device of the library in use produced for the K evaluation points of each problem set.  The generator also runs
the other entries tests/test_p2_role_rows.py checks (a prepared 3-step graph, the multi-point launch with two points -- the point
under test first, then second -- and the synchronous host call) and refuses to write a file if any of them differs from the recorded
rows in a single bit.  The committed file was recorded with the library of the commit before the limit block got one wave per path
family (select a library with ARMOUR_HIP_LIB).

The shapes are the smallest at which the kernel's paths differ: T = 8 gives Q = 56 collision rows at O = 1 (one partial 64-row
block) and 168 at O = 3 (two full blocks and a 40-row tail); B = 1 takes the by-value kernel arguments, B = 2 the pointer path.
Each case has two problem sets: `a`, a random state evaluated at a random k, at k = +1 and at k = -1 in every component, and `z`,
the same world started at rest (qd0 = qdd0 = 0) and evaluated at k = 0, where the stationary points of the limit rows are 0/0
and the select step must ignore them.

tests/test_p2_role_rows.py imports CASES, build_inputs' key names and evaluate() from here.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T = 8
OUT = os.path.join(HERE, "p2_role_rows.npz")
# name: (robot preset, mode, O, B, seed)
CASES = {
    "kinova_o1_b1": ("kinova", "armour", 1, 1, 900),
    "kinova_o3_b1": ("kinova", "armour", 3, 1, 910),
    "kinova_o3_b2": ("kinova", "armour", 3, 2, 920),
    "fetch_o1_b1": ("fetch", "armour", 1, 1, 930),
    "armtd_o3_b1": ("kinova", "armtd", 3, 1, 940),
}
SETS = ("a", "z")
ENTRIES = ("device", "steps", "multi", "multi_second", "host")
INPUT_KEYS = {"armour": ("q0", "qd0", "qdd0", "q_des", "obstacles"), "armtd": ("q0", "qd0", "q_des", "jrs", "k_range", "obstacles")}
N = 7   # factors of every preset used here


def declared_shapes(name):
    """{key: shape} of everything the fixture holds for one case."""
    robot, mode, O, B, _ = CASES[name]
    J = 7 if robot == "kinova" else 9
    m = (0 if mode == "armtd" else N * T) + J * T * O + 4 * N
    out = {}
    for s in SETS:
        K = 3 if s == "a" else 1
        pre = f"{name}__{s}__"
        for key in INPUT_KEYS[mode]:
            out[pre + key] = {"obstacles": (B, O, 12), "jrs": (B, N, 6, T)}.get(key, (B, N))
        out[pre + "k"] = (K, B, N)
        out[pre + "g"] = (K, B, m)
        out[pre + "jac"] = (K, B, m, N)
    return out


def build_inputs(name):
    """The two problem sets of a case and their evaluation points: {set: (inputs dict, ks [K,B,n])}."""
    from armour_amd.worlds import random_fetch_problem, random_k, random_problem, synthetic_offline_jrs
    robot, mode, O, B, seed = CASES[name]
    make = random_fetch_problem if robot == "fetch" else random_problem
    out = {}
    for s in SETS:
        ps = [make(seed + b, O) for b in range(B)]
        for p in ps:
            if s == "z":
                p["qd0"] = np.zeros(N); p["qdd0"] = np.zeros(N)
            if mode == "armtd":
                p["jrs"], p["k_range"] = synthetic_offline_jrs(p["qd0"], T)
        inputs = {key: np.stack([p[key] for p in ps]) for key in INPUT_KEYS[mode]}
        if s == "a":
            ks = np.stack([random_k(seed, B), np.ones((B, N)), -np.ones((B, N))])
        else:
            ks = np.zeros((1, B, N))
        out[s] = (inputs, ks)
    return out


def make_nlp(name, inputs):
    from armour_amd.planner import ArmourNLP, fetch_robot
    robot, mode = CASES[name][:2]
    nlp = ArmourNLP(robot=fetch_robot() if robot == "fetch" else None, T=T)
    if mode == "armtd":
        return nlp.set_parameters_armtd(inputs["q0"], inputs["qd0"], inputs["q_des"], inputs["jrs"], inputs["k_range"], inputs["obstacles"])
    return nlp.set_parameters(inputs["q0"], inputs["qd0"], inputs["qdd0"], inputs["q_des"], inputs["obstacles"])


def evaluate(nlp, ks, entry):
    """g [K,B,m] and jac [K,B,m,n] of the K points through one of the four entries.  Outputs start as NaN: a row nobody wrote shows."""
    import torch
    K, B, n = ks.shape
    m = nlp.m
    dev = torch.device("cuda:0")
    g = np.empty((K, B, m)); jac = np.empty((K, B, m, n))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    for i in range(K):
        if entry == "host":
            g[i], jac[i] = nlp.eval_g_jac(ks[i])
            continue
        if entry == "device":
            d_k = torch.from_numpy(np.ascontiguousarray(ks[i])).to(dev)
            d_g, d_j = nan(B, m), nan(B, m, n)
            torch.cuda.synchronize()
            nlp.eval_g_jac_device(d_k.data_ptr(), d_g.data_ptr(), d_j.data_ptr())
        elif entry == "steps":   # three chained launches into the same buffers: the last point's rows are what remains
            pts = np.stack([0.5 * ks[i], 0.1 - 0.25 * ks[i], ks[i]])
            d_k = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
            d_g, d_j = nan(B, m), nan(B, m, n)
            torch.cuda.synchronize()
            nlp.prepare_steps(d_k.data_ptr(), 3, d_g.data_ptr(), d_j.data_ptr())
            nlp.eval_g_jac_device_steps(d_k.data_ptr(), 3, d_g.data_ptr(), d_j.data_ptr())
        elif entry in ("multi", "multi_second"):   # two points in one launch; this one first (the k the kernel entry loads) or second
            at = 0 if entry == "multi" else 1
            other = ks[(i + 1) % K] if K > 1 else 0.3 - 0.5 * ks[i]
            pts = np.stack([ks[i], other] if at == 0 else [other, ks[i]])
            d_k = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
            d_g2, d_j2 = nan(2, B, m), nan(2, B, m, n)
            torch.cuda.synchronize()
            nlp.eval_g_jac_device_multi(d_k.data_ptr(), 2, d_g2.data_ptr(), d_j2.data_ptr())
            d_g, d_j = d_g2[at], d_j2[at]
        else:
            raise ValueError(entry)
        torch.cuda.synchronize()
        g[i], jac[i] = d_g.cpu().numpy(), d_j.cpu().numpy()
    return g, jac


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def main():
    data = {}
    for name in CASES:
        for s, (inputs, ks) in build_inputs(name).items():
            nlp = make_nlp(name, inputs)
            g, jac = evaluate(nlp, ks, "device")
            assert not np.isnan(g).any() and not np.isnan(jac).any(), (name, s)
            for entry in ENTRIES[1:]:
                g2, j2 = evaluate(nlp, ks, entry)
                assert same_bits(g, g2) and same_bits(jac, j2), f"{name}/{s}: entry {entry} differs from armour_eval_g_jac_device"
            pre = f"{name}__{s}__"
            for key, v in inputs.items():
                data[pre + key] = v
            data[pre + "k"], data[pre + "g"], data[pre + "jac"] = ks, g, jac
            nlp.close()
            print(f"{name}/{s}: m = {g.shape[-1]}, {ks.shape[0]} point(s)")
    for name in CASES:
        for key, shape in declared_shapes(name).items():
            assert data[key].shape == shape, (key, data[key].shape, shape)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(out, **data)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
