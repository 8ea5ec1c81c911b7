"""Row masks and row lists of relevance.hip against an exact restatement of the rule (tests/relevance_rule.py; include/armour_hip.h states it).

tests/test_row_relevance.py checks the masks in one direction, by sampling: no dropped row was violated at the sampled k.  Here both masks are
compared with the rule itself, row by row -- on tables built by program so that every row's fate is fixed by construction (a designated plane whose
d puts the row 1e-6 above or below a threshold, every other plane failing by 10 or carrying a zero normal), and on the device's own tables of two
built inputs -- and the lists (ascending rows, rows by residue class, the solver's torque rows, the packed plane entries) are read back through
armour_debug_get_row_lists and compared entry by entry.

The hand-built set: ArmourNLP(T = 40), B = 8, O = 2: Q = 560 collision rows, row0 = 280, m = 868 -- three 256-row passes of the list kernel, the last
partial, the residue classes offset by 24 from the collision index.  The relevance lists hold 0, 1, 63, 64, 65, 255, 256, 257 rows.  The solver's
mask contains the relevance mask, so its lists cannot take the same sizes in another order; they hold 0, 1, 64, 65, 255, 256, 257 and all 560 rows,
and the missing size 63 is among the solver's TORQUE lists, which hold 257, 256, 255, 65, 64, 63, 1, 0 rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

import relevance_rule as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
T = 40
EPS = 1e-6
REL_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257]
SOL_COUNTS = [0, 1, 64, 65, 255, 256, 257, 560]
TQ_SOL_COUNTS = [257, 256, 255, 65, 64, 63, 1, 0]
CLASSES = ["hull", "oblique", "p0", "p35", "ll", "zero", "empty", "full", "f7", "norm3"]
SPECIAL_B = 4                                   # the problem with room for the rows whose fate only a degree / a plane's norm decides
SPECIAL = {10: "deg1", 11: "deg3", 12: "norm3"}  # its (l, t) slots: twins with equal coefficients and degrees 1 | 3; a norm-3 row between need2(1) and need2(3)


# --------------------------------------------------------------------------------------------------------------- tables -> the rule's arguments
def rule_args(t, b, gl, gu, live=None, unit_normals=False):
    """problem b of tables in the layout of armour_debug_load_tables (tests/helpers.py oracle_tables) as relevance_rule.row_rule takes them"""
    J, Tn = t["link_count"].shape[1:3]
    n = t["torque_count"].shape[1]
    O = t["A"].shape[3]
    Q = J * Tn * O
    return dict(link_cen=t["link_center"][b, :, :, 0, :].reshape(J * Tn, 3), link_keys=t["link_keys"][b].reshape(J * Tn, -1),
                link_coef=t["link_coeffs"][b].reshape(J * Tn, -1, 3), link_cnt=t["link_count"][b].reshape(J * Tn),
                A=t["A"][b].transpose(1, 0, 2, 3, 4).reshape(Q, 36, 3), d=t["d"][b].transpose(1, 0, 2, 3).reshape(Q, 36),
                delta=t["delta"][b].transpose(1, 0, 2, 3).reshape(Q, 36), live=np.ones(36, bool) if live is None else live,
                tq_cen=t["torque_center"][b, :, :, 0].T.reshape(n * Tn), tq_keys=t["torque_keys"][b].transpose(1, 0, 2).reshape(n * Tn, -1),
                tq_coef=t["torque_coeffs"][b].transpose(1, 0, 2).reshape(n * Tn, -1), tq_cnt=t["torque_count"][b].T.reshape(n * Tn),
                gl=gl, gu=gu, O=O, unit_normals=unit_normals)


def closest(res, key, rows):
    d = np.abs(res["dist_" + key][rows])
    return float(d.min()) if d.size else np.inf


# --------------------------------------------------------------------------------------------------------------- the rule on the CPU
_ORACLE = {}


def oracle_77():
    """the oracle's tables of random_problem(77, 12) at T = 40, its bounds and the rule's verdicts (built once)"""
    if not _ORACLE:
        from armour_amd.worlds import random_problem
        from helpers import oracle_tables
        from oracle.cpu_oracle import Oracle
        p = random_problem(77, 12)
        o = Oracle(T=T).set_problem(p["q0"], p["qd0"], p["qdd0"], p["q_des"], p["obstacles"])
        _, _, gl, gu = o.bounds()
        res = rr.row_rule(**rule_args(oracle_tables([o]), 0, gl, gu, unit_normals=True))
        _ORACLE.update(o=o, gl=gl, gu=gu, res=res)
    return _ORACLE


def test_the_restatement_is_sound_against_the_oracle():
    """At 200 k (uniform draws and points near the corners, as tests/test_row_relevance.py draws them) no row the restatement drops is violated in the
    oracle's evaluation, and no row it drops from the solver's mask passes g +- 2 |J|_1 against its bound.  The counts are those of the issue that
    introduced this file: 86 relevant and 219 solver collision rows, 19 relevant torque rows, no undecided row, the closest collision row 5.5e-4 away."""
    from armour_amd.worlds import random_k
    c = oracle_77()
    o, gl, gu, res = c["o"], c["gl"], c["gu"], c["res"]
    n, nT = o.n, o.n * T
    Q = o.J * T * o.O
    assert not res["undecided_rel"].any() and not res["undecided_solver"].any()
    near = closest(res, "rel", slice(nT, nT + Q))
    counts = (int(res["rel"][nT:nT + Q].sum()), int(res["solver"][nT:nT + Q].sum()), int(res["rel"][:nT].sum()))
    print(f"random_problem(77, 12): relevant / solver collision rows, relevant torque rows {counts}; closest collision row {near:.2e}")
    assert counts == (86, 219, 19) and 5.0e-4 < near < 6.0e-4
    rng = np.random.default_rng(5)
    ks = random_k(0, 200)
    ks[::8] = np.sign(ks[::8]) * (1.0 - 0.05 * rng.random((25, n)))
    violated, candidate = np.zeros(o.m, bool), np.zeros(o.m, bool)
    for k in ks:
        g, jac = o.eval_g_jac(k)
        l1 = np.abs(jac).sum(1)
        violated |= (g > gu) | (g < gl)
        candidate |= ((gu < 1e18) & (g + 2.0 * l1 > gu)) | ((gl > -1e18) & (g - 2.0 * l1 < gl))
    assert not (violated & ~res["rel"]).any(), np.argwhere(violated & ~res["rel"])[:5]
    assert not (candidate & ~res["solver"]).any(), np.argwhere(candidate & ~res["solver"])[:5]
    assert not (res["rel"] & ~res["solver"]).any() and res["rel"][nT + Q:].all()


def test_the_restatement_is_tight_where_brute_force_is_exact():
    """PZs of <= 3 monomials of degree 1 in distinct factors: x(k) is linear in each k_j, so over the 2^n corners brute force gives the extremes of
    A . x(k) exactly, and with them the largest L for which one side of the plane holds at every k.  d is placed so that this L lies 1e-7 either side
    of 1e-9 (the relevance threshold) and of need2 (the solver's, whose |rd| is sum |coef| per axis at degree 1): the verdicts flip exactly there."""
    rng = np.random.default_rng(11)
    n, cases = 7, 24
    corners = np.array([[1.0 if (i >> j) & 1 else -1.0 for j in range(n)] for i in range(1 << n)])
    cen = rng.uniform(-0.5, 0.5, (cases, 3))
    cnt = rng.integers(0, 4, cases)
    keys, coef = np.zeros((cases, 3), np.uint64), np.zeros((cases, 3, 3))
    A, d, delta = np.zeros((cases, 36, 3)), np.zeros((cases, 36)), np.zeros((cases, 36))
    want_rel, want_sol = np.zeros(cases, bool), np.zeros(cases, bool)
    for i in range(cases):
        fac = rng.permutation(n)[:cnt[i]]
        keys[i, :cnt[i]] = [1 << (2 * int(f)) for f in fac]
        coef[i, :cnt[i]] = rng.uniform(-0.2, 0.2, (cnt[i], 3))
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        A[i, 7], delta[i, 7] = a, rng.uniform(0.01, 0.1)
        d[i, 3] = 1e6                                   # a zero-normal plane that must not count
        x = LD(cen[i]) + sum(LD(corners[:, int(f)])[:, None] * LD(coef[i, j]) for j, f in enumerate(fac)) if cnt[i] else LD(cen[i])[None]
        ax = (x * LD(a)).sum(1)
        rdn = np.sqrt((np.abs(LD(coef[i, :cnt[i]])).sum(0) ** 2).sum())
        need2 = rr.REL_MARGIN + 2 * rdn * (1 + rr.BOX_SLACK)
        h = (ax.max() - ax.min()) / 2
        which, side = i % 4, 1 if (i // 4) % 2 else -1    # threshold: relevance - | + , solver - | +
        L = (rr.REL_MARGIN if which < 2 else need2 + rr.BOX_SLACK * h) + (1e-7 if which % 2 else -1e-7)
        d[i, 7] = float(ax.max() + L + delta[i, 7]) if side > 0 else float(ax.min() - L - delta[i, 7])
        brute = max((ax - d[i, 7]).min(), (d[i, 7] - ax).min()) - LD(delta[i, 7])     # one of the plane's two values is >= brute at every corner
        want_rel[i] = not brute >= rr.REL_MARGIN
        want_sol[i] = not (brute >= rr.REL_MARGIN and brute - rr.BOX_SLACK * h >= need2)
        assert abs(brute - L) < 1e-12 and (cnt[i] > 0 or which < 2 or want_rel[i] == want_sol[i])
    col = rr.collision_rule(cen, keys, coef, cnt, A, d, delta, np.ones(36, bool), np.full(cases, -1e19), np.zeros(cases), 1, True)
    assert np.array_equal(col["rel"], want_rel) and np.array_equal(col["solver"], want_sol)
    assert want_rel.any() and not want_rel.all() and (want_sol & ~want_rel).any() and not want_sol.all()
    assert not col["undecided_rel"].any() and not col["undecided_solver"].any()


def test_the_restatement_counts_degrees_in_every_factor():
    """A key with degree 3 in the seventh factor (bits 12-13), in the eighth (bits 14-15), and one of total degree 21; and the verdict they decide: one
    monomial 0.1 e_x behind the plane x = d, |rd| = deg * 0.1, so need2 = 1e-9 + 0.2 deg (1 + 3e-5) and the row leaves the solver's mask at
    L - 3e-6 >= need2."""
    keys = np.array([3 << 12, 3 << 14, 0x3FFF, 1, 0], dtype=np.uint64)
    assert rr.key_degrees(keys).tolist() == [3, 3, 21, 1, 0]
    for key, deg in ((3 << 12, 3), (0x3FFF, 21), (3 << 14, 3)):
        for sign in (-1, 1):
            A, d, delta = np.zeros((1, 36, 3)), np.zeros((1, 36)), np.zeros((1, 36))
            A[0, 0] = [1, 0, 0]
            L = 1e-9 + 0.2 * deg * (1 + 3e-5) + 3e-6 + sign * 1e-7
            d[0, 0] = L + 0.1 * (1 + 1e-12)
            col = rr.collision_rule(np.zeros((1, 3)), np.array([[key]], np.uint64), np.array([[[0.1, 0, 0]]]), np.array([1]), A, d, delta,
                                    np.ones(36, bool), np.array([-1e19]), np.zeros(1), 1, True)
            assert not col["rel"][0] and col["solver"][0] == (sign < 0), (key, sign, col)
    tq = rr.torque_rule(np.array([0.0, 0.0]), np.array([[3 << 12], [3 << 12]], np.uint64), np.array([[0.1], [0.1]]), np.array([1, 1]),
                        np.array([-5.0, -5.0]), np.array([0.7 * (1 + 3e-5) - 1e-9 + 1e-7, 0.7 * (1 + 3e-5) - 1e-9 - 1e-7]))   # reach = (0.1 + 2 * 0.3)(1 + 3e-5)
    assert tq["rel"].tolist() == [False, False] and tq["solver"].tolist() == [False, True]


# --------------------------------------------------------------------------------------------------------------- the hand-built tables
def _keys(rng, M, nfac, must=()):
    out = set(int(k) for k in must)
    while len(out) < M:
        key = 0
        for f in rng.permutation(nfac)[:rng.integers(1, 4)]:
            key |= int(rng.integers(1, 4)) << (2 * int(f))
        out.add(key)
    return np.array(sorted(out), dtype=np.uint64)


def _perp(rng, a):
    w = np.cross(a, rng.normal(size=3))
    return w / np.linalg.norm(w)


_HAND = {}


def hand_built(shared, nfac=7):
    """The hand-built table set (module docstring): dict(tables, state, gl, gu, res [B] the rule's verdicts, cls [B][J*T], target [B][Q]).
    shared: the link x link normals (planes >= 21) are equal across the two obstacles (the loader then reads them from its compact record); else
    obstacle 1's are obstacle 0's with the components rotated, so they come from the full table.  nfac = 8: the eight-factor arm of
    tests/test_key128.py (J = 8), with a monomial of degree 3 in the eighth factor in the class "f7"."""
    if (shared, nfac) in _HAND:
        return _HAND[(shared, nfac)]
    from armour_amd.planner import kinova_robot
    B, O, J, n = 8, 2, nfac, nfac
    JT, Q, nT = J * T, J * T * O, n * T
    m = nT + Q + 4 * n
    capL, capT = 32, 128
    lim = np.full(n, 13.0)                                   # (13: the eighth joint of tests/test_key128.py make_eight_factor_arm)
    lim[:7] = list(kinova_robot().torque_limits)[:7]
    top = 3 << (2 * (nfac - 1))                              # degree 3 in the last factor
    t = dict(link_count=np.zeros((B, J, T), np.int32), link_center=np.zeros((B, J, T, 2, 3)), link_keys=np.zeros((B, J, T, capL), np.uint64),
             link_coeffs=np.zeros((B, J, T, capL, 3)), torque_count=np.zeros((B, n, T), np.int32), torque_center=np.zeros((B, n, T, 2)),
             torque_keys=np.zeros((B, n, T, capT), np.uint64), torque_coeffs=np.zeros((B, n, T, capT)), A=np.zeros((B, T, J, O, 36, 3)),
             d=np.zeros((B, T, J, O, 36)), delta=np.zeros((B, T, J, O, 36)), torque_radius=np.zeros((B, n, T)))
    gl, gu = np.zeros((B, m)), np.zeros((B, m))
    gl[:, nT:nT + Q] = -1e19
    cls_all, target_all = [], []
    corner = np.zeros((B, Q), bool)   # the collision rows violated at k = (1, .., 1), by construction
    for b in range(B):
        rng = np.random.default_rng(7000 + b)                # (the same draws in both table sets)
        R, S = REL_COUNTS[b], min(SOL_COUNTS[b], Q)
        cls = [SPECIAL[lt] if b == SPECIAL_B and lt in SPECIAL else CLASSES[(lt + 3 * b) % len(CLASSES)] for lt in range(JT)]
        if S == Q:   # every row listed: an empty PZ has |rd| = 0 and u = 0, its two thresholds coincide and no row of it can lie between them
            cls = ["oblique" if c == "empty" else c for c in cls]
        # ---- which rows are kept: R rows below the relevance threshold (A), S - R between the two (B, C; M: the special slots), the rest above both (D)
        forced = {q: ("D" if cls[q // O] == "deg1" else "M") for q in range(Q) if b == SPECIAL_B and (q // O) in SPECIAL}
        order = [int(q) for q in rng.permutation(Q) if q not in forced]
        target = np.full(Q, "D", dtype="U1")
        target[order[:R]] = "A"
        between = [q for q in order[R:] if cls[q // O] != "empty"][:S - R - sum(v == "M" for v in forced.values())]
        target[between[0::2]] = "B"
        target[between[1::2]] = "C"
        for q, v in forced.items():
            target[q] = v
        # ---- link PZs and their rows' planes
        for lt in range(JT):
            l, tt = lt // T, lt % T
            c = cls[lt]
            N = rng.normal(size=(36, 3))
            N /= np.linalg.norm(N, axis=1)[:, None]
            pstar = {"p0": 0, "p35": 35, "ll": 21 + lt % 15}.get(c, int(rng.integers(36)))
            if c in ("p0", "p35", "ll"):
                N[np.arange(36) != pstar] = 0.0
            if c == "zero":
                N[[p for p in (3, 20, 22, 30) if p != pstar]] = 0.0
            if c == "norm3":
                N *= 3.0
            a = N[pstar] / np.linalg.norm(N[pstar])
            M = {"empty": 0, "full": capL, "deg1": 3, "deg3": 3}.get(c, int(rng.integers(1, 12)))
            tm = rng.uniform(0.01, 0.05, M)
            co = np.array([tm[i] * (a if c == "hull" else a + 0.8 * _perp(rng, a)) for i in range(M)]).reshape(M, 3)
            must = {"f7": [top], "full": [0x3FFF], "deg1": [1, 4, 16], "deg3": [3, 12, 48]}.get(c, [])
            keys = _keys(rng, M, nfac, must)
            if c == "f7":
                co[list(keys).index(top)] *= 0.2 / tm[list(keys).index(top)]     # (large enough that its degree decides rows C and D)
            cen = rng.uniform(-0.5, 0.5, 3)
            if c == "deg3":   # the twin of the slot before: same centre, coefficients and planes, degrees 3 for 1
                cen, co, N, pstar = twin
            twin = (cen, co, N, pstar)
            t["link_count"][b, l, tt] = M
            t["link_center"][b, l, tt, 0] = cen
            t["link_keys"][b, l, tt, :M] = keys
            t["link_coeffs"][b, l, tt, :M] = co
            deg = rr.key_degrees(keys)
            rdn = lambda dg: np.sqrt(((LD(dg)[:, None] * np.abs(LD(co))).sum(0) ** 2).sum()) if M else LD(0)
            dl_star = rng.uniform(0.01, 0.1, O)
            sgn = rng.choice([-1.0, 1.0], O)
            for o in range(O):
                No = N.copy()
                if not shared and o == 1:
                    No[21:] = np.roll(N[21:], 1, axis=1)
                ac = (LD(No) * LD(cen)).sum(1)
                t["A"][b, tt, l, o] = No
                t["d"][b, tt, l, o] = ac.astype(np.float64)
                t["delta"][b, tt, l, o] = 10.0                                    # every other plane: L = -h - 10
                zero = ~(No != 0).any(1)
                t["d"][b, tt, l, o, zero] = 1e6 * (-1.0) ** np.arange(36)[zero]     # |0 - d| - delta = 1e6: must not count
                t["delta"][b, tt, l, o, zero] = 0.0
                ap = LD(No[pstar])
                h = np.abs((LD(co) * ap).sum(1)).sum() if M else LD(0)
                amax = max(LD(1), max(np.sqrt((LD(No[p]) ** 2).sum()) for p in range(36)) * rr.TIGHT)
                need2 = lambda dg, am: rr.REL_MARGIN + 2 * rdn(dg) * am * (1 + rr.BOX_SLACK)
                tg = target[lt * O + o]
                if tg == "M" and c == "norm3":
                    L = (need2(deg, LD(1)) + need2(deg, amax)) / 2 + rr.BOX_SLACK * h        # between need2(amax = 1) and need2(amax = 3): kept
                elif c in ("deg1", "deg3"):
                    L = (need2(np.ones(M), amax) + need2(3 * np.ones(M), amax)) / 2 + rr.BOX_SLACK * h   # only the degree decides: deg1 out, deg3 kept
                else:
                    L = {"A": rr.REL_MARGIN - EPS, "B": rr.REL_MARGIN + EPS, "C": need2(deg, amax) + rr.BOX_SLACK * h - EPS,
                         "D": need2(deg, amax) + rr.BOX_SLACK * h + EPS}[tg]
                t["d"][b, tt, l, o, pstar] = float(ac[pstar] + LD(sgn[o]) * (L + h * rr.TIGHT + LD(dl_star[o])))
                t["delta"][b, tt, l, o, pstar] = dl_star[o]
                # at k = (1, .., 1) every monomial is its coefficient; x is inside every other plane's slab (|A.(x - c)| < 7 < 10), so the row is
                # violated there iff x is inside the designated plane's too: the kept rows whose d lies on the side the coefficients point to
                val = np.abs((ap * (LD(cen) + LD(co).sum(0))).sum() - LD(t["d"][b, tt, l, o, pstar])) - LD(dl_star[o])
                assert abs(val) > 1e-7
                corner[b, lt * O + o] = val < 0
        # ---- torque PZs: TQ_SOL_COUNTS[b] rows in the solver's mask, half of them relevant; eps either side of every threshold
        order = rng.permutation(nT)
        St = TQ_SOL_COUNTS[b]
        kind = np.empty(nT, dtype="U3")
        kind[order[:St // 2]] = [("U+", "L+")[i % 2] for i in range(St // 2)]
        kind[order[St // 2:St]] = [("U-", "RU+", "L-", "RL+")[i % 4] for i in range(St - St // 2)]
        kind[order[St:]] = [("RU-", "RL-")[i % 2] for i in range(nT - St)]
        for r in range(nT):
            tt, j = r // n, r % n
            M = 100 if r == 5 else int(rng.integers(1, 20))   # (100: the fused evaluation's LDS holds 8 torque rows of at most ~120 monomials)
            keys = _keys(rng, M, nfac, [top] if r % 9 == 0 else [])
            upper = "U" in kind[r]
            co = rng.uniform(0.01, 0.05, M) * (1.0 if upper else -1.0) * (0.1 if M == 100 else 1.0)   # (the reach stays far from the other bound)
            deg = rr.key_degrees(keys)
            rad, radd = np.abs(LD(co)).sum(), (LD(deg) * np.abs(LD(co))).sum()
            reach = (rad + 2 * radd) * (1 + rr.BOX_SLACK)
            tr = rng.uniform(0.5, 1.5)
            lo, hi = -lim[j] + tr, lim[j] - tr                                   # (row_rules.h row_bounds)
            e = LD(EPS) if kind[r].endswith("+") else -LD(EPS)
            r_used = reach if kind[r].startswith("R") else rad
            cen = (LD(hi) - rr.REL_MARGIN + e - r_used) if upper else (LD(lo) + rr.REL_MARGIN - e + r_used)
            t["torque_count"][b, j, tt] = M
            t["torque_center"][b, j, tt, 0] = float(cen)
            t["torque_keys"][b, j, tt, :M] = keys
            t["torque_coeffs"][b, j, tt, :M] = co
            t["torque_radius"][b, j, tt] = tr
            gl[b, r], gu[b, r] = lo, hi
        cls_all.append(cls); target_all.append(target)
    state = dict(q0=np.zeros((B, n)), qd0=np.zeros((B, n)), qdd0=np.zeros((B, n)), q_des=np.full((B, n), 0.3))
    res = [rr.row_rule(**rule_args(t, b, gl[b], gu[b])) for b in range(B)]
    _HAND[(shared, nfac)] = dict(tables=t, state=state, gl=gl, gu=gu, res=res, cls=cls_all, target=target_all, corner=corner, B=B, O=O, J=J, n=n, Q=Q, nT=nT, m=m)
    return _HAND[(shared, nfac)]


def check_hand_built(hb):
    """what the fixture promises, through the restatement alone: no row undecided, the closest at least 1e-7 from its threshold, the lists' sizes,
    every row's fate the one it was built for, every class on both sides of both thresholds"""
    O, Q, nT = hb["O"], hb["Q"], hb["nT"]
    seen = set()
    for b, res in enumerate(hb["res"]):
        assert not res["undecided_rel"].any() and not res["undecided_solver"].any()
        rows = slice(0, nT + Q)
        assert min(closest(res, "rel", rows), closest(res, "solver", rows)) >= 1e-7, (b, closest(res, "rel", rows), closest(res, "solver", rows))
        rel, sol = res["rel"][nT:nT + Q], res["solver"][nT:nT + Q]
        tg = hb["target"][b]
        assert np.array_equal(rel, tg == "A") and np.array_equal(sol, np.isin(tg, ["A", "B", "C", "M"]))
        assert (int(rel.sum()), int(sol.sum()), int(res["solver"][:nT].sum())) == (REL_COUNTS[b], min(SOL_COUNTS[b], Q), TQ_SOL_COUNTS[b])
        assert int(res["rel"][:nT].sum()) == TQ_SOL_COUNTS[b] // 2 and res["rel"][nT + Q:].all() and res["solver"][nT + Q:].all()
        seen |= {(hb["cls"][b][q // O], tg[q]) for q in range(Q)}
    for c in CLASSES:
        need = "AD" if c == "empty" else "ABCD"
        assert all((c, s) in seen for s in need), (c, sorted(seen))
    assert {("deg1", "D"), ("deg3", "M"), ("norm3", "M")} <= seen


@pytest.mark.parametrize("shared", [True, False])
def test_hand_built_tables_fix_every_row(shared):
    hb = hand_built(shared)
    check_hand_built(hb)
    A = hb["tables"]["A"]
    assert np.array_equal(A[:, :, :, 0, 21:], A[:, :, :, 1, 21:]) == shared
    # rows only the tight sum separates (hull L < 1e-9 on every plane, tight L = 1e-9 + eps) are there in numbers among the oblique rows just above
    # the relevance threshold; the rows of class "hull" (coefficients along the normal) are separated by the hull pass already
    only_tight = 0
    for b in (4, 7):
        args = rule_args(hb["tables"], b, hb["gl"][b], hb["gu"][b])
        lt = np.arange(hb["Q"]) // hb["O"]
        r = np.abs(LD(args["link_coef"])).sum(1)[lt]
        c = LD(args["link_cen"])[lt]
        hull_sep = np.zeros(hb["Q"], bool)
        for p in range(36):
            a = LD(args["A"][:, p])
            L = np.abs((a * c).sum(1) - LD(args["d"][:, p])) - (np.abs(a) * r).sum(1) * rr.TIGHT - LD(args["delta"][:, p])
            hull_sep |= (a != 0).any(1) & (L >= rr.REL_MARGIN)
        obl = np.array([hb["cls"][b][q // hb["O"]] == "oblique" for q in range(hb["Q"])]) & (hb["target"][b] == "B")
        hul = np.array([hb["cls"][b][q // hb["O"]] == "hull" for q in range(hb["Q"])]) & (hb["target"][b] == "B") & (np.arange(hb["Q"]) % 2 == 0)
        only_tight += int((~hull_sep[obl]).sum())
        assert hul.any() and hull_sep[hul].all()
    assert only_tight >= 10, only_tight


# --------------------------------------------------------------------------------------------------------------- g off the same tables, in numpy
def numpy_g(t, b, k, nfac):
    """g of the torque and collision rows of problem b at k in fp64, in the evaluation's order: the slice sums centre + monomials in table order,
    a monomial is its coefficient times the factors' powers in factor order; planes ascending, zero normals skipped."""
    a = rule_args(t, b, None, None)
    pw = np.stack([np.ones_like(k), k, k * k, k * k * k], 1)   # [n][4]

    def slice_(cen, keys, coef, cnt):
        acc = np.array(cen, dtype=np.float64)
        for i in range(keys.shape[1]):
            v = np.array(coef[:, i], dtype=np.float64)
            for j in range(nfac):
                dj = ((keys[:, i] >> np.uint64(2 * j)) & np.uint64(3)).astype(int)
                v = v * (pw[j][dj] if v.ndim == 1 else pw[j][dj][:, None])
            on = i < cnt
            acc = np.where(on if v.ndim == 1 else on[:, None], acc + v, acc)
        return acc
    g_t = slice_(a["tq_cen"], a["tq_keys"], a["tq_coef"], a["tq_cnt"])
    x = slice_(a["link_cen"], a["link_keys"], a["link_coef"], a["link_cnt"])[np.arange(a["A"].shape[0]) // a["O"]]
    best = np.full(a["A"].shape[0], -100000000.0)
    for p in range(36):
        A = a["A"][:, p]
        nz = (A != 0).any(1)
        dot = A[:, 0] * x[:, 0] + A[:, 1] * x[:, 1] + A[:, 2] * x[:, 2]
        pos, neg = dot - (a["d"][:, p] + a["delta"][:, p]), -dot - (-a["d"][:, p] + a["delta"][:, p])
        best = np.where(nz, np.maximum(best, np.maximum(pos, neg)), best)
    return np.concatenate([g_t, -best])


# --------------------------------------------------------------------------------------------------------------- the device
def _load(hb, robot=None, params=None, options=()):
    from armour_amd.planner import ArmourNLP
    nlp = ArmourNLP(T=T) if robot is None else ArmourNLP(robot=robot, params=params)
    for opt, v in options:
        nlp.set_option(opt, v)
    s = hb["state"]
    return nlp.debug_load_tables(s["q0"], s["qd0"], s["qdd0"], s["q_des"], hb["tables"])


def _masks_equal_the_rule(nlp, hb):
    nT, Q = hb["nT"], hb["Q"]
    _, _, gl, gu = nlp.get_bounds_info()
    assert np.array_equal(gl[:, :nT + Q], hb["gl"][:, :nT + Q]) and np.array_equal(gu[:, :nT + Q], hb["gu"][:, :nT + Q])
    rel, cnt, _ = nlp.row_relevance()
    sol, cnt2, tq2, _ = nlp.solver_rows()
    want_rel, want_sol = np.stack([r["rel"] for r in hb["res"]]), np.stack([r["solver"] for r in hb["res"]])
    assert rel.shape == want_rel.shape == (hb["B"], hb["m"])
    assert np.array_equal(rel, want_rel), np.argwhere(rel != want_rel)[:8]
    assert np.array_equal(sol, want_sol), np.argwhere(sol != want_sol)[:8]
    assert cnt.tolist() == rel[:, nT:nT + Q].sum(1).tolist() == REL_COUNTS
    assert cnt2.tolist() == sol[:, nT:nT + Q].sum(1).tolist() and tq2.tolist() == sol[:, :nT].sum(1).tolist() == TQ_SOL_COUNTS
    return rel, sol


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False])
def test_hand_built_masks_equal_the_rule_exactly(shared):
    """row_relevance() and solver_rows() after debug_load_tables -- the `any_normals` branch, where the solver's bound takes each plane's own norm --
    equal the restatement's masks in every row, and the three counts are the masks' sums."""
    hb = hand_built(shared)
    nlp = _load(hb)
    _masks_equal_the_rule(nlp, hb)
    nlp.close()


def _check_lists(nlp, rel, sol, A, d, delta, stored_d, obs_center=None):
    """the lists of both sets against the masks, and every packed entry against the table (A [B][T][J][O][36][3] ...).  stored_d: the packed d is the
    table's; else it is a0 oc0 + a1 oc1 + a2 oc2 in fp64, in that order, within 2 ulp."""
    B, n, J, O = nlp.B, nlp.n, nlp.J, nlp.O
    nT = nlp.m - J * T * O - 4 * n
    Q = J * T * O
    skip = nlp.plane_skip()
    for which, mask in ((0, rel), (1, sol)):
        ls = nlp.debug_row_lists(which)
        per = (Q + 255) // 256
        for b in range(B):
            want = np.flatnonzero(mask[b, nT:nT + Q])
            cnt = int(ls["count"][b])
            assert cnt == len(want) and np.array_equal(ls["rows"][b, :cnt], want), (which, b)
            if which == 0:
                assert ls["aux"].shape == (B, 256, per)
                for c in range(256):
                    wc = want[(nT + want) % 256 == c]
                    assert ls["aux_count"][b, c] == len(wc) and np.array_equal(ls["aux"][b, c, :len(wc)], wc), (b, c)
            else:
                wt = np.flatnonzero(mask[b, :nT])
                assert ls["aux_count"][b] == len(wt) and np.array_equal(ls["aux"][b, :len(wt)], wt), b
            off, stride = int(ls["pack_off"][b, 0]), int(ls["pack_off"][b, 1])
            assert stride == (cnt + 15) // 16 * 16
            live = [p for p in range(36) if not (int(skip[b]) >> p) & 1]
            block = ls["packed"][off:off + 5 * len(live) * stride].reshape(len(live), 5, stride)[:, :, :cnt]
            if b + 1 < B:
                assert int(ls["pack_off"][b + 1, 0]) == off + 5 * len(live) * stride
            lt, o = want // O, want % O
            l, tt = lt // T, lt % T
            for j, p in enumerate(live):
                for c in range(3):
                    assert np.array_equal(block[j, c], A[b, tt, l, o, p, c]), (which, b, p, c)
                assert np.array_equal(block[j, 4], delta[b, tt, l, o, p]), (which, b, p)
                if stored_d:
                    assert np.array_equal(block[j, 3], d[b, tt, l, o, p]), (which, b, p)
                else:
                    oc = obs_center[b, o]
                    ref = A[b, tt, l, o, p, 0] * oc[:, 0] + A[b, tt, l, o, p, 1] * oc[:, 1] + A[b, tt, l, o, p, 2] * oc[:, 2]
                    assert (np.abs(block[j, 3] - ref) <= 2 * np.spacing(np.abs(ref))).all(), (which, b, p)


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False])
def test_hand_built_lists_hold_the_masks_rows_and_their_plane_entries(shared):
    """armour_debug_get_row_lists on lists of 0, 1, 63, 64, 65, 255, 256, 257 (and 560) rows: rows ascending, the residue classes of (row0 + q) mod 256,
    the solver's torque rows, strides rounded up to 16, and every packed entry the table's entry of that live plane of that row, bit for bit."""
    from armour_amd import _lib
    hb = hand_built(shared)
    nlp = _load(hb)
    with pytest.raises(_lib.ArmourError):
        nlp.debug_row_lists(0)                     # (not built yet: ARMOUR_ESTATE)
    rel, sol = _masks_equal_the_rule(nlp, hb)
    t = hb["tables"]
    _check_lists(nlp, rel, sol, t["A"], t["d"], t["delta"], stored_d=True)
    nlp.close()


def test_the_list_hook_refuses_a_handle_without_a_problem_set():
    from armour_amd import _lib
    L = _lib.load()
    assert L.armour_debug_get_row_lists(None, 0, None, None, None, None, None, None, 0, None) == -4   # ARMOUR_ESTATE


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False])
def test_hand_built_culled_records_equal_the_full_ones_in_every_field(shared):
    """ARMOUR_OPT_CULL_ROWS = 1 on the hand-built lists (the empty one in the same launch as the one of 257 rows): at k = 0, at k = (1, .., 1) -- the
    corner at which the kept rows whose designated plane lies on the side their coefficients point to are violated by 1e-6, and no other -- and at a random point of the box, every field of
    the record equals the full test's, on the host entry and on the device entry; n_violated is the count of a numpy evaluation of g off the same
    tables (the 4n limit rows, which no table holds, from the full evaluation), no row within 1e-9 of its bound."""
    import ctypes as C
    import torch
    from armour_amd import _lib
    from armour_amd.worlds import random_k
    hb = hand_built(shared)
    B, n, nT, Q = hb["B"], hb["n"], hb["nT"], hb["Q"]
    full, culled = _load(hb), _load(hb, options=[(_lib.OPT_CULL_ROWS, 1)])
    _, _, gl, gu = full.get_bounds_info()
    for name, k in (("zero", np.zeros((B, n))), ("corner", np.ones((B, n))), ("random", random_k(41, B))):
        rf, rc = full.eval_violations(k), culled.eval_violations(k)
        assert rf == rc, (name, rf, rc)
        d_k = torch.tensor(k, device="cuda", dtype=torch.float64)
        d_out = torch.zeros(B * C.sizeof(_lib.ArmourViolation), device="cuda", dtype=torch.uint8)
        culled.eval_violations_device(d_k.data_ptr(), d_out.data_ptr())
        torch.cuda.synchronize()
        rec = (_lib.ArmourViolation * B).from_buffer_copy(d_out.cpu().numpy().tobytes())
        g_dev = full.eval_g(k)
        for b in range(B):
            for f in ("l1_violation", "worst", "worst_row", "n_violated", "n_outside_slack", "feasible"):
                assert getattr(rec[b], f) == rf[b][f], (name, b, f)
            g = np.concatenate([numpy_g(hb["tables"], b, k[b], n), g_dev[b, nT + Q:]])
            assert not (np.abs(g - gu[b]) <= 1e-9).any() and not (np.abs(g - gl[b]) <= 1e-9).any()
            nv = int(((g > gu[b]) | (g < gl[b])).sum())
            assert rf[b]["n_violated"] == nv, (name, b, rf[b], nv)
            if name == "corner":   # the known subset: kept rows whose designated plane lies on the side the coefficients point to, no dropped row
                kept = hb["target"][b] == "A"
                assert np.array_equal(g[nT:nT + Q] > 0, hb["corner"][b]) and not (hb["corner"][b] & ~kept).any()
                assert REL_COUNTS[b] < 60 or 0.2 * kept.sum() < hb["corner"][b].sum() < kept.sum()
    full.close(); culled.close()


@pytest.mark.gpu
def test_hand_built_culled_solve_equals_the_full_one():
    """ARMOUR_OPT_SOLVE_CULL = 1 against 0 on the hand-built set, device form, as tests/test_solve.py compares them."""
    from armour_amd import _lib
    hb = hand_built(True)
    nlp = _load(hb)
    nlp.set_option(_lib.OPT_SOLVE_CULL, 0)
    full = nlp.solve(device_qp=True)
    nlp.set_option(_lib.OPT_SOLVE_CULL, 1)
    cul = nlp.solve(device_qp=True)
    for b, (a, c) in enumerate(zip(full, cul)):
        assert (np.array_equal(a["k_opt"], c["k_opt"]) and a["feasible"] == c["feasible"] and a["iterations"] == c["iterations"]
                and a["evaluations"] == c["evaluations"] and a["status"] == c["status"] and a["cost"] == c["cost"]
                and a["max_violation"] == c["max_violation"]), (b, a, c)
    assert any(a["iterations"] >= 1 for a in full)
    nlp.close()


# --------------------------------------------------------------------------------------------------------------- built tables
def _device_tables(nlp):
    """the device's own tables in the loader's layout, with its live planes [B][36]"""
    B, J, n, O = nlp.B, nlp.J, nlp.n, nlp.O
    capL, capT = 32, 128
    t = dict(link_count=np.zeros((B, J, T), np.int32), link_center=np.zeros((B, J, T, 2, 3)), link_keys=np.zeros((B, J, T, capL), np.uint64),
             link_coeffs=np.zeros((B, J, T, capL, 3)), torque_count=np.zeros((B, n, T), np.int32), torque_center=np.zeros((B, n, T, 2)),
             torque_keys=np.zeros((B, n, T, capT), np.uint64), torque_coeffs=np.zeros((B, n, T, capT)))
    for b in range(B):
        for which, cnt in (("link", J), ("torque", n)):
            for i in range(cnt):
                for tt in range(T):
                    cen, _, keys, co = nlp.pz(which, i, tt, b=b)
                    M = len(keys)
                    pre = "link" if which == "link" else "torque"
                    t[pre + "_count"][b, i, tt] = M
                    t[pre + "_center"][b, i, tt, 0] = cen if which == "link" else cen[0]
                    t[pre + "_keys"][b, i, tt, :M] = keys
                    t[pre + "_coeffs"][b, i, tt, :M] = co if which == "link" else co[:, 0]
    t["A"], t["d"], t["delta"] = nlp.hyperplanes()
    skip = nlp.plane_skip()
    live = np.array([[not (int(skip[b]) >> p) & 1 for p in range(36)] for b in range(B)])
    return t, live


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["random_problem(77, 12)", "random_batch(40, 8, 6)"])
def test_built_masks_and_lists_equal_the_rule(which):
    """set_parameters at T = 40 (B = 1: d stored; B = 8: lean tables, d recomputed from the obstacle centres): the device's own tables read back, the
    restatement applied over the live planes and over all 36 (a skipped plane is degenerate or a +- duplicate of a live one: same verdicts), both
    device masks equal to it on every decided row, no row undecided (cap, should a device run show some: 0.1 % of a problem's rows); the lists and
    the packed entries as on the hand-built set."""
    from armour_amd.planner import ArmourNLP
    from armour_amd.worlds import random_batch, random_problem
    p = random_problem(77, 12) if which.startswith("random_problem") else random_batch(40, 8, 6)
    nlp = ArmourNLP(T=T).set_parameters(p["q0"], p["qd0"], p["qdd0"], p["q_des"], p["obstacles"])
    B, n, O = nlp.B, nlp.n, nlp.O
    nT, Q = n * T, nlp.J * T * O
    _, _, gl, gu = nlp.get_bounds_info()
    rel, cnt, _ = nlp.row_relevance()
    sol, cnt2, tq2, _ = nlp.solver_rows()
    t, live = _device_tables(nlp)
    undecided, near = 0, np.inf
    for b in range(B):
        res = rr.row_rule(**rule_args(t, b, gl[b], gu[b], live=live[b], unit_normals=True))
        res36 = rr.row_rule(**rule_args(t, b, gl[b], gu[b], unit_normals=True))
        for key, dev in (("rel", rel[b]), ("solver", sol[b])):
            und, und36 = res["undecided_" + key], res36["undecided_" + key]
            undecided += int(und.sum())
            assert und.sum() <= 1e-3 * nlp.m
            ok = ~und & ~und36
            assert np.array_equal(res[key][ok], res36[key][ok]), (b, key, np.flatnonzero(res[key] != res36[key])[:8])
            assert np.array_equal(dev[~und], res[key][~und]), (b, key, np.flatnonzero(dev != res[key])[:8])
        near = min(near, closest(res, "rel", slice(nT, nT + Q)), closest(res, "solver", slice(nT, nT + Q)))
        assert cnt[b] == rel[b, nT:nT + Q].sum() and cnt2[b] == sol[b, nT:nT + Q].sum() and tq2[b] == sol[b, :nT].sum()
    counts = (int(cnt.sum()), int(cnt2.sum()), int(rel[:, :nT].sum()))
    print(f"{which}: undecided rows {undecided}; closest collision row {near:.2e} from a threshold; relevant / solver collision rows, relevant torque rows {counts}")
    assert undecided == 0
    assert counts == ((86, 219, 19) if B == 1 else (519, 989, 132))
    obs = np.asarray(p["obstacles"], dtype=float).reshape(B, O, 12)
    _check_lists(nlp, rel, sol, t["A"], t["d"], t["delta"], stored_d=(B == 1), obs_center=obs[:, :, 0:3])
    nlp.close()


# --------------------------------------------------------------------------------------------------------------- the 128-bit-key ABI
def _body_key128():
    """(runs with ARMOUR_KEY128=1)  the hand-built masks on the eight-factor arm: a monomial of degree 3 in the EIGHTH factor (bits 14-15 of the
    table key) decides rows -- the last step of the kernels' degree loop, which runs to ARMOUR_MAX_FACTORS."""
    sys.path.insert(0, ROOT)
    from armour_amd import _lib
    from armour_amd.planner import default_params, kinova_robot
    import test_key128 as tk
    assert _lib.MAXF == 8
    hb = hand_built(True, nfac=8)
    check_hand_built(hb)
    top = np.uint64(3 << 14)
    assert (hb["tables"]["link_keys"] == top).any() and (hb["tables"]["torque_keys"] == top).any()
    params = default_params(T)
    params.k_range[7] = params.k_range[6]
    nlp = _load(hb, robot=tk.make_eight_factor_arm(kinova_robot()), params=params)
    assert (nlp.n, nlp.J, nlp.m) == (8, 8, hb["m"])
    _masks_equal_the_rule(nlp, hb)
    nlp.close()
    print("key128 masks ok", flush=True)


@pytest.mark.gpu
def test_hand_built_masks_in_the_128_bit_key_abi():
    env = dict(os.environ, ARMOUR_KEY128="1")
    env.pop("ARMOUR_HIP_LIB", None)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_row_masks as t; t._body_key128()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "key128 masks ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_hand_built_tables_for_eight_factors_fix_every_row():
    """CPU: the eight-factor set's promises (it needs no library: the rule and numpy alone)"""
    hb = hand_built(True, nfac=8)
    check_hand_built(hb)
    assert (hb["tables"]["link_keys"] == np.uint64(3 << 14)).any()
