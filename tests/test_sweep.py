"""armour_sweep (S candidates of the same problems judged in one go) and the rescue built on it: candidate set, selection rule and merge on the
CPU, scenario checks with the CPU oracle, and on the GPU parity with armour_eval_violations / armour_eval_f, independence, the oracle, argument
checks, the rescue on eight named reference worlds, and the wiring into run_trials."""
import numpy as np
import pytest

T = 40
# eight of the reference's worlds (first planning iteration) on which the CPU oracle finds candidate 0 safe and another candidate of the S = 32 set
# safe at a lower cost: chosen with the oracle, asserted in test_rescue_worlds_qualify_by_the_oracle
RESCUE_WORLDS = ("scene_013_001", "scene_013_002", "scene_013_003", "scene_013_004", "scene_013_005", "scene_013_006", "scene_013_007", "scene_013_008")
RESCUE_S = 32
# the parity problems: worlds.random_batch(seed, B, O) -- moving random states, B in {1, 3}, O in {1, 7, 20}
PARITY_PROBLEMS = ((5300, 1, 1), (5100, 3, 7), (5200, 1, 20))
PARITY_S = 67


def _rescue_worlds():
    from armour_amd import scenes
    by_name = dict(scenes.reference_worlds())
    return [(name, by_name[name]) for name in RESCUE_WORLDS]


def reference_records(g, gl, gu, row0, Q, n_checked, torque_slack, collision_slack):
    """numpy restatement of armour_eval_violations' record from the full g of ONE problem (in the style of tests/test_batch_api.py)."""
    viol = np.maximum(0.0, np.maximum(gl - g, g - gu))
    out = np.zeros(g.shape[0], bool)
    out[:row0] = (g[:row0] < gl[:row0] - torque_slack) | (g[:row0] > gu[:row0] + torque_slack)
    c = slice(row0, row0 + Q)
    out[c] = (np.arange(Q) < n_checked) & (g[c] > collision_slack)
    out[row0 + Q:] = (g[row0 + Q:] < gl[row0 + Q:]) | (g[row0 + Q:] > gu[row0 + Q:])
    return dict(l1=float(viol.sum()), worst=float(viol.max()), worst_row=int(np.argmax(viol)) if viol.max() > 0 else -1,
                n_violated=int((viol > 0).sum()), n_outside_slack=int(out.sum()), feasible=int(not out.any()))


def _oracle_records(o, cand):
    """(records, costs, g) of the candidates of one oracle problem."""
    _, _, gl, gu = o.bounds()
    row0, Q = o.n * o.T, o.J * o.T * o.O
    recs, costs, gs = [], [], []
    for k in cand:
        g, _ = o.eval_g_jac(k, want_jac=False)
        recs.append(reference_records(g, gl, gu, row0, Q, Q, o.params.torque_violation_threshold, o.params.collision_violation_threshold))
        costs.append(o.eval_f(k))
        gs.append(g)
    return recs, np.array(costs), np.array(gs)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_new_entries_are_exported():
    from armour_amd import _lib
    L = _lib.load()
    for name in ("armour_sweep", "armour_solve_from", "armour_sweep_tile"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    import ctypes as C
    assert C.sizeof(_lib.ArmourSweepRecord) == 40
    from armour_amd.planner import SWEEP_DTYPE
    assert SWEEP_DTYPE.itemsize == 40
    assert 1 <= L.armour_sweep_tile() <= 64


def _halton_by_hand(i, base):
    digits = []
    while i:
        digits.append(i % base)
        i //= base
    return sum(d / base ** (p + 1) for p, d in enumerate(digits))


def test_sweep_candidates():
    from armour_amd.planner import sweep_candidates
    k = sweep_candidates(7, 128)
    assert k.shape == (128, 7) and not k[0].any()
    assert np.all(np.abs(k) <= 1.0)
    assert np.array_equal(k, sweep_candidates(7, 128))
    assert np.array_equal(sweep_candidates(7, 64), k[:64])
    # the first points by hand: base 2 gives 1/2, 1/4, 3/4, 1/8, 5/8, ...; base 3 gives 1/3, 2/3, 1/9, 4/9, ...
    assert np.allclose(k[1:6, 0], 2 * np.array([1 / 2, 1 / 4, 3 / 4, 1 / 8, 5 / 8]) - 1, rtol=0, atol=1e-15)
    assert np.allclose(k[1:5, 1], 2 * np.array([1 / 3, 2 / 3, 1 / 9, 4 / 9]) - 1, rtol=0, atol=1e-15)
    primes = (2, 3, 5, 7, 11, 13, 17)
    for i in range(1, 16):
        for j, p in enumerate(primes):
            assert abs(k[i, j] - (2 * _halton_by_hand(i, p) - 1)) <= 1e-15, (i, j)
    assert sweep_candidates(3, 5).shape == (5, 3)
    with pytest.raises(ValueError):
        sweep_candidates(7, 0)


def test_best_candidate_rule():
    from armour_amd.planner import best_candidate
    feas = np.array([[0, 1, 1, 1], [0, 0, 0, 0], [1, 1, 0, 1], [1, 0, 0, 0]])
    cost = np.array([[0.1, 3.0, 2.0, 2.0], [1.0, 1.0, 1.0, 1.0], [5.0, 5.0, 1.0, 5.0], [9.0, 1.0, 1.0, 1.0]])
    # cheapest among the feasible; the lowest index among equals; -1 if none; an infeasible candidate never wins however cheap
    assert best_candidate(feas, cost).tolist() == [2, -1, 0, 0]


def _res(feasible, cost, k=0.0, **kw):
    return dict(k_opt=np.full(7, k), cost=cost, max_violation=0.0 if feasible else 1.0, feasible=feasible, iterations=3, evaluations=4, status=1, time_ms=0.1, **kw)


def test_merge_rescue_codes():
    from armour_amd.planner import SWEEP_DTYPE, best_candidate, merge_rescue
    cand = np.array([[0.0] * 7, [0.25] * 7, [0.5] * 7])
    rec = np.zeros((5, 3), dtype=SWEEP_DTYPE)
    rec["feasible"] = [[1, 1, 1], [0, 1, 1], [0, 1, 1], [0, 0, 0], [0, 1, 1]]
    rec["cost"] = [[1, 1, 1], [9, 4, 4], [9, 5, 4], [1, 1, 1], [9, 4, 3]]
    best = best_candidate(rec["feasible"], rec["cost"])
    assert best.tolist() == [0, 1, 2, -1, 2]                        # problem 1: the tie goes to the lower index
    first = [_res(True, 7.0, k=0.9), _res(False, 8.0), _res(False, 8.0), _res(False, 8.0), _res(False, 8.0)]
    refined = [_res(True, 0.5, k=-0.9), _res(True, 3.5, k=0.3), _res(True, 4.5, k=0.4), _res(True, 0.1), _res(False, 0.1, k=0.7)]
    out, code = merge_rescue(first, cand, rec, best, refined)
    assert code.tolist() == [0, 2, 1, -1, 1]
    assert out[0] is first[0]                                       # a feasible first result is never replaced, however good the refined one
    assert out[1] is refined[1]                                     # refined, feasible and no dearer than its candidate
    # a refined result dearer than its candidate loses to the candidate: the candidate itself is the plan
    assert out[2]["feasible"] is True and out[2]["cost"] == 4.0 and np.array_equal(out[2]["k_opt"], cand[2])
    assert out[3] is first[3]                                       # no safe candidate: the failure stays (whatever the refined solve says)
    assert out[4]["cost"] == 3.0 and np.array_equal(out[4]["k_opt"], cand[2])   # an infeasible refined result loses as well
    # per-problem candidates, and no refined solve at all
    out, code = merge_rescue(first, np.stack([cand + 0.01 * b for b in range(5)]), rec, best, None)
    assert code.tolist() == [0, 1, 1, -1, 1] and np.array_equal(out[1]["k_opt"], cand[1] + 0.01)


def test_rescue_worlds_qualify_by_the_oracle():
    """Part one of the scenario check: on each named world candidate 0 is safe and another candidate of the S = 32 set is safe at a lower cost."""
    from armour_amd.planner import best_candidate, sweep_candidates
    from oracle.cpu_oracle import Oracle
    cand = sweep_candidates(7, RESCUE_S)
    o = Oracle(T=T)
    for name, p in _rescue_worlds():
        o.set_problem(p["q0"], p["qd0"], p["qdd0"], p["q_des"], p["obstacles"])
        recs, cost, _ = _oracle_records(o, cand)
        feas = np.array([r["feasible"] for r in recs])
        best = best_candidate(feas[None], cost[None])[0]
        assert feas[0] == 1 and best > 0 and cost[best] < cost[0], (name, feas[0], best)


def test_parity_problems_have_both_verdicts_by_the_oracle():
    """Part two: the candidate set gives the parity problems both safe and unsafe records (one of them both at once)."""
    from armour_amd.planner import sweep_candidates
    from armour_amd.worlds import random_batch
    from oracle.cpu_oracle import Oracle
    cand = sweep_candidates(7, PARITY_S)
    counts = []
    for seed, B, O in PARITY_PROBLEMS:
        bp = random_batch(seed, B, O)
        for b in range(B):
            o = Oracle(T=T).set_problem(bp["q0"][b], bp["qd0"][b], bp["qdd0"][b], bp["q_des"][b], bp["obstacles"][b])
            recs, _, _ = _oracle_records(o, cand)
            counts.append(sum(r["feasible"] for r in recs))
    assert any(0 < c < PARITY_S for c in counts), counts
    assert any(c == 0 for c in counts) and any(c > 0 for c in counts), counts


# ---------------------------------------------------------------------------------------------------------------- GPU
def _compare_with_entries(nlp, cand, sw, per_problem):
    """every record of a sweep against armour_eval_violations (culled and full) and armour_eval_f at the same point"""
    from armour_amd import _lib
    from armour_amd.planner import best_candidate
    rec, B = sw["records"], nlp.B
    S = rec.shape[1]
    for cull in (1, 0):
        nlp.set_option(_lib.OPT_CULL_ROWS, cull)
        for s in range(S):
            k = cand[:, s] if per_problem else np.tile(cand[s], (B, 1))
            ref, f = nlp.eval_violations(k), nlp.eval_f(k)
            for b in range(B):
                r, e = rec[b, s], ref[b]
                for fld in ("worst_row", "n_violated", "n_outside_slack"):
                    assert r[fld] == e[fld], (cull, b, s, fld, r, e)
                assert bool(r["feasible"]) == e["feasible"] and r["worst"] == e["worst"], (cull, b, s, r, e)
                assert abs(r["l1_violation"] - e["l1_violation"]) <= nlp.m * 2.0 ** -52 * e["l1_violation"], (cull, b, s, r, e)
                assert r["cost"] == f[b], (b, s)
    nlp.set_option(_lib.OPT_CULL_ROWS, 0)
    assert np.array_equal(sw["best"], best_candidate(rec["feasible"], rec["cost"]))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,B,O", PARITY_PROBLEMS)
def test_sweep_equals_the_existing_entries(seed, B, O):
    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP, sweep_candidates
    from armour_amd.worlds import random_batch
    C = _lib.load().armour_sweep_tile()
    bp = random_batch(seed, B, O)
    nlp = ArmourNLP(T=T).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    full = sweep_candidates(nlp.n, PARITY_S)
    verdicts = set()
    for S in sorted({1, max(1, C - 1), C, C + 1, PARITY_S}):
        sw = nlp.sweep(full[:S])
        _compare_with_entries(nlp, full[:S], sw, False)
        verdicts |= set(sw["records"]["feasible"].ravel().tolist())
    assert verdicts <= {0, 1}
    # per-problem candidates: problem b takes the shared set rotated by b
    S = C + 1
    per = np.stack([np.roll(full[:S], b, axis=0) for b in range(B)])
    _compare_with_entries(nlp, per, nlp.sweep(per, per_problem=True), True)
    nlp.close()


@pytest.mark.gpu
def test_sweep_sees_both_verdicts_on_the_parity_problems():
    from armour_amd.planner import ArmourNLP, sweep_candidates
    from armour_amd.worlds import random_batch
    seen = set()
    for seed, B, O in PARITY_PROBLEMS:
        bp = random_batch(seed, B, O)
        nlp = ArmourNLP(T=T).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
        seen |= set(nlp.sweep(sweep_candidates(nlp.n, PARITY_S))["records"]["feasible"].ravel().tolist())
        nlp.close()
    assert seen == {0, 1}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["armtd", "input_constraints_off", "gripper", "far_obstacle"])
def test_sweep_modes(mode):
    """ARMTD comparison mode, no torque rows, the 8-link gripper preset, and a problem whose row list is empty (one far obstacle)."""
    from armour_amd import scenes
    from armour_amd.planner import ArmourNLP, default_params, kinova_gripper_robot, sweep_candidates
    from armour_amd.worlds import random_batch, synthetic_offline_jrs
    B, O, S = 3, 7, 9
    bp = random_batch(5100, B, O)
    if mode == "armtd":
        jk = [synthetic_offline_jrs(bp["qd0"][b], T) for b in range(B)]
        nlp = ArmourNLP(T=T).set_parameters_armtd(bp["q0"], bp["qd0"], bp["q_des"], np.stack([j for j, _ in jk]), np.stack([k for _, k in jk]), bp["obstacles"])
        assert nlp.m == nlp.J * T * O + 4 * nlp.n
    elif mode == "input_constraints_off":
        pr = default_params(T)
        pr.input_constraints_off = 1
        nlp = ArmourNLP(params=pr).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
        assert nlp.m == nlp.J * T * O + 4 * nlp.n
    elif mode == "gripper":
        nlp = ArmourNLP(robot=kinova_gripper_robot(), T=T).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
        assert nlp.J == 8
    else:
        far = np.tile(scenes.FAR_BOX, (B, 1, 1))
        nlp = ArmourNLP(T=T).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], far)
        assert not nlp.row_relevance()[1].any()
    cand = sweep_candidates(nlp.n, S)
    _compare_with_entries(nlp, cand, nlp.sweep(cand), False)
    nlp.close()


def _body_k128():
    """(runs with ARMOUR_KEY128=1: libarmour_hip_k128.so, ARMOUR_MAX_FACTORS = 8)  The eight-factor arm of tests/test_key128.py, two problems,
    S = C + 1 candidates in the first eight primes: every record against armour_eval_violations / armour_eval_f, best against the numpy rule."""
    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP, default_params, kinova_robot, sweep_candidates
    from test_key128 import make_eight_factor_arm
    assert _lib.MAXF == 8 and _lib.load().armour_abi_max_factors() == 8
    n, O, B = 8, 7, 2
    rng = np.random.default_rng(2025)
    lb = np.array([-np.pi, -2.41, -np.pi, -2.66, -np.pi, -2.23, -np.pi, -2.2]) + 0.3
    q0 = rng.uniform(lb, -lb, (B, n))
    qd0, qdd0 = rng.uniform(-0.3, 0.3, (B, n)), rng.uniform(-0.5, 0.5, (B, n))
    q_des = q0 + rng.uniform(-np.pi / 8, np.pi / 8, (B, n))
    obs = np.zeros((B, O, 12))
    obs[:, :, 0:3] = rng.uniform([-0.8, -0.8, 0.05], [0.8, 0.8, 1.2], (B, O, 3))
    sz = rng.uniform(0.01, 0.5, (B, O, 3))
    obs[:, :, 3], obs[:, :, 7], obs[:, :, 11] = sz[:, :, 0] / 2, sz[:, :, 1] / 2, sz[:, :, 2] / 2
    pr = default_params(T)
    pr.k_range[7] = pr.k_range[6]
    nlp = ArmourNLP(robot=make_eight_factor_arm(kinova_robot()), params=pr).set_parameters(q0, qd0, qdd0, q_des, obs)
    assert (nlp.n, nlp.J, nlp.m) == (8, 8, 8 * T + 8 * T * O + 32)
    C = _lib.load().armour_sweep_tile()
    cand = sweep_candidates(8, C + 1)
    assert cand.shape == (C + 1, 8) and cand[1, 7] == 2.0 / 19 - 1.0       # the eighth prime
    _compare_with_entries(nlp, cand, nlp.sweep(cand), False)
    per = np.stack([cand, cand[::-1]])
    _compare_with_entries(nlp, per, nlp.sweep(per, per_problem=True), True)
    nlp.close()
    print("sweep k128 ok", flush=True)


@pytest.mark.gpu
def test_sweep_with_128_bit_keys_and_eight_factors():
    """The one configuration with ARMOUR_MAX_FACTORS = 8 and n = 8: 8-entry k-power tables, products over eight factors, an 8-bit continuous mask,
    the 8-prime candidate set.  The ABI is chosen per process, so the body runs in a child (the loader pattern of tests/test_key128.py)."""
    import os

    from test_key128 import ROOT, _run
    r = _run("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_sweep as t; t._body_k128()" % (ROOT, os.path.join(ROOT, "tests")))
    assert r.returncode == 0 and "sweep k128 ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_sweep_records_depend_on_problem_and_point_only():
    from armour_amd.planner import ArmourNLP, sweep_candidates
    from armour_amd.worlds import random_batch
    bp = random_batch(5100, 3, 7)
    nlp = ArmourNLP(T=T).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    cand = sweep_candidates(nlp.n, PARITY_S)
    a = nlp.sweep(cand)
    again = nlp.sweep(cand)
    assert a["records"].tobytes() == again["records"].tobytes() and np.array_equal(a["best"], again["best"])   # the same call twice
    alone = nlp.sweep(cand[65:66])                                   # S = 1 against position 65 of S = 67
    assert alone["records"][:, 0].tobytes() == a["records"][:, 65].tobytes()
    per = nlp.sweep(np.stack([cand] * 3), per_problem=True)          # per_problem with the same points
    assert per["records"].tobytes() == a["records"].tobytes()
    nlp.close()
    one = ArmourNLP(T=T).set_parameters(*(bp[f][1:2] for f in ("q0", "qd0", "qdd0", "q_des", "obstacles")))   # problem 1 of B = 3, alone
    solo = one.sweep(cand)
    assert solo["records"][0].tobytes() == a["records"][1].tobytes() and solo["best"][0] == a["best"][1]
    one.close()


@pytest.mark.gpu
def test_sweep_against_the_oracle():
    """One problem, 16 candidates, against the live oracle's g: verdicts and counts wherever no row lies within 1e-9 of a bound or slack, l1 to 1e-9."""
    from armour_amd.planner import ArmourNLP, sweep_candidates
    from armour_amd.worlds import random_batch
    from oracle.cpu_oracle import Oracle
    seed, B, O = PARITY_PROBLEMS[0]
    bp = random_batch(seed, B, O)
    nlp = ArmourNLP(T=T).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    o = Oracle(T=T).set_problem(bp["q0"][0], bp["qd0"][0], bp["qdd0"][0], bp["q_des"][0], bp["obstacles"][0])
    cand = sweep_candidates(nlp.n, 16)
    rec = nlp.sweep(cand)["records"][0]
    recs, cost, gs = _oracle_records(o, cand)
    _, _, gl, gu = o.bounds()
    row0, Q = o.n * o.T, o.J * o.T * o.O
    ts, cs = o.params.torque_violation_threshold, o.params.collision_violation_threshold
    compared = 0
    for s in range(16):
        g = gs[s]
        edges = [g - gl, g - gu, g[:row0] - (gl[:row0] - ts), g[:row0] - (gu[:row0] + ts), g[row0:row0 + Q] - cs]
        assert abs(rec[s]["l1_violation"] - recs[s]["l1"]) <= 1e-9 * max(1.0, recs[s]["l1"])
        assert abs(rec[s]["cost"] - cost[s]) <= 1e-9 * max(1.0, abs(cost[s]))
        if min(np.abs(e[np.isfinite(e)]).min() for e in edges) <= 1e-9:
            continue
        compared += 1
        for fld in ("n_violated", "n_outside_slack", "feasible"):
            assert rec[s][fld] == recs[s][fld], (s, fld)
    assert compared >= 8


@pytest.mark.gpu
def test_sweep_refuses_bad_arguments_and_the_handle_lives_on():
    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP, sweep_candidates
    from armour_amd.worlds import random_batch
    bp = random_batch(5300, 1, 1)
    nlp = ArmourNLP(T=T).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    good = sweep_candidates(nlp.n, 8)
    for bad in (np.where(np.arange(56).reshape(8, 7) == 30, 1.0 + 1e-12, good), np.where(np.arange(56).reshape(8, 7) == 5, np.nan, good),
                np.where(np.arange(56).reshape(8, 7) == 55, -np.inf, good), np.zeros((0, 7)), np.zeros((_lib.SWEEP_MAX_CANDIDATES + 1, 7))):
        with pytest.raises(_lib.ArmourError) as ei:
            nlp.sweep(bad)
        assert ei.value.code == _lib.EINVAL
    sw = nlp.sweep(good)
    _compare_with_entries(nlp, good, sw, False)
    nlp.close()


def _full_g_feasible(nlp, k):
    g, _ = nlp.eval_g_jac(k)
    return nlp.finalize_solution(g)


@pytest.mark.gpu
def test_rescue_on_the_named_worlds():
    """Every one of the eight worlds, with its first solve marked failed, is rescued: a plan that the full-g check accepts, at a cost that is at
    most its best candidate's (the CPU leg has shown that the inputs qualify)."""
    from armour_amd import scenes
    from armour_amd.planner import ArmourNLP, sweep_candidates
    bt = scenes.as_batch(_rescue_worlds())
    nlp = ArmourNLP(T=T)
    nlp.set_parameters(bt["q0"], bt["qd0"], bt["qdd0"], bt["q_des"], bt["obstacles"])
    first = [dict(r, feasible=False) for r in nlp.solve()]
    cand = sweep_candidates(nlp.n, RESCUE_S)
    sw = nlp.sweep(cand)
    res, rescued = nlp.solve_rescued(S=RESCUE_S, first=first)
    assert (rescued >= 1).all(), rescued
    feas = _full_g_feasible(nlp, np.stack([r["k_opt"] for r in res]))
    f = nlp.eval_f(np.stack([r["k_opt"] for r in res]))
    for b, r in enumerate(res):
        assert sw["best"][b] >= 0
        assert r["feasible"] and feas[b], (b, rescued[b])
        assert r["cost"] <= sw["records"][b, sw["best"][b]]["cost"] and f[b] == r["cost"], (b, rescued[b], r["cost"])
    # a feasible first solve is left alone
    kept, code = nlp.solve_rescued(S=RESCUE_S)
    again = nlp.solve()
    for r, e, c in zip(kept, again, code):
        if e["feasible"]:
            assert c == 0 and np.array_equal(r["k_opt"], e["k_opt"]) and r["cost"] == e["cost"]
    nlp.close()


@pytest.mark.gpu
def test_trials_with_and_without_rescue():
    """Guards the WIRING of rescue_candidates into run_trials, not its effect: these four worlds may see no rescue at all.  rescue_candidates = 0 is
    the run without the argument; with 64 candidates no executed piece collides and whatever was rescued is a feasible plan."""
    from armour_amd import scenes
    from armour_amd.trials import run_trials
    worlds = scenes.reference_worlds()[:4]
    kw = dict(T=T, max_iterations=6, per_step_build=True)
    base = run_trials(worlds, **kw)
    zero = run_trials(worlds, rescue_candidates=0, **kw)
    for a, b in zip(base["worlds"], zero["worlds"]):
        assert a["outcome"] == b["outcome"] and len(a["records"]) == len(b["records"])
        for ra, rb in zip(a["records"], b["records"]):
            assert np.array_equal(ra["k_opt"], rb["k_opt"], equal_nan=True) and ra["feasible"] == rb["feasible"] and rb["rescued"] == 0
    assert zero["summary"]["rescued_iterations"] == 0
    resc = run_trials(worlds, rescue_candidates=64, **kw)
    n_rescued = 0
    for w in resc["worlds"]:
        for r in w["records"]:
            assert r["audit_verdict"] != 1, (w["name"], r["iteration"])
            assert r["rescued"] in (-1, 0, 1, 2)
            if r["rescued"] > 0:
                n_rescued += 1
                assert r["feasible"]
    assert resc["summary"]["rescued_iterations"] == n_rescued
