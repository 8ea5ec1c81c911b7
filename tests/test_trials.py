"""Whole planning trials (armour_amd/trials.py): the re-planning loop over W worlds in lockstep.

CPU: the loop's logic with a scripted planner backend (state hand-over, braking, the failure count, leaving the batch, the goal check).
GPU: iteration 1 against armour_solve on the reference's worlds, the safety claim over whole trials, moving-arm inputs against the live
oracle, independence of the batch, a synthetic short move, and tracked execution."""
import numpy as np
import pytest

from test_pz_ops import margin_agrees
from test_reference_scenes import C_TOL, G_TOL, J_TOL, R_TOL, _rows_differ_only_through_noise_planes

K_RANGE = np.full(7, np.pi / 48)
START = np.array([0.0, 0.6, 0.0, 1.2, 0.0, 0.6, 0.0])


# ----------------------------------------------------------------------------------------------------------- a scripted backend
class ScriptedPlanner:
    """plan() answers from a script per world: script[w] = list of (feasible, k) per planning iteration of that world (the last entry
    repeats).  A world is recognised by the x coordinate of its (far) obstacle, 100 + w."""

    def __init__(self, scripts):
        from armour_amd.planner import kinova_robot
        self.robot, self.k_range, self.duration, self.t_plan = kinova_robot(), K_RANGE, 1.0, 0.5
        self.scripts, self.calls, self.batches = scripts, {w: 0 for w in scripts}, []

    def plan(self, q0, qd0, qdd0, q_des, obstacles):
        ids = [int(round(o[0, 0])) - 100 for o in obstacles]
        self.batches.append(ids)
        out = []
        for w in ids:
            sc = self.scripts[w]
            feasible, k = sc[min(self.calls[w], len(sc) - 1)]
            self.calls[w] += 1
            out.append(dict(k_opt=np.asarray(k, dtype=np.float64) if feasible else np.full(7, np.nan), feasible=feasible, iterations=3, time_ms=0.1))
        return out, 1.0, 2.0


def _world(w, start, goal, lookahead=1.0):
    far = np.array([[100.0 + w, 0, 0, 0.01, 0, 0, 0, 0.01, 0, 0, 0, 0.01]])
    return (f"w{w}", dict(q0=np.asarray(start, dtype=np.float64), goal=np.asarray(goal, dtype=np.float64), obstacles=far, lookahead=lookahead))


def _run(worlds, scripts, **kw):
    from armour_amd.trials import run_trials
    be = ScriptedPlanner(scripts)
    return run_trials(worlds, backend=be, audit_on_host=True, **kw), be


# ----------------------------------------------------------------------------------------------------------- CPU
def test_state_hand_over_is_c2_and_the_braking_piece_ends_at_rest():
    from armour_amd.planner import desired_trajectory
    k1, k2 = np.full(7, 0.8), np.array([0.5, -1, 0.2, 0, 1, -0.3, 0.7])
    goal = START + 3.0
    res, _ = _run([_world(0, START, goal)], {0: [(True, k1), (True, k2), (False, None), (False, None), (True, k1)]}, max_iterations=5, stop_threshold=4)
    recs = res["worlds"][0]["records"]
    assert [r["executed"] for r in recs] == ["plan", "plan", "brake", "stay", "plan"]
    assert np.array_equal(recs[0]["q0"], START) and not recs[0]["qd0"].any() and not recs[0]["qdd0"].any()
    want = desired_trajectory(START, np.zeros(7), np.zeros(7), k1, 0.5, k_range=K_RANGE)
    for got, w in zip((recs[1]["q0"], recs[1]["qd0"], recs[1]["qdd0"]), want):
        assert np.array_equal(got, w)
    assert np.abs(recs[1]["qd0"]).min() > 0                                      # a moving-arm input
    want = desired_trajectory(recs[1]["q0"], recs[1]["qd0"], recs[1]["qdd0"], k2, 0.5, k_range=K_RANGE)
    for got, w in zip((recs[2]["q0"], recs[2]["qd0"], recs[2]["qdd0"]), want):
        assert np.array_equal(got, w)
    # iteration 3 found no plan: the arm runs the second plan's braking half and is then at rest at that plan's end
    piece = recs[2]["piece"]
    assert np.array_equal(piece[0], recs[1]["q0"]) and np.array_equal(piece[3], k2) and piece[4:] == (0.5, 1.0)
    end = desired_trajectory(recs[1]["q0"], recs[1]["qd0"], recs[1]["qdd0"], k2, 1.0, k_range=K_RANGE)
    assert np.array_equal(recs[3]["q0"], end[0]) and np.abs(end[1]).max() <= 1e-14 and np.abs(end[2]).max() <= 1e-12
    assert not recs[3]["qd0"].any() and not recs[3]["qdd0"].any()
    # iteration 4 found none either: already at rest, the arm stays, and iteration 5 plans from the same state
    assert np.array_equal(recs[4]["q0"], recs[3]["q0"]) and not recs[4]["qd0"].any()
    assert [r["fails"] for r in recs] == [0, 0, 1, 2, 0]
    assert res["worlds"][0]["outcome"] == "iteration_limit" and res["summary"]["iteration_limit"] == 1
    from armour_amd.trials import moving_states
    ms = moving_states(res)
    assert len(ms) == 4 and np.array_equal(ms[0][1], recs[1]["qd0"]) and ms[0][4].shape == (1, 12)


@pytest.mark.parametrize("threshold", [0, 2, 4])
def test_stuck_exactly_when_the_failure_count_exceeds_the_threshold(threshold):
    k = np.full(7, 0.5)
    script = [(True, k)] + [(False, None)] * 2 + [(True, k)] + [(False, None)] * 50
    res, _ = _run([_world(0, START, START + 3.0)], {0: script}, stop_threshold=threshold, max_iterations=100)
    w = res["worlds"][0]
    fails = [r["fails"] for r in w["records"]]
    assert w["outcome"] == "stuck" and fails[-1] == threshold + 1 and max(fails[:-1], default=0) <= threshold
    if threshold >= 2:      # the two early failures were forgiven by the success that followed
        assert fails[:5] == [0, 1, 2, 0, 1] and w["iterations"] == 4 + threshold + 1
    else:
        assert w["iterations"] == 1 + threshold + 1
    # with no plan ever found the arm never moves
    res, _ = _run([_world(0, START, START + 3.0)], {0: [(False, None)]}, stop_threshold=threshold)
    w = res["worlds"][0]
    assert w["outcome"] == "stuck" and w["iterations"] == threshold + 1 and all(r["executed"] == "stay" for r in w["records"])
    assert all(np.array_equal(r["q0"], START) for r in w["records"])


def test_a_finished_world_leaves_the_batch():
    k = np.zeros(7)
    k[1] = 1.0
    near = START.copy()
    near[1] += 0.12                     # |goal - start| = 0.12: the first plan's 0.5 k_range = 0.033 brings it within pi / 30
    worlds = [_world(0, START, near), _world(1, START, START + 3.0), _world(2, START, START + 3.0)]
    res, be = _run(worlds, {0: [(True, k)], 1: [(True, k)], 2: [(False, None)]}, stop_threshold=1, max_iterations=4)
    assert [w["outcome"] for w in res["worlds"]] == ["goal", "iteration_limit", "stuck"]
    assert [w["iterations"] for w in res["worlds"]] == [1, 4, 2]
    assert be.batches == [[0, 1, 2], [1, 2], [1], [1]]
    s = res["summary"]
    assert (s["goal"], s["stuck"], s["iteration_limit"], s["collision"], s["iterations"], s["batches"]) == (1, 1, 1, 0, 7, 4)
    assert all(r["audit_verdict"] == 0 for w in res["worlds"] for r in w["records"])


def test_goal_check_wraps_angles_and_looks_at_nodes_on_the_piece():
    from armour_amd.trials import goal_reached
    goal = np.array([3.1, 0, 0, 0, 0, 0, 0.0])
    q = np.array([-3.1, 0, 0, 0, 0, 0, 0.0])                      # 0.083 rad away the short way round
    assert goal_reached(q, goal, np.pi / 30) and not goal_reached(q, goal, 0.08)
    assert not goal_reached(q + 0.05, goal, np.pi / 30)           # |(0.033, 0.05 x 6)|_2 = 0.127
    assert goal_reached(np.stack([q + 1.0, q, q - 1.0]), goal, np.pi / 30)      # any node counts
    # a world whose goal lies across the wrap: reached in the first iteration, going the short way
    k = np.zeros(7)
    k[0] = -1.0
    start = np.array([-3.1, 0.6, 0.0, 1.2, 0.0, 0.6, 0.0])
    g2 = start.copy()
    g2[0] = 3.07
    res, _ = _run([_world(0, start, g2)], {0: [(True, k)]})
    assert res["worlds"][0]["outcome"] == "goal" and res["worlds"][0]["iterations"] == 1
    assert res["worlds"][0]["records"][0]["q_des"][0] < -3.1     # the straight-line waypoint goes the short way round as well


def test_a_proved_hit_ends_the_trial_as_collision_and_undecided_does_not():
    from test_roadmap import config_clearance, geometry, link_boxes, robot_dict
    from armour_amd.planner import kinova_robot
    g = geometry(robot_dict(kinova_robot()))
    k = np.zeros(7)
    k[0] = 1.0
    c = link_boxes(g, (START + 0.25 * K_RANGE * k)[None])[2][0, 5]
    hit_box = np.array([[100.0, 0, 0, 0.01, 0, 0, 0, 0.01, 0, 0, 0, 0.01], [c[0], c[1], c[2], 0.05, 0, 0, 0, 0.05, 0, 0, 0, 0.05]])
    name, p = _world(0, START, START + 3.0)
    p["obstacles"] = hit_box
    res, _ = _run([(name, p)], {0: [(True, k)]})
    w = res["worlds"][0]
    assert w["outcome"] == "collision" and w["iterations"] == 1 and w["records"][0]["audit_verdict"] == 1
    assert 0 < w["records"][0]["t_hit"] < 0.5 and w["records"][0]["clearance"] < 0
    # a box the arm passes within the tube's reach of: undecided pieces are counted and the trial goes on
    _, R, x = link_boxes(g, START[None])
    near_box = hit_box.copy()
    for dist in np.arange(0.6, 0.0, -0.001):                    # slide a box towards the last link until it is 2 - 5 mm away
        near_box[1, 0:3] = x[0, 6] + dist * R[0, 6][:, 2]
        cl = config_clearance(g, START[None], near_box)[0]
        if cl < 0.005:
            break
    assert 0.002 < cl < 0.005, cl
    p2 = dict(p, obstacles=near_box)
    res, _ = _run([(name, p2)], {0: [(True, np.zeros(7))]}, max_iterations=3, tube=np.full(7, 0.02))
    w = res["worlds"][0]
    assert w["outcome"] == "iteration_limit" and w["undecided"] == 3 and res["summary"]["undecided_pieces"] == 3
    assert all(r["audit_verdict"] == 2 and r["clearance"] > 0 for r in w["records"])


# ----------------------------------------------------------------------------------------------------------- GPU
SOLVE = dict(tolerance=1e-7, max_iterations=100)      # tests/test_reference_scenes.py


@pytest.fixture(scope="module")
def reference_trials():
    from armour_amd import scenes
    from armour_amd.trials import run_trials
    ws = scenes.reference_worlds()
    return ws, run_trials(ws, T=100, solve_options=SOLVE, max_iterations=400, audit_step=0.01)


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_iteration_one_is_armour_solve_on_the_reference_batch(reference_trials):
    from armour_amd import scenes
    from armour_amd.planner import ArmourNLP
    ws, res = reference_trials
    bp = scenes.as_batch(ws)
    nlp = ArmourNLP(T=100).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    sols = nlp.solve(**SOLVE)
    nlp.close()
    first = [w["records"][0] for w in res["worlds"]]
    assert sum(r["feasible"] for r in first) == 107
    for b, (r, s) in enumerate(zip(first, sols)):
        assert r["feasible"] == s["feasible"] and np.array_equal(r["k_opt"], s["k_opt"]), ws[b][0]
        assert np.array_equal(r["q_des"], bp["q_des"][b])


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_no_executed_piece_of_a_whole_trial_collides(reference_trials):
    """The reference's safety claim, audited: no executed piece -- new plan or braking half -- is a proved hit, every sample clearance is
    positive, and no trial ends in a collision.  A failure here is a finding about the planner or the audit: it names world, iteration, t_hit."""
    ws, res = reference_trials
    s = res["summary"]
    print("trial summary:", {k: v for k, v in s.items()})
    bad = [(w["name"], r["iteration"], r["executed"], r["t_hit"], r["clearance"]) for w in res["worlds"] for r in w["records"]
           if r["audit_verdict"] == 1 or not r["clearance"] > 0]
    assert not bad, bad
    assert all(w["outcome"] in ("goal", "stuck", "iteration_limit") for w in res["worlds"]), [(w["name"], w["outcome"]) for w in res["worlds"]]
    assert s["collision"] == 0 and s["goal"] + s["stuck"] + s["iteration_limit"] == 107
    assert any(r["executed"] == "plan" and np.any(r["qd0"] != 0) for w in res["worlds"] for r in w["records"])


@pytest.mark.gpu
@pytest.mark.timeout(3000)
def test_moving_arm_states_against_the_live_oracle(reference_trials):
    """Up to 128 states with qd0 != 0 from the trials: tables, g, the Jacobian and the prune margin against the CPU oracle, with the helpers
    and tolerances of tests/test_reference_scenes.py (its noise-plane rule included)."""
    from armour_amd import scenes
    from armour_amd._lib import ArmourLimits
    from armour_amd.planner import ArmourNLP
    from armour_amd.trials import moving_states
    from armour_amd.worlds import random_k
    from helpers import PZ_TESTS_K
    from oracle.cpu_oracle import Oracle
    ws, res = reference_trials
    states = [s for s in moving_states(res) if np.any(s[1] != 0)]
    feasible_worlds = {w for w, wr in enumerate(res["worlds"]) if wr["records"][0]["feasible"]}
    if len(states) > 128:
        pick = np.random.default_rng(5).choice(len(states), 128, replace=False)
        states = [states[i] for i in sorted(pick)]
    else:
        assert feasible_worlds <= {s[5]["world"] for s in states}                 # at least one per feasible world
    assert len(states) >= min(128, len(feasible_worlds))
    T, O = 100, 14
    B = len(states)
    q0, qd0, qdd0, q_des = (np.stack([s[c] for s in states]) for c in range(4))
    obs = np.stack([scenes.pad_obstacles(s[4], O) for s in states])
    nlp = ArmourNLP(T=T, limits=ArmourLimits(max_batch=B, max_obstacles=O)).set_parameters(q0, qd0, qdd0, q_des, obs)
    n, J = nlp.n, nlp.J
    ks = np.stack([np.tile(PZ_TESTS_K, (B, 1)), random_k(78, B)])
    outs = [tuple(a.copy() for a in nlp.eval_g_jac(k)) for k in ks]
    tr, gens, margin = nlp.torque_radius(), nlp.link_generators(), nlp.prune_margin()
    worst = dict(coef=0.0, radius=0.0, g=0.0, jac=0.0)
    n_noise = n_flip = 0
    for b, st in enumerate(states):
        o = Oracle(T=T).set_problem(q0[b], qd0[b], qdd0[b], q_des[b], obs[b])
        om = o.min_margin()
        if om <= 1e-9:        # within rounding of a prune flip the two builds may legitimately keep different monomials (include/armour_hip.h,
            n_flip += 1       # armour_get_prune_margin): parity is defined away from it; such a state is counted, not compared
            continue
        assert margin_agrees(margin[b], om), (st[5], margin[b], om)                      # tests/test_prune_margin.py
        for which, cnt in (("link", J), ("torque", n)):
            for i in range(cnt):
                for t in range(b % 4, T, 4):
                    c, ind, keys, co = o.pz(which, i, t)
                    c2, ind2, keys2, co2 = nlp.pz(which, i, t, b=b)
                    assert np.array_equal(keys, keys2), (st[5], which, i, t)
                    if len(keys):
                        worst["coef"] = max(worst["coef"], np.abs(co - co2).max())
                    worst["coef"] = max(worst["coef"], np.abs(c - c2).max())
                    worst["radius"] = max(worst["radius"], np.abs(ind - ind2).max())
        worst["radius"] = max(worst["radius"], np.abs(tr[b] - o.torque_radius()).max())
        worst["coef"] = max(worst["coef"], np.abs(gens[b] - o.link_generators()).max())
        for s in range(2):
            gr, jr = o.eval_g_jac(ks[s, b])
            dg, dj = np.abs(outs[s][0][b] - gr), np.abs(outs[s][1][b] - jr).max(axis=1)
            off = np.nonzero((dg > G_TOL) | (dj > J_TOL))[0]
            if off.size:
                p = dict(q0=q0[b], qd0=qd0[b], qdd0=qdd0[b], q_des=q_des[b], obstacles=st[4])
                n_noise += _rows_differ_only_through_noise_planes(str(st[5]), p, o, T, O, off, ks[s, b], outs[s][0][b], gr)
                dg[off], dj[off] = 0.0, 0.0
            worst["g"], worst["jac"] = max(worst["g"], dg.max()), max(worst["jac"], dj.max())
        assert worst["coef"] <= C_TOL and worst["radius"] <= R_TOL and worst["g"] <= G_TOL and worst["jac"] <= J_TOL, (st[5], worst)
    nlp.close()
    print(f"{B} moving-arm states: worst deviations {worst}; {n_noise} row(s) decided by a noise plane; smallest device prune margin {margin.min():.3e}")
    assert n_noise <= 16 and n_flip <= 2, (n_noise, n_flip)


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_a_world_alone_gives_the_record_it_has_in_the_batch():
    from armour_amd import scenes
    from armour_amd.trials import run_trials
    ws = scenes.reference_worlds()
    kw = dict(T=100, solve_options=SOLVE, max_iterations=12, per_step_build=True)
    batch = run_trials(ws, **kw)
    for b in (3, 104):
        one = run_trials([ws[b]], **kw)["worlds"][0]
        ref = batch["worlds"][b]
        assert one["outcome"] == ref["outcome"] and one["iterations"] == ref["iterations"]
        for r1, r2 in zip(one["records"], ref["records"]):
            for key in ("q0", "qd0", "qdd0", "q_des", "k_opt"):
                assert np.array_equal(r1[key], r2[key], equal_nan=True), (b, r1["iteration"], key)
            assert (r1["feasible"], r1["executed"], r1["audit_verdict"], r1["sqp_iterations"]) == (r2["feasible"], r2["executed"], r2["audit_verdict"], r2["sqp_iterations"])
            assert r1["clearance"] == r2["clearance"]


def _saturated_iterations(d, goal_radius, nodes=10):
    """Iterations a lone joint needs to come within goal_radius of a goal d away when every plan takes k = 1 on it (a waypoint 1 rad
    ahead asks for all the plan can give), and the smallest margin by which a goal check on the way was decided."""
    from armour_amd.trials import bezier_q
    q = qd = qdd = 0.0
    margin = np.inf
    for it in range(1, 100):
        t = np.linspace(0, 0.5, nodes + 1)
        qs = bezier_q(np.array([q]), np.array([qd]), np.array([qdd]), np.array([1.0]), K_RANGE[:1], 1.0, t)[:, 0]
        margin = min(margin, np.abs(np.abs(d - qs) - goal_radius).min())
        if np.any(np.abs(d - qs) <= goal_radius):
            return it, margin
        from armour_amd.planner import desired_trajectory
        a, b, c = desired_trajectory([q], [qd], [qdd], [1.0], 0.5, k_range=K_RANGE[:1])
        q, qd, qdd = a[0], b[0], c[0]
    raise AssertionError("not reached")


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_a_short_move_in_an_empty_world_ends_at_the_goal():
    from armour_amd.trials import run_trials
    worlds, want = [], []
    for w, d in enumerate((0.13, 0.35)):
        goal = START.copy()
        goal[1] += d
        worlds.append(_world(w, START, goal, lookahead=1.0))
        it, margin = _saturated_iterations(d, np.pi / 30)
        assert margin > 1e-3, (d, margin)          # no goal check on the way is closer than 1 mrad to its radius: the count does not hang on the solver's tolerance
        want.append(it)
    assert want[0] == 1 and want[1] > 1
    res = run_trials(worlds, T=100, solve_options=SOLVE, max_iterations=20)
    assert [w["outcome"] for w in res["worlds"]] == ["goal", "goal"]
    assert [w["iterations"] for w in res["worlds"]] == want
    assert all(r["audit_verdict"] == 0 and r["feasible"] for w in res["worlds"] for r in w["records"])


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_tracked_trials_stay_within_the_ultimate_bound():
    from armour_amd import scenes
    from armour_amd.planner import kinova_robot
    from armour_amd.tracking import ultimate_bound
    from armour_amd.trials import run_trials
    ws = scenes.reference_worlds()[:8]
    res = run_trials(ws, T=100, solve_options=SOLVE, max_iterations=3, tracked=True, tube="ultimate_bound")
    _, qe, qde = ultimate_bound(kinova_robot())
    n = 0
    for w in res["worlds"]:
        for r in w["records"]:
            t = r["tracking"]
            assert t["status"] == 0 and t["limit_flags"] == 0, (w["name"], r["iteration"], t)
            assert t["max_pos_error"] <= qe and t["max_vel_error"] <= qde, (w["name"], r["iteration"], t, qe, qde)
            assert r["audit_verdict"] != 1
            n += 1
    assert n == 24
    s = res["summary"]["tracking"]
    assert s["max_pos_error"] <= s["ultimate_bound_position"] and s["limit_flags"] == 0
