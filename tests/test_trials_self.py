"""run_trials(self_check=...) (armour_amd/trials.py): the executed pieces audited against the arm itself.

CPU: the wiring with a scripted planner backend (the pattern of tests/test_trials.py).  GPU: one short run on reference worlds."""
import numpy as np
import pytest

K_RANGE = np.full(7, np.pi / 48)
START = np.array([0.0, 0.6, 0.0, 1.2, 0.0, 0.6, 0.0])
NEAR_FOLD = np.array([0.0, 2.1, 0.0, 2.5, 0.0, 0.69, 0.0])      # self-free by 3 mm; joint 6 past 0.712 and the last link is inside the first


class ScriptedPlanner:
    """plan() answers from a script per world: script[w] = list of (feasible, k) per planning iteration of that world (the last entry
    repeats).  A world is recognised by the x coordinate of its (far) obstacle, 100 + w."""

    def __init__(self, scripts):
        from armour_amd.planner import kinova_robot
        self.robot, self.k_range, self.duration, self.t_plan = kinova_robot(), K_RANGE, 1.0, 0.5
        self.scripts, self.calls = scripts, {w: 0 for w in scripts}

    def plan(self, q0, qd0, qdd0, q_des, obstacles):
        out = []
        for w in [int(round(o[0, 0])) - 100 for o in obstacles]:
            sc = self.scripts[w]
            feasible, k = sc[min(self.calls[w], len(sc) - 1)]
            self.calls[w] += 1
            out.append(dict(k_opt=np.asarray(k, dtype=np.float64) if feasible else np.full(7, np.nan), feasible=feasible, iterations=3, time_ms=0.1))
        return out, 1.0, 2.0


def _world(w, start, goal):
    far = np.array([[100.0 + w, 0, 0, 0.01, 0, 0, 0, 0.01, 0, 0, 0, 0.01]])
    return (f"w{w}", dict(q0=np.asarray(start, dtype=np.float64), goal=np.asarray(goal, dtype=np.float64), obstacles=far, lookahead=1.0))


def _run(worlds, scripts, **kw):
    from armour_amd.trials import run_trials
    return run_trials(worlds, backend=ScriptedPlanner(scripts), audit_on_host=True, **kw)


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b, equal_nan=True)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and np.isnan(a):
        return isinstance(b, float) and np.isnan(b)
    return a == b


def _scripts():
    fold = np.zeros(7)
    fold[5] = 1.0                                  # joint 6 on: 0.69 -> 0.69 + pi/48 = 0.755 at the plan's end
    k = np.full(7, 0.5)
    return [_world(0, START, START + 3.0), _world(1, NEAR_FOLD, NEAR_FOLD + 1.0)], {0: [(True, k), (False, None)], 1: [(True, fold)]}


def test_none_changes_nothing_and_record_adds_fields_only():
    worlds, scripts = _scripts()
    base = _run(worlds, scripts, max_iterations=4)
    none = _run(worlds, scripts, max_iterations=4, self_check=None)
    rec = _run(worlds, scripts, max_iterations=4, self_check="record")
    assert set(none["summary"]) == set(base["summary"])
    added = {"self_verdict", "self_t_hit", "self_clearance"}
    for wb, wn, wr in zip(base["worlds"], none["worlds"], rec["worlds"]):
        assert wb["outcome"] == wn["outcome"] == wr["outcome"] and len(wb["records"]) == len(wn["records"]) == len(wr["records"])
        for rb, rn, rr in zip(wb["records"], wn["records"], wr["records"]):
            assert set(rn) == set(rb) and set(rr) == set(rb) | added
            assert all(_same(rb[key], rn[key]) and _same(rb[key], rr[key]) for key in rb if key not in ("build_ms", "solve_ms"))
    assert set(rec["summary"]) == set(base["summary"]) | {"self_hit_pieces", "self_undecided_pieces"}
    v0 = [r["self_verdict"] for r in rec["worlds"][0]["records"]]
    v1 = [r["self_verdict"] for r in rec["worlds"][1]["records"]]
    assert set(v0) <= {0, 2} and 1 in v1                         # the fold is recorded, and nothing stops on it
    assert rec["worlds"][1]["outcome"] != "self_collision" and rec["summary"]["self_hit_pieces"] == v1.count(1)
    hit = rec["worlds"][1]["records"][v1.index(1)]
    assert hit["self_clearance"] < 0 and 0 <= hit["self_t_hit"] <= 0.5


def test_stop_ends_the_world_at_the_self_hitting_piece():
    from armour_amd.trials import SELF_OUTCOME
    worlds, scripts = _scripts()
    rec = _run(worlds, scripts, max_iterations=4, self_check="record")
    res = _run(worlds, scripts, max_iterations=4, self_check="stop")
    v1 = [r["self_verdict"] for r in rec["worlds"][1]["records"]]
    w = res["worlds"][1]
    assert w["outcome"] == SELF_OUTCOME == "self_collision" and w["iterations"] == v1.index(1) + 1 and w["records"][-1]["self_verdict"] == 1
    assert res["worlds"][0]["outcome"] == rec["worlds"][0]["outcome"] and res["summary"]["self_collision"] == 1
    with pytest.raises(ValueError):
        _run(worlds, scripts, self_check="halt")


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_record_leaves_the_outcomes_of_reference_worlds_alone():
    from armour_amd import scenes
    from armour_amd.self_check import calibrate_shrink
    from armour_amd.trials import run_trials
    worlds = scenes.reference_worlds()[:4]
    kw = dict(T=40, max_iterations=6, per_step_build=True, solve_options=dict(tolerance=1e-7, max_iterations=100))
    base = run_trials(worlds, **kw)
    Q = np.stack([p["q0"] for _, p in scenes.reference_worlds()] + [p["goal"] for _, p in scenes.reference_worlds()])
    from armour_amd.planner import kinova_robot
    rec = run_trials(worlds, self_check="record", self_shrink=calibrate_shrink(kinova_robot(), Q, host=True), **kw)
    assert [w["outcome"] for w in rec["worlds"]] == [w["outcome"] for w in base["worlds"]]
    assert [w["iterations"] for w in rec["worlds"]] == [w["iterations"] for w in base["worlds"]]
    for key in ("goal", "collision", "stuck", "iteration_limit"):
        assert rec["summary"][key] == base["summary"][key]
    sv = [r["self_verdict"] for w in rec["worlds"] for r in w["records"]]
    print(f"self verdicts of {len(sv)} executed pieces: {np.bincount(sv, minlength=3).tolist()}")
    assert all(v in (0, 1, 2) for v in sv) and rec["summary"]["self_hit_pieces"] == sv.count(1)
