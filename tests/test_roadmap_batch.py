"""Queries joined to a checked roadmap in one call (include/armour_hip.h armour_roadmap_connect_batch / armour_roadmap_descend_batch,
Roadmap.connect_many / descend_many, field_hlps(batched=True)) and the trials' one waypoint call per iteration.

CPU: run_trials with a scripted backend and a scripted factory that offers get_waypoints.  GPU: connect_many against the numpy search of
test_roadmap_knn.py and the numpy edge rules of test_roadmap.py / test_self_check.py, descend_many against descend query for query, and
whole trials with and without `batched`."""
import numpy as np
import pytest

from test_roadmap import _limits, _reference_obstacles, _robot, config_clearance, edge_free_np, geometry, robot_dict
from test_roadmap_knn import knn_np
from test_trials import START, ScriptedPlanner, _world

SOLVE = dict(tolerance=1e-7, max_iterations=100)      # tests/test_reference_scenes.py


# ----------------------------------------------------------------------------------------------------------- CPU
class _ScriptedHLP:
    """A waypoint that depends on the world, the state and the lookahead, so that a waypoint given to the wrong world shows."""

    def __init__(self, i):
        self.i = i

    def get_waypoint(self, q_cur, lookahead):
        return None if self.i == 2 else q_cur + 0.01 * (self.i + 1) * lookahead


def test_run_trials_asks_a_batched_factory_once_per_iteration():
    from armour_amd.trials import run_trials
    k = np.zeros(7)
    k[1] = 1.0
    near = START.copy()
    near[1] += 0.12
    worlds = [_world(0, START, near), _world(1, START, START + 3.0, lookahead=0.5), _world(2, START, START + 3.0)]
    scripts = {0: [(True, k)], 1: [(True, k)], 2: [(False, None)]}
    calls = []

    def per_world(i, world):
        return _ScriptedHLP(i)

    def batched(i, world):
        return _ScriptedHLP(i)

    def get_waypoints(indices, qs, lookaheads):
        calls.append((list(indices), [q.copy() for q in qs], list(lookaheads)))
        return [_ScriptedHLP(i).get_waypoint(q, la) for i, q, la in zip(indices, qs, lookaheads)]

    batched.get_waypoints = get_waypoints
    res = {}
    for name, hlp in (("loop", per_world), ("batched", batched)):
        be = ScriptedPlanner(scripts)
        res[name] = run_trials(worlds, backend=be, audit_on_host=True, hlp=hlp, stop_threshold=1, max_iterations=4)
        assert be.batches == [[0, 1, 2], [1, 2], [1], [1]]
    assert [c[0] for c in calls] == [[0, 1, 2], [1, 2], [1], [1]]                    # one call per iteration, the live worlds
    assert [c[2] for c in calls] == [[1.0, 0.5, 1.0], [0.5, 1.0], [0.5], [0.5]]
    for wa, wb in zip(res["loop"]["worlds"], res["batched"]["worlds"]):
        assert wa["outcome"] == wb["outcome"] and len(wa["records"]) == len(wb["records"])
        for ra, rb in zip(wa["records"], wb["records"]):
            assert np.array_equal(ra["q_des"], rb["q_des"]) and np.array_equal(ra["q0"], rb["q0"])
    recs = res["batched"]["worlds"]
    assert np.array_equal(recs[1]["records"][0]["q_des"], START + 0.01 * 2 * 0.5)    # world 1's own rule and lookahead
    assert np.array_equal(recs[2]["records"][0]["q_des"], START + 3.0)               # no waypoint: the goal
    for it, (_, qs, _) in enumerate(calls):                                          # the states handed over are the records' q0
        live = [w for w in recs if len(w["records"]) > it]
        assert all(np.array_equal(q, w["records"][it]["q0"]) for q, w in zip(qs, live))
    for r in res.values():
        assert len(r["batches"]) == 4 and all("hlp_ms" in b and b["hlp_ms"] >= 0.0 for b in r["batches"])


# ----------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def setup():
    """The 800-node roadmap of test_roadmap_field.py's parity test, the first 17 reference worlds with their goals, 61 starts free in
    their worlds, and the calibrated self table."""
    from armour_amd.roadmap import Roadmap, uniform_roadmap
    from armour_amd.scenes import reference_worlds
    from armour_amd.self_check import calibrate_shrink
    from test_self_check import _reference_configs
    robot = _robot("kinova")
    g, (lb, ub, cont) = geometry(robot_dict(robot)), _limits(robot)
    step = 0.1
    nodes, edges = uniform_roadmap(800, 2.5, 4, 5, lb, ub, cont)
    rm = Roadmap(robot, nodes, edges, continuous=cont, edge_step=step)
    ws = reference_worlds()[:17]
    obs = _reference_obstacles()["obstacles"][:17]
    goals = np.stack([np.asarray(p["goal"], dtype=np.float64) for _, p in ws])
    rng = np.random.default_rng(12)
    world, starts = [], []
    while len(starts) < 61:
        w = len(starts) % 17
        q = lb + (ub - lb) * rng.random(7)
        if config_clearance(g, q[None], obs[w])[0] > 1e-6:
            world.append(w)
            starts.append(q)
    shrink = calibrate_shrink(robot, _reference_configs(), host=True)
    yield dict(robot=robot, g=g, cont=cont, step=step, rm=rm, nodes=nodes, ws=ws, obs=obs, goals=goals, world=np.array(world, dtype=np.int32),
               starts=np.stack(starts), shrink=shrink)
    rm.close()


def _masks(s, self_on):
    """check + (self check, use_self) -> free [W,N] as the searches read it, and the self edge rule (None when off)"""
    rm = s["rm"]
    v = rm.check(s["obs"])
    rm.use_self(False)
    if not self_on:
        return v["node_free"], None
    from test_self_check import edge_self_free_np
    sv = rm.check_self(shrink=s["shrink"])
    rm.use_self(True)
    return v["node_free"] & sv["node_free"], lambda a, b: edge_self_free_np(s["g"], a, b, s["step"], shrink=s["shrink"])


@pytest.mark.gpu
@pytest.mark.parametrize("self_on", [False, True])
def test_connect_many_against_the_numpy_search_and_edge_rules(setup, self_on):
    s = setup
    rm, g, world, starts, step = s["rm"], s["g"], s["world"], s["starts"], s["step"]
    free, self_rule = _masks(s, self_on)
    got = rm.connect_many(world, starts, targets=s["goals"][world], connect_k=8)
    want = knn_np(s["nodes"], starts, s["cont"], 8, free=free[world])
    assert np.array_equal(got["node"], want[0]) and np.array_equal(got["dist"], want[1]) and np.array_equal(got["count"], want[2])
    assert (got["count"] == 8).all()

    def rule(a, b, w):
        ok, cl = edge_free_np(g, a, b, s["obs"][w], step)
        assert abs(cl) > 1e-9, cl                                      # no edge so close to an obstacle that rounding decides it
        if ok and self_rule is not None:
            ok, margin = self_rule(a, b)
            assert abs(margin) > 1e-9, margin
        return ok

    for i in range(61):
        w = world[i]
        assert got["direct"][i] == rule(starts[i], s["goals"][w], w), i
        for c in range(8):
            assert got["edge_ok"][i, c] == rule(starts[i], s["nodes"][got["node"][i, c]], w), (i, c)
    assert 0 < got["edge_ok"].sum() < got["edge_ok"].size
    # without targets there is no `direct`, and the rest is the same; connect_k = 0 joins nothing
    again = rm.connect_many(world, starts, connect_k=8)
    assert "direct" not in again and all(np.array_equal(again[key], got[key]) for key in ("node", "dist", "edge_ok", "count"))
    none = rm.connect_many(world, starts, targets=s["goals"][world], connect_k=0)
    assert none["node"].shape == (61, 0) and (none["count"] == 0).all() and np.array_equal(none["direct"], got["direct"])
    rm.use_self(False)


@pytest.mark.gpu
@pytest.mark.parametrize("self_on", [False, True])
def test_descend_many_equals_descend(setup, self_on):
    from armour_amd import _lib
    s = setup
    rm, world, starts = s["rm"], s["world"], s["starts"]
    _masks(s, self_on)
    rm.field(s["goals"], connect_k=8)
    got = rm.descend_many(world, starts, connect_k=8)
    kinds = {"none": 0, "direct": 0, "nodes": 0}
    for i in range(61):
        path, length = rm.descend(int(world[i]), starts[i], connect_k=8)
        assert (path is None) == (got[i][0] is None), i
        assert np.float64(length).tobytes() == np.float64(got[i][1]).tobytes(), (i, length, got[i][1])
        if path is None:
            kinds["none"] += 1
            assert got[i][1] == np.inf
            continue
        assert np.array_equal(path, got[i][0]), i
        kinds["direct" if len(path) == 2 else "nodes"] += 1
    assert kinds["direct"] > 0 and kinds["nodes"] > 0, kinds           # the comparison is not of one kind of answer alone
    # too little room for the node sequences: ECAPACITY, and the offsets say how much is needed
    with pytest.raises(_lib.ArmourError) as ei:
        rm.descend_many(world, starts, connect_k=8, seq_capacity=0)
    assert ei.value.code == _lib.ECAPACITY
    need = sum(len(p) - 2 for p, _ in got if p is not None)
    exact = rm.descend_many(world, starts, connect_k=8, seq_capacity=need)
    assert all((a[0] is None and b[0] is None) or np.array_equal(a[0], b[0]) for a, b in zip(exact, got))
    with pytest.raises(_lib.ArmourError) as ei:
        rm.descend_many(world, starts, connect_k=8, seq_capacity=need - 1)
    assert ei.value.code == _lib.ECAPACITY
    with pytest.raises(_lib.ArmourError) as ei:
        rm.descend_many([17], starts[:1])
    assert ei.value.code == _lib.EINVAL
    # a new check ends the field
    rm.check(s["obs"])
    with pytest.raises(_lib.ArmourError) as ei:
        rm.descend_many(world, starts)
    assert ei.value.code == _lib.ESTATE
    rm.use_self(False)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_trials_with_one_waypoint_call_per_iteration_equal_the_per_world_loop(setup):
    from armour_amd.roadmap import field_hlps
    from armour_amd.trials import run_trials
    s = setup
    rm, worlds = s["rm"], s["ws"][:8]
    rm.use_self(False)
    res = {}
    for batched in (False, True):
        make = field_hlps(rm, worlds, connect_k=8, batched=batched)
        assert hasattr(make, "get_waypoints") == batched
        res[batched] = run_trials(worlds, hlp=make, T=64, solve_options=SOLVE, max_iterations=6)
    records = 0
    for wa, wb in zip(res[False]["worlds"], res[True]["worlds"]):
        assert wa["outcome"] == wb["outcome"] and len(wa["records"]) == len(wb["records"]), wa["name"]
        for ra, rb in zip(wa["records"], wb["records"]):
            assert np.array_equal(ra["q_des"], rb["q_des"]) and np.array_equal(ra["q0"], rb["q0"]), (wa["name"], ra["iteration"])
            assert ra["feasible"] == rb["feasible"] and ra["executed"] == rb["executed"]
            records += 1
    assert records >= 8
    assert all("hlp_ms" in b for r in res.values() for b in r["batches"])
