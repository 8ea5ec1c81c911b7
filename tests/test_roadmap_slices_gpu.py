"""The time-sliced check and the earliest-arrival search on the device (armour_roadmap_check_slices, armour_roadmap_arrival) against their
host twins and against K window checks of the device, on the roadmaps of tests/test_roadmap_moving.py; plan_slices against its own composition
on a host handle; spacetime_hlps in whole trials."""
import numpy as np
import pytest

from test_roadmap import _robot
from test_roadmap_moving import STEP, _case, _host
from test_roadmap_slices import T0, bit, box_case, ones, search_case, slices_refusals, some_extras

pytestmark = pytest.mark.gpu

FAMILIES = ("node_slices", "edge_slices", "extra_slices")


@pytest.fixture(scope="module", params=["kinova", "fetch"])
def case(request):
    """The CPU tests' roadmap and worlds of one robot on a device handle and on a host handle"""
    from armour_amd.roadmap import Roadmap
    robot, g, nodes, edges, cont, obs, vel = _case(request.param)
    dev = Roadmap(robot, nodes, edges, continuous=cont, edge_step=STEP)
    host = _host(robot, nodes, edges, cont)
    yield dict(name=request.param, robot=robot, nodes=nodes, edges=edges, cont=cont, obs=obs, vel=vel, dev=dev, host=host)
    dev.close()
    host.close()


@pytest.mark.parametrize("K,dt", [(1, 0.3), (33, 0.05), (64, 0.03)])
def test_device_slices_equal_the_host_twin_and_k_window_checks(case, K, dt):
    dev, host, obs, vel = case["dev"], case["host"], case["obs"], case["vel"]
    xw, xa, xb = some_extras(case["nodes"], 3)
    d = dev.check_slices(obs, vel, T0, dt, K, extra_world=xw, extra_a=xa, extra_b=xb)
    h = host.check_slices(obs, vel, T0, dt, K, extra_world=xw, extra_a=xa, extra_b=xb, host=True)
    for fam in FAMILIES + ("slice_times",):
        assert np.array_equal(d[fam], h[fam]), (K, fam)
    assert d["ms"] > 0
    m = d["edge_slices"]
    assert (m != 0).any() and (m != np.uint64(ones(K))).any() and (K == 1 or ((m != 0) & (m != np.uint64(ones(K)))).any())
    t = d["slice_times"]
    for k in range(K):                                                   # the sliced launch against K launches of the window check
        v = dev.check_moving(obs, vel, t[:, k], t[:, k + 1])
        assert np.array_equal(bit(d["node_slices"], k), v["node_free"]) and np.array_equal(bit(d["edge_slices"], k), v["edge_free"]), (K, k)
    none = dev.check_slices(obs, vel, T0, dt, K, tables=False)           # Q = 0, and nothing read back
    assert none["node_slices"] is None and none["extra_slices"].size == 0


def test_three_worlds_in_one_call_equal_three_calls(case):
    dev, obs, vel = case["dev"], case["obs"], case["vel"]
    xw, xa, xb = some_extras(case["nodes"], 3)
    all_ = dev.check_slices(obs, vel, T0, 0.05, 33, extra_world=xw, extra_a=xa, extra_b=xb)
    for w in range(3):
        mine = xw == w
        one = dev.check_slices(obs[w], vel[w], T0[w], 0.05, 33, extra_world=np.zeros(int(mine.sum()), dtype=np.int32), extra_a=xa[mine], extra_b=xb[mine])
        assert np.array_equal(one["node_slices"][0], all_["node_slices"][w]) and np.array_equal(one["edge_slices"][0], all_["edge_slices"][w])
        assert np.array_equal(one["extra_slices"], all_["extra_slices"][mine]) and np.array_equal(one["slice_times"][0], all_["slice_times"][w])


@pytest.mark.parametrize("O", [1, 256])
def test_one_obstacle_and_the_obstacle_cap(O):
    """O = ARMOUR_ROADMAP_MAX_OBSTACLES with K = 64: 62 KB of obstacles and 1 KB of slice times in LDS, on 8 nodes"""
    from armour_amd.roadmap import Roadmap
    from armour_amd.scenes import boxes_to_obstacles
    from test_moving_audit import random_motion
    from test_roadmap_moving import make_roadmap
    robot = _robot("kinova")
    nodes, edges, cont = make_roadmap(robot, N=8)
    rng = np.random.default_rng(8)
    boxes = np.concatenate([rng.uniform([-1.5, -1.5, 0.0], [1.5, 1.5, 1.5], (O, 3)), rng.uniform(0.02, 0.06, (O, 3))], axis=1)
    if O == 1:
        boxes[0, :3] = [0.5, 0.0, 0.6]
    obs = boxes_to_obstacles(boxes)[None]
    vel = random_motion(rng, obs, lo=0.05, hi=0.2)
    if O == 256:
        vel[0, ::3] = 0.0                                                # boxes at rest among the moving ones: the one-test branch
    dev, host = Roadmap(robot, nodes, edges, continuous=cont, edge_step=STEP), _host(robot, nodes, edges, cont)
    xw, xa, xb = some_extras(nodes, 1)
    a = dev.check_slices(obs, vel, 0.0, 0.05, 64, extra_world=xw, extra_a=xa, extra_b=xb)
    b = host.check_slices(obs, vel, 0.0, 0.05, 64, extra_world=xw, extra_a=xa, extra_b=xb, host=True)
    for fam in FAMILIES:
        assert np.array_equal(a[fam], b[fam]), (O, fam)
    dev.close()
    host.close()


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("K,dt,step_len", [(5, 0.2, 2.0), (64, 0.03, 0.25)])
def test_device_arrival_equals_the_host_twin(case, W, K, dt, step_len):
    obs, vel = case["obs"][:W], case["vel"][:W] * 0.5
    _, d, *_ = search_case(case["dev"], obs, vel, T0[:W], dt, K, step_len, host=False)
    _, h, *_ = search_case(case["host"], obs, vel, T0[:W], dt, K, step_len, host=True)
    for key in ("reach", "goal_slice", "path_len", "path_node", "path_slice"):
        assert np.array_equal(d[key], h[key]), (W, K, key)
    assert ((1 <= d["sweeps"]) & (d["sweeps"] <= K + 1)).all() and d["ms"] > 0
    assert K == 5 or (d["goal_slice"] >= 0).any()                        # (tests/test_roadmap_slices.py prints the same worlds' goal slices)


def test_the_arriving_box_on_the_device():
    rm, s, a, _ = box_case(host=False, moving=True)
    rm.close()
    rm, sh, ah, _ = box_case(host=True, moving=True)
    rm.close()
    for fam in FAMILIES:
        assert np.array_equal(s[fam], sh[fam]), fam
    for key in ("reach", "goal_slice", "path_len", "path_node", "path_slice"):
        assert np.array_equal(a[key], ah[key]), key
    assert a["goal_slice"][0] > 12 and a["path_slice"][0, 0] > 0


def test_a_sliced_check_and_a_search_leave_descend_alone(case):
    dev, obs, vel = case["dev"], case["obs"], case["vel"] * 0.25
    rng = np.random.default_rng(5)
    nodes = case["nodes"]
    world = (np.arange(18) % 3).astype(np.int32)
    starts = nodes[rng.integers(0, nodes.shape[0], 18)] + rng.normal(scale=0.05, size=(18, nodes.shape[1]))
    goals = nodes[rng.integers(0, nodes.shape[0], 3)] + rng.normal(scale=0.05, size=(3, nodes.shape[1]))
    dev.check_moving(obs, vel, T0, T0 + 0.2)
    dev.field(goals, connect_k=6)
    before = dev.descend_many(world, starts, connect_k=6)
    search_case(dev, obs, case["vel"], T0 + 3.0, 0.03, 64, 0.25, host=False)
    after = dev.descend_many(world, starts, connect_k=6)
    assert sum(p is not None for p, _ in before) >= 3
    for (pa, la), (pb, lb) in zip(before, after):
        assert np.float64(la).tobytes() == np.float64(lb).tobytes() and ((pa is None and pb is None) or pa.tobytes() == pb.tobytes())


def test_plan_slices_equals_its_composition_on_the_host_handle(case):
    dev, host, obs, vel, nodes = case["dev"], case["host"], case["obs"], case["vel"] * 0.25, case["nodes"]
    rng = np.random.default_rng(4)
    starts, goals = nodes[[3, 17, 30]] + rng.uniform(-0.1, 0.1, (3, nodes.shape[1])), nodes[[41, 8, 22]] + rng.uniform(-0.1, 0.1, (3, nodes.shape[1]))
    d = dev.plan_slices(starts, goals, obs, vel, T0, 0.1, 64, speed=5.0, connect_k=4)
    h = host.plan_slices(starts, goals, obs, vel, T0, 0.1, 64, speed=5.0, connect_k=4, host=True)
    assert np.array_equal(dev.last_slices["extra_slices"], host.last_slices["extra_slices"])
    for pd, ph in zip(d, h):
        assert pd["goal_slice"] == ph["goal_slice"] and (pd["path"] is None) == (ph["path"] is None)
        if pd["path"] is not None:
            assert all(np.array_equal(pd[key], ph[key]) for key in ("path", "node", "slice", "time"))
    assert any(p["path"] is not None for p in d)


def test_device_entries_refuse_what_the_host_entries_refuse(case):
    from armour_amd import _lib
    dev = case["dev"]
    slices_refusals(dev, host=False)
    with pytest.raises(_lib.ArmourError) as ei:                              # the host twins take handles of armour_roadmap_create_host only
        dev.check_slices(case["obs"], case["vel"], T0, 0.1, 4, host=True)
    assert ei.value.code == _lib.EINVAL
    dev.check_slices(case["obs"], case["vel"], T0, 0.1, 4)
    with pytest.raises(_lib.ArmourError) as ei:
        dev.arrival(0.5, 0, 0, host=True)
    assert ei.value.code == _lib.EINVAL
    dev.check_self()
    dev.use_self(True)
    try:
        with pytest.raises(_lib.ArmourError) as ei:                          # the self masks are not part of the space-time search
            dev.arrival(0.5, 0, 0)
        assert ei.value.code == _lib.ESTATE
    finally:
        dev.use_self(False)
    assert dev.arrival(0.5, 0, 0)["goal_slice"].tolist() == [-1, -1, -1]     # no extra edge joins start or goal to anything


# ----------------------------------------------------------------------------------------------------------- whole trials
def test_spacetime_hlps_in_whole_trials():
    """Two reference worlds, at most 6 iterations: no `plan` or `brake` piece is a proved hit of the moving audit, and the planner's slices
    begin at the worlds' clocks."""
    from armour_amd import scenes
    from armour_amd.roadmap import spacetime_hlps
    from armour_amd.trials import run_trials
    from test_trials_moving import GPU_SEED, SOLVE, _trial_roadmap, seeded_velocities
    picks = (48, 54)
    all_ws = scenes.reference_worlds()
    ws = [all_ws[i] for i in picks]
    vel = seeded_velocities(ws, picks, GPU_SEED)
    rm = _trial_roadmap()
    make = spacetime_hlps(rm, ws, vel, speed=1.0, dt=0.25, K=32, connect_k=8)
    clocks = []
    inner = make.get_waypoints

    def recording(indices, qs, lookaheads):
        out = inner(indices, qs, lookaheads)
        clocks.append((make.last_check["slice_times"].copy(), [p["goal_slice"] for p in make.last_plans]))
        return out

    make.get_waypoints = recording
    res = run_trials(ws, hlp=make, velocities=vel, T=64, solve_options=SOLVE, max_iterations=6, per_step_build=True)
    rm.close()
    recs = [(w, r) for w in res["worlds"] for r in w["records"]]
    print({k: v for k, v in res["summary"].items() if "_ms" not in k}, [w["outcome"] for w in res["worlds"]], [g for _, g in clocks])
    bad = [(w["name"], r["iteration"], r["executed"], r["t_hit"]) for w, r in recs if r["executed"] in ("plan", "brake") and r["audit_verdict"] == 1]
    assert not bad, bad
    assert res["summary"]["collision"] == 0 and sum(r["feasible"] for _, r in recs) >= 2
    assert len(clocks) >= 2
    for it, (times, _) in enumerate(clocks):                             # iteration `it` of a live world planned at that world's clock
        assert times.shape == (2, 33)
        for b, w in enumerate(res["worlds"]):
            if it < len(w["records"]):
                assert times[b, 0] == w["records"][it]["t_world"], (it, b)
    assert any(any(t[:, 0] > 0) for t, _ in clocks)                      # the clocks moved
