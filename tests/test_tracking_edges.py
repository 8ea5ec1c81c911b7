"""armour_track where it turns numbers into a verdict: the limit monitors, the stop paths and their neighbours, ragged time grids, the
edges of a 64-lane block, and the whole thing in the 8-factor ABI (libarmour_hip_k128.so) -- test_tracking.py holds the numeric core.

Everything is compared with test_tracking.host_track through its _compare (1e-9; flags, steps, t_end and first_violation_t exactly).  A
flag is asserted on the device only where the restatement says how far the monitored value is from the limit at EVERY node (its
`margins`): the limits are placed half-way between two nodes of a recorded restatement trace and every margin must be >= MARGIN = 1e-6,
1000 x the parity tolerance.  Passive-plant runs and runs on Fetch presets first show their conditioning on the restatement alone
(_well_conditioned): 1e-9 would otherwise test the growth of a rounding error and not the kernel.  The Fetch presets' own V_m = 1e-7 makes
the robust rule chatter at dt = 1e-3, so those runs pass V_max = 1e-2.

Not covered: status 1 (nominal torque outside the interval torque) -- the interval model encloses the nominal one by construction and no
state reaches it.

Seen on one MI355X (largest |device - restatement| over states, maxima and traces; every test prints its own, -s shows them):
  limit calls 1.1e-14 each (flags [7,3,7,5,5,5], [1,7,5,1,5,5], [4,7,7,0,5,5]; margins on the restatement: 6.7e-5 speed, 1.9e-4 position,
  1.2e-3 torque), zero torque limit 1.1e-14 (ratios 0.14 .. 0.36), limits crossed from below 5.7e-14 (flags [6,0,4]); stops 1.7e-18 (passive
  plant), 8.7e-19 (robust, nominal); ragged grid 7.1e-15, the 1e-9 rule's two sides and the last-bit grid <= 5.6e-17; B = 130 passive 6.9e-18,
  B = 65 robust 8.9e-16; 8-factor ABI: Kinova robust 8.9e-15, fetch8 nominal and robust 1.4e-14, the Kinova rollouts' bits EQUAL to the
  7-factor library's in every field and trace entry.  Nothing is above 1e-11; the tolerance stays the project's 1e-9 for this kernel.
  Conditioning on the restatement (z0 (1 + 1e-13)): <= 1.5e-13 at the end of the 8-factor ABI's rollouts (asserted everywhere: <= 1e-11).
Every one of the nine kernel mutations listed in DESIGN 7.1 fails between 1 and 10 of the 16 device tests here.
"""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from armour_amd import _lib
from test_tracking import N_J, _compare, _plans, _reference, _robot, _same_bits, _start_inside, host_track, with_limits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_RANGE = np.full(N_J, np.pi / 48)
MARGIN = 1e-6
FIELDS = ("status", "steps", "limit_flags", "t_end", "q", "qd", "max_pos_error", "max_vel_error", "max_V", "max_robust_input", "max_torque_ratio",
          "first_violation_t", "trace")
TORQUE, POSITION, SPEED = _lib.TRACK_LIMIT_TORQUE, _lib.TRACK_LIMIT_POSITION, _lib.TRACK_LIMIT_SPEED


def _simulate(*a, **kw):
    from armour_amd.tracking import simulate_tracking
    return simulate_tracking(*a, **kw)


def _bit_equal(a, b, lane_a, lane_b, fields=FIELDS):
    for name in fields:
        x, y = getattr(a, name), getattr(b, name)
        if x is None and y is None:
            continue
        assert np.array_equal(np.asarray(x[lane_a]), np.asarray(y[lane_b]), equal_nan=True), (name, lane_a, lane_b)


def _well_conditioned(run_of, z0):
    """The conditioning guard: the restatement from z0 (1 + 1e-13) must end within 1e-11 of the restatement from z0.  Returns the base run."""
    base, moved = run_of(z0), run_of(z0 * (1 + 1e-13))
    growth = max(np.abs(base["q"] - moved["q"]).max(), np.abs(base["qd"] - moved["qd"]).max())
    assert base["status"] == moved["status"] == 0 and growth <= 1e-11, growth
    return base


# ------------------------------------------------------------------------------------------------ 1. limit monitors
@functools.lru_cache(maxsize=None)
def _limit_runs():
    """Six robust rollouts of 60 steps on uncertain plants, started inside the bound, restated once with the default robot and every node kept."""
    from armour_amd.tracking import plant_samples
    rb = _robot()
    rng = np.random.default_rng(21)
    B, D = 6, 1.0
    q0, qd0, qdd0, k = _plans(rng, B)
    sm, sI = plant_samples(rb, B, rb.mass_uncertainty, rng)
    z0 = _start_inside(rb, rng, q0, qd0, qdd0, k, K_RANGE, D, sm, sI)
    kw = dict(t1=0.06, dt=1e-3, controller="robust", record_every=1)
    host = [host_track(rb, q0[b], qd0[b], qdd0[b], k[b], K_RANGE, D, sm=sm[b], sI=sI[b], z0=z0[b], **kw) for b in range(B)]
    assert all(h["status"] == 0 and h["steps"] == 60 and h["limit_flags"] == 0 for h in host)
    return dict(args=(q0, qd0, qdd0, k, K_RANGE, D), kw=dict(kw, z0=z0, mass_scale=sm, inertia_scale=sI), host=host)


WINDOWS = ((3, 19), (22, 38), (41, 57))   # the nodes of the first, second and third crossing of a call


def _crossings(values, window, joints):
    """Per joint at most one (joint, node m, limit): the node in `window` nearest its middle at which |value| exceeds its running maximum,
    and the limit half-way between that maximum and |value[m]| -- so the joint first crosses the limit at node m exactly."""
    out = []
    mid = 0.5 * (window[0] + window[1])
    a = np.abs(values)
    for j in joints:
        run = np.maximum.accumulate(a[:, j])
        ms = [m for m in range(window[0], window[1] + 1) if a[m, j] > run[m - 1]]
        if ms:
            m = min(ms, key=lambda x: (abs(x - mid), x))
            out.append((j, m, 0.5 * (run[m - 1] + a[m, j])))
    return out


def _limited_robot(speed=None, position=None, torque=None, zero_torque=None):
    rb = _robot()
    if speed:
        rb.speed_limits[speed[0]] = speed[2]
    if position:
        rb.state_limits_lb[position[0]], rb.state_limits_ub[position[0]] = -position[2], position[2]
    if torque:
        rb.torque_limits[torque[0]] = torque[2]
    if zero_torque is not None:
        rb.torque_limits[zero_torque] = 0.0
    return rb


def _conditions(runs, src):
    """What the issue asks of a call before the device is looked at: margins, the source rollout's flags 7 at an interior node, three flag words."""
    margin = min(min(r["margins"].values()) for r in runs)
    words = {r["limit_flags"] for r in runs}
    t = runs[src]["first_violation_t"]
    return margin >= MARGIN and runs[src]["limit_flags"] == 7 and 0.0 < t < runs[src]["t_end"] and len(words) >= 3


@functools.lru_cache(maxsize=None)
def _limit_call(first):
    """The call whose earliest crossing is of quantity `first`: limits from rollout SOURCE[first]'s trace, one joint per quantity, the three
    crossing nodes in the three WINDOWS.  The speed joint is never joint 0 (a monitor reading joint 0's limit for every joint must show).
    The first combination of joints (in index order) that meets _conditions is taken."""
    setup = _limit_runs()
    src = {"speed": 0, "position": 1, "torque": 2}[first]
    order = {"speed": ("speed", "position", "torque"), "position": ("position", "torque", "speed"), "torque": ("torque", "speed", "position")}[first]
    nodes = setup["host"][src]["nodes"]
    series = dict(position=np.array([nd[1] for nd in nodes]), speed=np.array([nd[2] for nd in nodes]), torque=np.array([nd[3] for nd in nodes]))
    cands = {q: _crossings(series[q], WINDOWS[order.index(q)], range(1, N_J) if q == "speed" else range(N_J)) for q in order}
    for s, p, t in itertools.product(cands["speed"], cands["position"], cands["torque"]):
        rb = _limited_robot(speed=s, position=p, torque=t)
        runs = [with_limits(h, rb) for h in setup["host"]]
        if _conditions(runs, src):
            return dict(robot=rb, runs=runs, src=src, chosen=dict(speed=s, position=p, torque=t), order=order)
    raise AssertionError(f"no placement of limits from rollout {src} meets the conditions")


def test_limits_placed_between_nodes_flag_the_restatement():
    """CPU ground of the limit tests: each of the three calls meets the conditions, its crossings come in the intended order, and limits
    change no state."""
    setup = _limit_runs()
    for first in ("speed", "position", "torque"):
        call = _limit_call(first)
        runs, src, ch = call["runs"], call["src"], call["chosen"]
        assert _conditions(runs, src)
        assert min(min(r["margins"].values()) for r in runs) >= MARGIN
        m = {q: ch[q][1] for q in ch}
        assert len(set(m.values())) == 3 and min(m, key=m.get) == first and all(v >= 1 for v in m.values())
        assert runs[src]["first_violation_t"] == m[first] * runs[src]["h"]
        for r, h in zip(runs, setup["host"]):
            assert r["q"] is h["q"] and r["nodes"] is h["nodes"]
        print(f"{first} first: rollout {src}, (joint, node, limit) {ch}, flags {[r['limit_flags'] for r in runs]}, "
              f"margins {min(r['margins']['position'] for r in runs):.1e} (position) {min(r['margins']['speed'] for r in runs):.1e} (speed) "
              f"{min(r['margins']['torque'] for r in runs):.1e} (torque)")


ZERO_TORQUE_JOINT = 1


def test_a_zero_torque_limit_flags_and_gives_no_ratio_on_the_restatement():
    setup = _limit_runs()
    runs = [with_limits(h, _limited_robot(zero_torque=ZERO_TORQUE_JOINT)) for h in setup["host"]]
    for r, h in zip(runs, setup["host"]):
        u = np.array([nd[3][ZERO_TORQUE_JOINT] for nd in r["nodes"]])
        first = int(np.flatnonzero(u != 0)[0])
        assert r["limit_flags"] == TORQUE and r["first_violation_t"] == r["nodes"][first][0]
        assert np.isfinite(r["max_torque_ratio"]) and 0 < r["max_torque_ratio"] <= h["max_torque_ratio"]
        assert r["margins"]["torque"] >= MARGIN


@pytest.mark.gpu
@pytest.mark.parametrize("first", ["speed", "position", "torque"])
def test_device_limit_monitors_equal_the_restatement(first):
    setup, call = _limit_runs(), _limit_call(first)
    assert _conditions(call["runs"], call["src"])
    dev = _simulate(call["robot"], *setup["args"], **setup["kw"])
    worst = _compare(dev, call["runs"])
    assert sorted(set(dev.limit_flags)) == sorted({r["limit_flags"] for r in call["runs"]}) and dev.limit_flags[call["src"]] == 7
    print(f"limits, {first} first: flags {list(dev.limit_flags)}, first_violation_t {list(dev.first_violation_t)}, worst {worst:.2e}")


@pytest.mark.gpu
def test_device_zero_torque_limit_flags_and_gives_no_ratio():
    setup = _limit_runs()
    rb = _limited_robot(zero_torque=ZERO_TORQUE_JOINT)
    runs = [with_limits(h, rb) for h in setup["host"]]
    assert min(r["margins"]["torque"] for r in runs) >= MARGIN
    dev = _simulate(rb, *setup["args"], **setup["kw"])
    worst = _compare(dev, runs)
    assert np.all(np.isfinite(dev.max_torque_ratio)) and np.all(dev.limit_flags == TORQUE)
    for b, r in enumerate(runs):
        first = int(np.flatnonzero(dev.trace[b][:, 2, ZERO_TORQUE_JOINT] != 0)[0])
        assert _same_bits(dev.first_violation_t[b], r["nodes"][first][0])
    print(f"zero torque limit: ratio {list(dev.max_torque_ratio)}, worst {worst:.2e}")


@functools.lru_cache(maxsize=None)
def _sagging_runs():
    """The passive plant from rest: the arm sags under gravity.  Three rollouts of 40 steps, conditioning shown first."""
    rb = _robot()
    rng = np.random.default_rng(22)
    B, D = 3, 1.0
    q0, qd0, qdd0, k = _plans(rng, B)
    z0 = np.concatenate([rng.uniform(-1.0, 1.0, (B, N_J)), np.zeros((B, N_J))], axis=1)
    kw = dict(t1=0.04, dt=1e-3, controller="none", record_every=1)
    host = [_well_conditioned(lambda z, b=b: host_track(rb, q0[b], qd0[b], qdd0[b], k[b], K_RANGE, D, z0=z, **kw), z0[b]) for b in range(B)]
    return dict(args=(q0, qd0, qdd0, k, K_RANGE, D), kw=dict(kw, z0=z0), host=host)


@functools.lru_cache(maxsize=None)
def _one_sided_call():
    """Only state_limits_lb of one joint and one speed limit are tightened, each half-way before a node at which rollout 0 moves further
    in the NEGATIVE direction; no joint of any rollout crosses an upper position limit or a speed limit from above."""
    setup = _sagging_runs()
    nodes = setup["host"][0]["nodes"]
    q, qd = np.array([nd[1] for nd in nodes]), np.array([nd[2] for nd in nodes])
    default = _robot()
    for jp, js in itertools.product(range(N_J), range(1, N_J)):
        lo = np.minimum.accumulate(q[:, jp])
        mp = [m for m in range(8, 20) if q[m, jp] < lo[m - 1] and q[m, jp] > default.state_limits_lb[jp]]
        hi = np.maximum.accumulate(np.abs(qd[:, js]))
        ms = [m for m in range(22, 36) if qd[m, js] < 0 and -qd[m, js] > hi[m - 1]]
        if not (mp and ms):
            continue
        rb = _robot()
        rb.state_limits_lb[jp] = 0.5 * (lo[mp[0] - 1] + q[mp[0], jp])
        rb.speed_limits[js] = 0.5 * (hi[ms[0] - 1] - qd[ms[0], js])
        runs = [with_limits(h, rb) for h in setup["host"]]
        ub, speed = np.array(rb.state_limits_ub[:N_J]), np.array(rb.speed_limits[:N_J])
        above = any(np.any(nd[1] > ub) or np.any(nd[2] > speed) for r in runs for nd in r["nodes"])
        if not above and runs[0]["limit_flags"] == (POSITION | SPEED) and min(min(r["margins"].values()) for r in runs) >= MARGIN:
            return dict(robot=rb, runs=runs, chosen=(jp, mp[0], js, ms[0]))
    raise AssertionError("no one-sided placement found")


def test_one_sided_limits_flag_the_restatement_from_below_only():
    call = _one_sided_call()
    jp, mp, js, ms = call["chosen"]
    r = call["runs"][0]
    assert r["limit_flags"] == (POSITION | SPEED) and r["first_violation_t"] == mp * r["h"] and mp < ms
    # with the two negative-side comparisons dropped nothing would be flagged at all
    lb, ub, speed, _ = [np.array(x[:N_J]) for x in (call["robot"].state_limits_lb, call["robot"].state_limits_ub, call["robot"].speed_limits, call["robot"].torque_limits)]
    assert not any(np.any(nd[1] > ub) or np.any(nd[2] > speed) for run in call["runs"] for nd in run["nodes"])
    assert any(nd[1][jp] < lb[jp] for nd in r["nodes"]) and any(nd[2][js] < -speed[js] for nd in r["nodes"])
    print(f"one-sided: lb of joint {jp} crossed at node {mp}, -speed of joint {js} at node {ms}, flags {[x['limit_flags'] for x in call['runs']]}")


@pytest.mark.gpu
def test_device_flags_limits_crossed_from_below():
    setup, call = _sagging_runs(), _one_sided_call()
    dev = _simulate(call["robot"], *setup["args"], **setup["kw"])
    worst = _compare(dev, call["runs"])
    assert dev.limit_flags[0] == (POSITION | SPEED)
    print(f"one-sided limits: flags {list(dev.limit_flags)}, worst {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 2. stops and their neighbours
def _stop_setup(B, stopped, controller, seed):
    from armour_amd.tracking import plant_samples
    rb = _robot()
    rng = np.random.default_rng(seed)
    D = 1.0
    q0, qd0, qdd0, k = _plans(rng, B)
    sm, sI = plant_samples(rb, B, rb.mass_uncertainty, rng)
    if controller == "none":
        z0 = np.concatenate([q0 + rng.uniform(-5e-3, 5e-3, (B, N_J)), qd0 + rng.uniform(-5e-3, 5e-3, (B, N_J))], axis=1)
    else:
        z0 = _start_inside(rb, rng, q0, qd0, qdd0, k, K_RANGE, D, sm, sI)
    for b in stopped:
        z0[b, N_J + 2] = 1e200
    kw = dict(t1=0.012, dt=1e-3, controller=controller, record_every=4)
    run_of = lambda b, z: host_track(rb, q0[b], qd0[b], qdd0[b], k[b], K_RANGE, D, sm=sm[b], sI=sI[b], z0=z, **kw)
    return rb, (q0, qd0, qdd0, k), sm, sI, z0, kw, run_of


def _assert_stopped_at_node_0(dev, b, z0, flags):
    assert dev.status[b] == 2 and dev.steps[b] == 0 and dev.t_end[b] == 0.0
    assert _same_bits(dev.q[b], z0[b, :N_J]) and _same_bits(dev.qd[b], z0[b, N_J:])
    assert dev.max_V[b] == np.inf and dev.max_vel_error[b] >= 1e199 and dev.limit_flags[b] == flags and dev.first_violation_t[b] == 0.0
    assert _same_bits(dev.trace[b][0, 0], z0[b, :N_J]) and _same_bits(dev.trace[b][0, 1], z0[b, N_J:])
    assert np.all(np.isnan(dev.trace[b][1:]))


def test_restatement_stops_at_node_0_on_a_state_that_overflows():
    for controller, flags in (("none", SPEED), ("nominal", SPEED | TORQUE), ("robust", SPEED | TORQUE)):
        rb, plans, sm, sI, z0, kw, run_of = _stop_setup(2, (0,), controller, 31)
        r = run_of(0, z0[0])
        assert (r["status"], r["steps"], r["t_end"], r["limit_flags"], r["first_violation_t"]) == (2, 0, 0.0, flags, 0.0), (controller, r["status"], r["limit_flags"])
        assert r["max_V"] == np.inf and r["max_vel_error"] >= 1e199 and np.array_equal(r["q"], z0[0, :N_J]) and np.array_equal(r["qd"], z0[0, N_J:])
        assert np.all(np.isnan(r["trace"][1:])) and np.array_equal(r["trace"][0, 1], z0[0, N_J:])


@functools.lru_cache(maxsize=None)
def _passive_stop_runs():
    """B = 5 on the passive plant, lanes 1 and 3 overflow at node 0; the live lanes behind the conditioning guard."""
    B, stopped = 5, (1, 3)
    setup = _stop_setup(B, stopped, "none", 32)
    z0, run_of = setup[4], setup[6]
    host = [run_of(b, z0[b]) if b in stopped else _well_conditioned(lambda z, b=b: run_of(b, z), z0[b]) for b in range(B)]
    assert [h["status"] for h in host] == [0, 2, 0, 2, 0]
    return setup, host


@pytest.mark.gpu
def test_stopped_rollouts_keep_node_0_and_leave_their_neighbours_alone():
    B, stopped, live = 5, (1, 3), [0, 2, 4]
    (rb, plans, sm, sI, z0, kw, run_of), host = _passive_stop_runs()
    dev = _simulate(rb, *plans, K_RANGE, 1.0, z0=z0, mass_scale=sm, inertia_scale=sI, steps_per_launch=5, **kw)
    assert dev.trace.shape[1] == 4
    for b in stopped:
        _assert_stopped_at_node_0(dev, b, z0, SPEED)
    worst = _compare(dev, host)
    alone = _simulate(rb, *[a[live] for a in plans], K_RANGE, 1.0, z0=z0[live], mass_scale=sm[live], inertia_scale=sI[live], steps_per_launch=5, **kw)
    for i, b in enumerate(live):
        _bit_equal(dev, alone, b, i)
        assert dev.status[b] == 0 and dev.steps[b] == 12
    print(f"stops, passive plant: worst {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("controller", ["robust", "nominal"])
def test_a_stop_under_a_controller_leaves_the_live_lane_alone(controller):
    rb, plans, sm, sI, z0, kw, run_of = _stop_setup(2, (0,), controller, 31)
    host = [run_of(b, z0[b]) for b in range(2)]
    assert host[0]["status"] == 2 and host[0]["limit_flags"] == 5 and host[1]["status"] == 0
    dev = _simulate(rb, *plans, K_RANGE, 1.0, z0=z0, mass_scale=sm, inertia_scale=sI, steps_per_launch=5, **kw)
    _assert_stopped_at_node_0(dev, 0, z0, 5)
    worst = _compare(dev, host)
    alone = _simulate(rb, *[a[1:] for a in plans], K_RANGE, 1.0, z0=z0[1:], mass_scale=sm[1:], inertia_scale=sI[1:], steps_per_launch=5, **kw)
    _bit_equal(dev, alone, 1, 0)
    print(f"stops, {controller}: worst {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 3. the time grid
DT = 1e-3
T1_BELOW, T1_ABOVE = 70 * DT + 5e-10 * DT, 70 * DT + 5e-9 * DT   # (t1 - t0)/dt on either side of the rule's 1e-9
# last_bit: on the three grids above t0 + N h happens to round to t1 itself, so "node N is at t1" could not be told from "at t0 + N h"; here
# (N = 35) the two differ in the last bit
GRIDS = dict(ragged=(0.13, 0.2005), below=(0.0, T1_BELOW), above=(0.0, T1_ABOVE), last_bit=(0.07, 0.10445))
GRID_N = dict(ragged=71, below=70, above=71, last_bit=35)


def _rule_N(t0, t1, dt):
    return int(np.ceil((t1 - t0) / dt - 1e-9))


def test_the_grid_cases_land_where_intended():
    assert all(_rule_N(*GRIDS[name], DT) == N for name, N in GRID_N.items())
    assert T1_BELOW / DT > 70 and int(np.ceil(T1_BELOW / DT)) == 71    # without the 1e-9 the first would take 71 steps
    # the last node is t1 itself, not t0 + N h: on at least one grid the two differ in their bits, so the rule can be seen
    differ = [name for name, (t0, t1) in GRIDS.items() if t0 + _rule_N(t0, t1, DT) * ((t1 - t0) / _rule_N(t0, t1, DT)) != t1]
    assert differ == ["last_bit"]
    # h = (t1 - t0)/N is not dt on the ragged grids
    assert all((t1 - t0) / _rule_N(t0, t1, DT) != DT for t0, t1 in GRIDS.values())


@functools.lru_cache(maxsize=None)
def _grid_setup(name):
    """Nominal controller, two rollouts starting ON the reference at t0 (z0 = None)."""
    rb = _robot()
    q0, qd0, qdd0, k = _plans(np.random.default_rng(41), 2)
    t0, t1 = GRIDS[name]
    kw = dict(t0=t0, t1=t1, dt=DT, controller="nominal")
    host = {}

    def host_runs(record_every):
        if record_every not in host:
            host[record_every] = [host_track(rb, q0[b], qd0[b], qdd0[b], k[b], K_RANGE, 1.0, record_every=record_every, **kw) for b in range(2)]
        return host[record_every]
    return rb, (q0, qd0, qdd0, k, K_RANGE, 1.0), kw, host_runs


def test_restatement_on_the_ragged_grid():
    rb, args, kw, host_runs = _grid_setup("ragged")
    for r in host_runs(7):
        assert (r["N"], r["steps"], r["status"]) == (71, 71, 0) and r["t_end"] == 0.2005 and r["trace"].shape[0] == 11
        assert r["max_pos_error"] <= 1e-10 and r["max_vel_error"] <= 1e-9     # exact tracking from a start on the reference at t0 = 0.13
        assert np.array_equal(r["trace"][10, 0], r["nodes"][70][1]) and not np.array_equal(r["trace"][10, 0], r["q"])


@pytest.mark.gpu
def test_ragged_grid_ends_at_t1_and_records_every_seventh_node():
    rb, args, kw, host_runs = _grid_setup("ragged")
    host = host_runs(7)
    dev = _simulate(rb, *args, record_every=7, **kw)
    assert np.all(dev.steps == 71) and _same_bits(dev.t_end, [0.2005, 0.2005]) and dev.trace.shape[1] == 11
    worst = _compare(dev, host)
    assert not np.array_equal(dev.trace[:, 10, 0], dev.q)                    # node 70 is the last record, node 71 is the state
    lone = _simulate(rb, *args, record_every=71 + 5, **kw)
    assert lone.trace.shape[1] == 1
    for b in range(2):
        assert _same_bits(lone.trace[b, 0], dev.trace[b, 0])
        start = _reference(args[0][b], args[1][b], args[2][b], args[3][b], K_RANGE, 1.0, 0.13)   # z0 = NULL: on the reference at t0
        assert np.abs(lone.trace[b, 0, 0] - start[0]).max() <= 1e-14 and np.abs(lone.trace[b, 0, 1] - start[1]).max() <= 1e-14
    _bit_equal(lone, dev, slice(None), slice(None), fields=FIELDS[:-1])
    print(f"ragged grid: worst {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["below", "above", "last_bit"])
def test_step_count_and_last_node_follow_the_rule(name):
    rb, args, kw, host_runs = _grid_setup(name)
    host = host_runs(0)
    N = _rule_N(kw["t0"], kw["t1"], DT)
    assert N == GRID_N[name] and all(r["N"] == N and r["steps"] == N for r in host)
    dev = _simulate(rb, *args, **kw)
    assert np.all(dev.steps == N) and _same_bits(dev.t_end, [kw["t1"]] * 2)
    worst = _compare(dev, host)
    print(f"grid {name}: N {N}, worst {worst:.2e}")


@pytest.mark.gpu
def test_steps_per_launch_at_and_above_the_node_count_changes_no_bit():
    rb, args, kw, _ = _grid_setup("ragged")
    N = 71
    one = _simulate(rb, *args, record_every=7, steps_per_launch=1, **kw)
    assert np.all(one.steps == N)
    for S in (N, N + 1, 10 * N):
        _bit_equal(_simulate(rb, *args, record_every=7, steps_per_launch=S, **kw), one, slice(None), slice(None))


# ------------------------------------------------------------------------------------------------ 4. block edges
def _edge_setup(B, controller, seed):
    from armour_amd.tracking import plant_samples
    rb = _robot()
    rng = np.random.default_rng(seed)
    q0, qd0, qdd0, k = _plans(rng, B)
    sm, sI = plant_samples(rb, B, rb.mass_uncertainty, rng)
    z0 = np.concatenate([q0 + rng.uniform(-5e-3, 5e-3, (B, N_J)), qd0 + rng.uniform(-5e-3, 5e-3, (B, N_J))], axis=1)
    kw = dict(t1=0.003, dt=1e-3, controller=controller, record_every=1)
    run_of = lambda b, z: host_track(rb, q0[b], qd0[b], qdd0[b], k[b], K_RANGE, 1.0, sm=sm[b], sI=sI[b], z0=z, **kw)
    sim = lambda s: _simulate(rb, q0[s], qd0[s], qdd0[s], k[s], K_RANGE, 1.0, z0=z0[s], mass_scale=sm[s], inertia_scale=sI[s], **kw)
    return z0, run_of, sim


@functools.lru_cache(maxsize=None)
def _passive_edge_runs():
    B = 130
    z0, run_of, sim = _edge_setup(B, "none", 51)
    return sim, [_well_conditioned(lambda z, b=b: run_of(b, z), z0[b]) for b in range(B)]


def test_passive_plant_runs_are_well_conditioned():
    """CPU: the conditioning guard of every passive-plant comparison below (the sagging arm's is in _sagging_runs)."""
    assert len(_passive_edge_runs()[1]) == 130 and len(_passive_stop_runs()[1]) == 5 and len(_sagging_runs()["host"]) == 3


@pytest.mark.gpu
def test_every_lane_of_three_blocks_on_the_passive_plant():
    B = 130
    sim, host = _passive_edge_runs()
    dev = sim(slice(0, B))
    assert np.all(dev.steps == 3)
    worst = _compare(dev, host)
    print(f"B = 130, passive plant: worst {worst:.2e}")


@pytest.mark.gpu
def test_a_second_mostly_idle_block_under_the_robust_controller():
    B, lanes = 65, [0, 63, 64]
    z0, run_of, sim = _edge_setup(B, "robust", 52)
    dev = sim(slice(0, B))
    assert np.all(dev.steps == 3) and np.all(dev.status == 0)
    worst = _compare(dev, [run_of(b, z0[b]) for b in lanes], lanes=lanes)
    _bit_equal(dev, sim(slice(64, 65)), 64, 0)
    for size in (63, 64):
        full = sim(slice(0, size))
        _bit_equal(full, sim(slice(size - 1, size)), size - 1, 0)
        _bit_equal(full, dev, size - 1, size - 1)
    print(f"B = 65, robust: worst {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 5. the 8-factor ABI
def _k128_robots():
    from armour_amd import planner
    return (("kinova", planner.kinova_robot()), ("fetch8", planner.fetch8_robot()))


def _k128_rollouts(name, rb, controller):
    """B = 4, N = 20 with plant scales and a trace, every rollout behind the conditioning guard.
    Kinova: plants within +-5 %, model_uncertainty 0.05, starts at 0.9 V_max -- the robust input is at work within the 20 steps (max |v| 0.3 to
    0.8 on the restatement).  Fetch presets: V_max = 1e-2.  Under the nominal controller plants within the robot's +-3 % and starts 1e-3
    off the reference.  Under the robust controller the Fetch's interval torque radius is ~2.4 N m at 3 %, so once |r| passes
    alpha V_max / 2.4 = 4e-3 the input switches on with a gain that RK4 at dt = 1e-3 cannot follow: it chatters and a 1e-13 perturbation grows
    to 1e-9 in 20 steps (measured on the restatement; the guard refuses such a run).  So those rollouts stay below that: plants within +-0.1 %,
    starts 1e-5 off the reference, v = 0 throughout -- the robust update runs in full (interval passes, lambda's comparison) with lambda = 0;
    a non-zero v in this ABI is held by the controller cell of the same test (Fetch, 8 of 8) and by the Kinova rollouts (7 of 8)."""
    from armour_amd.tracking import plant_samples
    n = rb.num_factors
    rng = np.random.default_rng(61)
    B, D, kr = 4, 1.0, np.full(n, np.pi / 48)
    q0, qd0, qdd0, k = _plans(rng, B, n)
    eps = 0.05 if name == "kinova" else rb.mass_uncertainty
    sm, sI = plant_samples(rb, B, eps if name == "kinova" or controller == "nominal" else 1e-3, rng)
    if name == "kinova":
        z0 = _start_inside(rb, rng, q0, qd0, qdd0, k, kr, D, sm, sI, frac=0.9)
    else:
        off = 1e-3 if controller == "nominal" else 1e-5
        z0 = np.stack([np.concatenate(_reference(q0[b], qd0[b], qdd0[b], k[b], kr, D, 0.0)[:2]) for b in range(B)]) + rng.uniform(-off, off, (B, 2 * n))
    kw = dict(t1=0.02, dt=1e-3, controller=controller, record_every=1, V_max=1e-2)
    run_of = lambda b, z: host_track(rb, q0[b], qd0[b], qdd0[b], k[b], kr, D, sm=sm[b], sI=sI[b], z0=z, eps=eps, **kw)
    host = [_well_conditioned(lambda z, b=b: run_of(b, z), z0[b]) for b in range(B)]
    if controller == "robust":
        assert all(h["max_robust_input"] > 0.1 for h in host) if name == "kinova" else all(h["max_robust_input"] == 0 for h in host)
    return (rb, q0, qd0, qdd0, k, kr, D), dict(kw, z0=z0, mass_scale=sm, inertia_scale=sI, model_uncertainty=eps), host


def _body_k128_cpu():
    """(runs with ARMOUR_KEY128=1)  the restatement's exactness under the nominal controller with 8 slots per array, and the entry's argument checks"""
    import test_tracking as tt
    from oracle import cpu_oracle as orc
    assert _lib.MAXF == 8 and orc.MAXF == 8 and _lib.load().armour_abi_max_factors() == 8
    for name, rb in _k128_robots():
        n = rb.num_factors
        assert n == {"kinova": 7, "fetch8": 8}[name]
        q0, qd0, qdd0, k = _plans(np.random.default_rng(5), 1, n)
        out = host_track(rb, q0[0], qd0[0], qdd0[0], k[0], np.full(n, np.pi / 48), 1.0, t1=0.1, controller="nominal")
        assert out["status"] == 0 and out["steps"] == 100 and out["max_pos_error"] <= 1e-10 and out["max_vel_error"] <= 1e-9, (name, out["max_pos_error"])
        print(f"{name}: nominal controller tracks to {out['max_pos_error']:.1e} rad, {out['max_vel_error']:.1e} rad/s", flush=True)
    for name, rb in _k128_robots():   # the conditioning guards of the device comparison
        for controller in (("robust",) if name == "kinova" else ("nominal", "robust")):
            _k128_rollouts(name, rb, controller)
    tt.test_entry_checks_its_arguments()
    print("track k128 cpu ok", flush=True)


def _body_k128_gpu(kinova_default_abi):
    """(runs with ARMOUR_KEY128=1)  one cell of the controller's device-against-oracle comparison, then tracking against the restatement"""
    import test_controller as tc
    from armour_amd.controller import kinova_controller
    from oracle.cpu_oracle import robust_controller
    assert _lib.MAXF == 8 and _lib.load().armour_abi_max_factors() == 8
    eps, V_max, alpha, B = 0.03, 1e-2, 1.0, 304
    for name, rb in _k128_robots():
        n = rb.num_factors
        Kr = np.random.default_rng(500).uniform(5, 20, n)
        arrs = tc._wide_states(700 + n, B, n, far=4)
        got = tc._through_both_kernels(lambda: kinova_controller(Kr, alpha, V_max, tc.R_THR, *arrs, eps=eps, robot=rb))
        refs = [robust_controller(Kr, alpha, V_max, tc.R_THR, *[a[s] for a in arrs], eps=eps, robot=rb) for s in range(B)]
        tc._assert_matches_oracle(got, range(B), lambda s: refs[s], ("k128", name))
        assert sum(r["v"].any() for r in refs) >= 0.05 * B
        print(f"controller, {name} (n = {n} of 8): {B} states at 1e-12", flush=True)
    for name, rb in _k128_robots():
        for controller in (("robust",) if name == "kinova" else ("nominal", "robust")):
            args, kw, host = _k128_rollouts(name, rb, controller)
            dev = _simulate(*args, **kw)
            assert np.all(dev.steps == 20)
            worst = _compare(dev, host)
            print(f"tracking, {name}, {controller}: worst {worst:.2e}", flush=True)
            if name == "kinova":
                ref = np.load(kinova_default_abi)
                same = all(np.array_equal(getattr(dev, f), ref[f], equal_nan=True) for f in FIELDS)
                print(f"kinova bits equal across ABIs: {same}", flush=True)
    print("track k128 gpu ok", flush=True)


def _run_k128(call):
    env = dict(os.environ, ARMOUR_KEY128="1")
    env.pop("ARMOUR_HIP_LIB", None)
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_tracking_edges as t; t.%s" % (ROOT, os.path.join(ROOT, "tests"), call)
    return subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_eight_factor_abi_restatement_and_argument_checks():
    r = _run_k128("_body_k128_cpu()")
    assert r.returncode == 0 and "track k128 cpu ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)


@pytest.mark.gpu
def test_eight_factor_abi_controller_and_tracking_on_the_device(tmp_path):
    # the Kinova rollouts of the child in this process' 7-factor ABI, for the bit comparison the child prints
    args, kw, host = _k128_rollouts("kinova", _robot(), "robust")
    dev = _simulate(*args, **kw)
    _compare(dev, host)
    path = str(tmp_path / "kinova_default_abi.npz")
    np.savez(path, **{f: getattr(dev, f) for f in FIELDS})
    r = _run_k128("_body_k128_gpu(%r)" % path)
    assert r.returncode == 0 and "track k128 gpu ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout)
