"""Time-sliced roadmap verdicts and the earliest-arrival search (include/armour_hip.h armour_roadmap_check_slices / armour_roadmap_arrival,
armour_amd.roadmap.Roadmap.check_slices / arrival / plan_slices): the host twins.

The sliced check is defined by the window rule: bit k of a mask is armour_roadmap_check_moving's verdict on [slice_times[k], slice_times[k + 1]],
so the library's own window check (tests/test_roadmap_moving.py compares it with a numpy restatement) is the reference, slice by slice.  The
search is restated here as a plain breadth-first search over (node, slice) states written from the header's definition, with Python integers
and no mask arithmetic.  Shared helpers for tests/test_roadmap_slices_gpu.py live here too."""
import collections
import ctypes as C
import heapq

import numpy as np
import pytest

from test_roadmap import _robot, config_clearance
from test_roadmap_moving import STEP, _case, _host, arriving_box_scene

T0 = np.array([0.0, 0.4, -0.3])                  # one clock per world
# (K, dt): 33 crosses the dword boundary of the mask, 64 is the full-width mask; every horizon K dt is 1 - 2 s, over which boxes at
# 0.2 - 1.0 m/s arrive at and leave nodes and edges
SLICINGS = ((1, 0.3), (5, 0.2), (33, 0.05), (64, 0.03))


def ones(K):
    return (1 << K) - 1


def bit(masks, k):
    return ((masks >> np.uint64(k)) & np.uint64(1)).astype(bool)


def some_extras(nodes, W, seed=3):
    """(world [Q], a [Q,n], b [Q,n]): per world one edge between two nodes that the roadmap does not join, one from a random configuration to a
    node, and one degenerate edge a == b on a node"""
    rng = np.random.default_rng(seed)
    N, n = nodes.shape
    world, a, b = [], [], []
    for w in range(W):
        i, j, k = rng.choice(N, 3, replace=False)
        world += [w, w, w]
        a += [nodes[i], nodes[j] + rng.uniform(-0.3, 0.3, n), nodes[k]]
        b += [nodes[j], nodes[i], nodes[k]]
    return np.array(world, dtype=np.int32), np.array(a), np.array(b)


# ----------------------------------------------------------------------------------------------------------- the sliced check
@pytest.mark.parametrize("name", ["kinova", "fetch"])
@pytest.mark.parametrize("K,dt", SLICINGS)
def test_every_bit_is_the_window_check_on_its_slice(name, K, dt):
    robot, g, nodes, edges, cont, obs, vel = _case(name)
    rm = _host(robot, nodes, edges, cont)
    xw, xa, xb = some_extras(nodes, obs.shape[0])
    s = rm.check_slices(obs, vel, T0, dt, K, extra_world=xw, extra_a=xa, extra_b=xb, host=True)
    bare = rm.check_slices(obs, vel, T0, dt, K, host=True)                          # Q = 0 with null arrays
    assert np.array_equal(bare["node_slices"], s["node_slices"]) and np.array_equal(bare["edge_slices"], s["edge_slices"]) and bare["extra_slices"].size == 0
    t = s["slice_times"]
    assert t.shape == (3, K + 1) and np.array_equal(t, T0[:, None] + np.arange(K + 1)[None, :] * dt)
    for fam in ("node_slices", "edge_slices", "extra_slices"):
        assert s[fam].dtype == np.uint64 and (K == 64 or not (s[fam] >> np.uint64(K)).any()), fam       # bits >= K are 0
    for k in range(K):
        v = rm.check_moving(obs, vel, t[:, k], t[:, k + 1], host=True)
        assert np.array_equal(bit(s["node_slices"], k), v["node_free"]), (name, K, k)
        assert np.array_equal(bit(s["edge_slices"], k), v["edge_free"]), (name, K, k)
        for i in range(xw.size):                                                     # an extra edge: the direct edge of plan() in that window
            direct = rm.plan(int(xw[i]), xa[i], xb[i], connect_k=0) is not None
            assert bool(bit(s["extra_slices"][i:i + 1], k)[0]) == direct, (name, K, k, i)
    for fam in ("node_slices", "edge_slices"):
        m = s[fam]
        mixed = int(((m != 0) & (m != np.uint64(ones(K)))).sum())
        print(f"{name} K={K} {fam}: {int((m != 0).sum())} with a set bit, {int((m != np.uint64(ones(K))).sum())} with a cleared bit, {mixed} whose slices differ")
        assert (m != 0).any() and (m != np.uint64(ones(K))).any(), (name, K, fam)
        assert K == 1 or mixed >= 1, (name, K, fam)
    rm.close()


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_a_degenerate_extra_edge_is_the_node_rule(name):
    robot, g, nodes, edges, cont, obs, vel = _case(name)
    rm = _host(robot, nodes, edges, cont)
    W, N = obs.shape[0], nodes.shape[0]
    xw = np.repeat(np.arange(W, dtype=np.int32), N)
    xq = np.tile(nodes, (W, 1))
    s = rm.check_slices(obs, vel, T0, 0.05, 33, extra_world=xw, extra_a=xq, extra_b=xq, host=True)
    assert np.array_equal(s["extra_slices"].reshape(W, N), s["node_slices"])
    assert len(np.unique(s["extra_slices"])) > 2
    rm.close()


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_obstacles_at_rest_give_all_slices_or_none(name):
    robot, g, nodes, edges, cont, obs, _ = _case(name)
    rm = _host(robot, nodes, edges, cont)
    zero = np.zeros(obs.shape[:2] + (3,))
    static = rm.check_moving(obs, zero, 0.0, 0.0, host=True)            # the static rule, for any window (tests/test_roadmap_moving.py)
    for w in range(obs.shape[0]):
        assert np.array_equal(static["node_free"][w], config_clearance(g, nodes, obs[w]) > 0)
    for K in (1, 33, 64):
        s = rm.check_slices(obs, zero, T0, 0.11, K, host=True)
        for fam, key in (("node_slices", "node_free"), ("edge_slices", "edge_free")):
            assert np.array_equal(s[fam], np.where(static[key], np.uint64(ones(K)), np.uint64(0))), (name, K, fam)
    assert static["node_free"].any() and not static["node_free"].all() and static["edge_free"].any() and not static["edge_free"].all()
    rm.close()


def test_a_sliced_check_leaves_the_window_state_alone():
    robot, g, nodes, edges, cont, obs, vel = _case("kinova")
    rm = _host(robot, nodes, edges, cont)
    rm.check_moving(obs, vel * 0.25, [0.0, 0.4, -0.3], [0.2, 0.5, 0.0], host=True)
    pairs = [(w, i, j) for w in range(3) for i, j in ((0, 40), (7, 23), (12, 31))]
    before = [rm.plan(w, nodes[i] + 0.01, nodes[j] - 0.01) for w, i, j in pairs]
    rm.check_slices(obs, vel, T0 + 5.0, 0.2, 7, host=True)
    after = [rm.plan(w, nodes[i] + 0.01, nodes[j] - 0.01) for w, i, j in pairs]
    assert sum(p is not None and p.shape[0] > 2 for p in before) >= 2
    for a, b in zip(before, after):
        assert (a is None and b is None) or np.array_equal(a, b)
    rm.close()


# ----------------------------------------------------------------------------------------------------------- the search, restated
def edge_steps(length, step_len):
    ratio = length / step_len
    assert abs(ratio - round(ratio)) > 1e-9 or ratio == round(ratio), ratio       # not within rounding of an integer, unless exactly one
    return max(1, int(np.ceil(ratio)))


def roadmap_lengths(rm):
    from armour_amd.roadmap import wrapped_diff
    d = wrapped_diff(rm.nodes[rm.edges[:, 0]], rm.nodes[rm.edges[:, 1]], rm.continuous.astype(bool))
    return np.sqrt((d * d).sum(-1))


def world_graph(rm, w, K, step_len, node_slices, edge_slices, start_mask, goal_mask, extras):
    """(mask [N + 2] of Python ints, edges [(u, v, steps, mask)] with the roadmap's edges first): world w's graph as the header defines it.
    extras: (x_world, x_u, x_v, x_len, x_mask)."""
    N = rm.N
    mask = [int(m) for m in node_slices[w]] + [(int(start_mask[w]) | 1) & ones(K), int(goal_mask[w]) & ones(K)]
    lens = roadmap_lengths(rm)
    es = [(int(a), int(b), edge_steps(lens[e], step_len), int(edge_slices[w, e])) for e, (a, b) in enumerate(rm.edges)]
    xw, xu, xv, xl, xm = extras
    es += [(int(xu[i]), int(xv[i]), edge_steps(xl[i], step_len), int(xm[i]) & ones(K)) for i in range(len(xw)) if xw[i] == w]
    return mask, es


def arrival_np(N, K, mask, es):
    """reach [N + 2] as Python ints by a breadth-first search over (node, slice) states: from (u, k) wait to (u, k + 1) if u is free in
    slice k + 1; cross an edge of c <= K steps to (v, k + c) if the edge is free in every slice k .. k + c - 1 and v is free in slice k + c."""
    free = lambda m, k: k < K and (m >> k) & 1
    adj = collections.defaultdict(list)
    for u, v, c, m in es:
        if c <= K:
            adj[u].append((v, c, m))
            adj[v].append((u, c, m))
    seen = {(N, 0)}
    todo = collections.deque(seen)
    while todo:
        u, k = todo.popleft()
        nxt = [(u, k + 1)] if free(mask[u], k + 1) else []
        nxt += [(v, k + c) for v, c, m in adj[u] if all(free(m, k + i) for i in range(c)) and free(mask[v], k + c)]
        for st in nxt:
            if st not in seen:
                seen.add(st)
                todo.append(st)
    reach = [0] * (N + 2)
    for v, k in seen:
        reach[v] |= 1 << k
    return reach


def check_path(N, K, mask, es, reach, goal_slice, path_len, path_node, path_slice):
    """the path is valid: from (N, .) to (N + 1, goal_slice), slices strictly increasing, each hop a usable edge left late enough, with its
    avail bit set, and every wait at a node inside the node's mask"""
    if goal_slice < 0:
        assert path_len == 0 and (path_node == -1).all() and (path_slice == -1).all()
        return
    P = int(path_len)
    assert 2 <= P <= K and (path_node[P:] == -1).all() and (path_slice[P:] == -1).all()
    nodes, sl = [int(v) for v in path_node[:P]], [int(k) for k in path_slice[:P]]
    assert nodes[0] == N and nodes[-1] == N + 1 and sl[-1] == goal_slice
    assert all(a < b for a, b in zip(sl, sl[1:]))
    for i in range(P - 1):
        u, v, ku, kv = nodes[i], nodes[i + 1], sl[i], sl[i + 1]
        first = 0 if i == 0 else ku                                     # the arm is at the start from slice 0 on
        hops = [(c, m) for a, b, c, m in es if {a, b} == {u, v} and c <= K and kv - c >= ku and all((m >> (kv - c + j)) & 1 for j in range(c))]
        assert any(all((mask[u] >> k) & 1 for k in range(first, kv - c + 1)) for c, m in hops) and (mask[v] >> kv) & 1, (i, u, v, ku, kv)
        assert (reach[u] >> ku) & 1 and (reach[v] >> kv) & 1


def search_case(rm, obs, vel, t0, dt, K, step_len, host, seed=11, join=4, odd_edges=True):
    """check_slices with the extras of a start and a goal per world, then arrival: (slices, arrival, extras, start_mask, goal_mask).  Start
    and goal are random configurations joined to their `join` nearest nodes and to each other; with odd_edges, two more start -> goal edges
    whose masks are all ones: one of exactly K steps and one of K + 1."""
    rng = np.random.default_rng(seed)
    W, N, n = obs.shape[0], rm.N, rm.n
    starts = rm.nodes[rng.choice(N, W)] + rng.uniform(-0.2, 0.2, (W, n))
    goals = rm.nodes[rng.choice(N, W)] + rng.uniform(-0.2, 0.2, (W, n))
    index, dist, _ = rm.knn(np.concatenate([starts, goals]), join, host=host)
    xw, xa, xb, xu, xv, xl = [], [], [], [], [], []
    for w in range(W):
        for side, (q, end) in enumerate(((starts[w], N), (goals[w], N + 1))):
            for c in range(join):
                v = int(index[side * W + w, c])
                xw.append(w), xa.append(q), xb.append(rm.nodes[v]), xu.append(end), xv.append(v), xl.append(dist[side * W + w, c])
        xw.append(w), xa.append(starts[w]), xb.append(goals[w]), xu.append(N), xv.append(N + 1), xl.append(float(np.linalg.norm(goals[w] - starts[w])))
    Q = len(xw)
    ext_w = np.concatenate([np.array(xw, dtype=np.int32), np.arange(W, dtype=np.int32), np.arange(W, dtype=np.int32)])
    ext_a = np.concatenate([np.array(xa), starts, goals])
    ext_b = np.concatenate([np.array(xb), starts, goals])
    s = rm.check_slices(obs, vel, t0, dt, K, extra_world=ext_w, extra_a=ext_a, extra_b=ext_b, host=host)
    xm = list(s["extra_slices"][:Q])
    start_mask, goal_mask = s["extra_slices"][Q:Q + W].copy(), s["extra_slices"][Q + W:].copy()
    if odd_edges:
        for w in range(W):
            for length in (step_len * K, step_len * (K + 0.5)):
                xw.append(w), xu.append(N), xv.append(N + 1), xl.append(length), xm.append(np.uint64(ones(K)))
    order = np.argsort(np.array(xw), kind="stable")
    extras = tuple(np.array(a)[order] for a in (np.array(xw, dtype=np.int32), np.array(xu, dtype=np.int32), np.array(xv, dtype=np.int32), np.array(xl),
                                                np.array(xm, dtype=np.uint64)))
    a = rm.arrival(step_len, start_mask, goal_mask, *extras, host=host)
    return s, a, extras, start_mask, goal_mask


@pytest.mark.parametrize("name", ["kinova", "fetch"])
@pytest.mark.parametrize("K,dt", [(5, 0.2), (64, 0.03)])
def test_arrival_is_the_breadth_first_search_of_the_definition(name, K, dt):
    robot, g, nodes, edges, cont, obs, vel = _case(name)
    rm = _host(robot, nodes, edges, cont)
    step_len = 0.25 if K == 64 else 2.0                 # (a power of two: step_len * K / step_len is K exactly)
    reached = 0
    for seed in (11, 12):
        s, a, extras, sm, gm = search_case(rm, obs, vel * 0.5, T0, dt, K, step_len, host=True, seed=seed)
        assert edge_steps(step_len * K, step_len) == K and edge_steps(step_len * (K + 0.5), step_len) == K + 1
        for w in range(obs.shape[0]):
            mask, es = world_graph(rm, w, K, step_len, s["node_slices"], s["edge_slices"], sm, gm, extras)
            reach = arrival_np(rm.N, K, mask, es)
            assert [int(r) for r in a["reach"][w]] == reach, (name, K, seed, w)
            want = (reach[rm.N + 1] & -reach[rm.N + 1]).bit_length() - 1
            assert a["goal_slice"][w] == want and 1 <= a["sweeps"][w] <= K + 1, (name, K, seed, w, a["sweeps"][w])
            check_path(rm.N, K, mask, es, reach, want, a["path_len"][w], a["path_node"][w], a["path_slice"][w])
            reached += want >= 0
            print(f"{name} K={K} seed {seed} world {w}: goal slice {want}, {int(a['path_len'][w])} path entries, {int(a['sweeps'][w])} sweeps, "
                  f"{sum(bin(r).count('1') for r in reach)} states")
    assert reached >= 1, "no world reaches its goal: the paths were not exercised"
    rm.close()


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_in_a_static_free_world_the_goal_slice_is_the_dijkstra_distance_in_steps(name):
    robot, g, nodes, edges, cont, obs, vel = _case(name)
    rm = _host(robot, nodes, edges, cont)
    far = obs.copy()
    far[:, :, 0] += 40.0                                                 # no obstacle within reach: every mask is all ones
    K, step_len = 64, 0.5
    hits = 0
    for seed in (11, 12, 13):
        s, a, extras, sm, gm = search_case(rm, far, np.zeros_like(vel), T0, 0.1, K, step_len, host=True, seed=seed, odd_edges=False)
        assert (s["node_slices"] == np.uint64(ones(K))).all() and (s["edge_slices"] == np.uint64(ones(K))).all()
        for w in range(far.shape[0]):
            mask, es = world_graph(rm, w, K, step_len, s["node_slices"], s["edge_slices"], sm, gm, extras)
            dist = {rm.N: 0}
            heap = [(0, rm.N)]
            adj = collections.defaultdict(list)
            for u, v, c, m in es:
                adj[u].append((v, c)), adj[v].append((u, c))
            while heap:
                d, u = heapq.heappop(heap)
                if d > dist[u]:
                    continue
                for v, c in adj[u]:
                    if d + c < dist.get(v, 1 << 30):
                        dist[v] = d + c
                        heapq.heappush(heap, (d + c, v))
            want = dist.get(rm.N + 1, 1 << 30)
            assert a["goal_slice"][w] == (want if want < K else -1), (name, seed, w, want)
            hits += want < K
    assert hits >= 3, hits
    rm.close()


def box_case(host, moving, dt=0.25, K=32, step_len=0.125, t0=1.0):
    """arriving_box_scene from world time t0, with the arm half a radian of joint 0 before node 0 and the goal half a radian past node 1,
    both off the box's line (the box sweeps nodes 0 and 1 as well as the edge, so an arm that waited AT node 0 would be struck): the two
    joining edges and the short edge take 4 slices each, the detour over node 2 twenty.  Returns (roadmap, slices, arrival, graph) -- close
    the roadmap."""
    robot = _robot("kinova")
    nodes, edges, cont, box, vel = arriving_box_scene(robot)
    from armour_amd.roadmap import Roadmap
    rm = Roadmap(robot, nodes, edges, continuous=cont, edge_step=0.1, host=host)
    N = 3
    start, goal = nodes[0].copy(), nodes[1].copy()
    start[0] -= 0.5
    goal[0] += 0.5
    xw = np.zeros(4, dtype=np.int32)
    s = rm.check_slices(box, vel if moving else np.zeros_like(vel), t0, dt, K, extra_world=xw, extra_a=np.stack([start, goal, start, goal]),
                        extra_b=np.stack([nodes[0], nodes[1], start, goal]), host=host)
    sm, gm = s["extra_slices"][2:3], s["extra_slices"][3:4]
    extras = (xw[:2], np.array([N, N + 1], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([0.5, 0.5]), s["extra_slices"][:2])
    a = rm.arrival(step_len, sm, gm, *extras, host=host)
    mask, es = world_graph(rm, 0, K, step_len, s["node_slices"], s["edge_slices"], sm, gm, extras)
    return rm, s, a, (mask, es)


def test_a_box_that_crosses_the_short_edge_delays_the_arrival():
    rm, s0, a0, _ = box_case(host=True, moving=False)
    rm.close()
    rm, s, a, (mask, es) = box_case(host=True, moving=True)
    K = 32
    short = int(s["edge_slices"][0, 0])
    print(f"short edge free in {short:032b}, at rest goal slice {a0['goal_slice'][0]}, moving {a['goal_slice'][0]}, path {a['path_node'][0, :a['path_len'][0]]} "
          f"at {a['path_slice'][0, :a['path_len'][0]]}")
    assert int(s0["edge_slices"][0, 0]) == ones(K) and a0["goal_slice"][0] == 4 + 4 + 4             # start -> node 0, the short edge, node 1 -> goal
    assert 0 < short < ones(K)                                           # the box is on the edge in some slices
    reach = arrival_np(3, K, mask, es)
    want = (reach[4] & -reach[4]).bit_length() - 1
    assert want > a0["goal_slice"][0] and a["goal_slice"][0] == want   # later than at rest, and the detour or the wait of the restatement
    assert [int(r) for r in a["reach"][0]] == reach
    check_path(3, K, mask, es, reach, want, a["path_len"][0], a["path_node"][0], a["path_slice"][0])
    assert a["path_slice"][0, 0] > 0                                    # it waits at the start until the box has passed
    rm.close()


# ----------------------------------------------------------------------------------------------------------- plan_slices
def test_plan_slices_times_its_polyline_by_the_slices():
    robot, g, nodes, edges, cont, obs, vel = _case("kinova")
    rm = _host(robot, nodes, edges, cont)
    rng = np.random.default_rng(4)
    starts, goals = nodes[[3, 17, 30]] + rng.uniform(-0.1, 0.1, (3, 7)), nodes[[41, 8, 22]] + rng.uniform(-0.1, 0.1, (3, 7))
    plans = rm.plan_slices(starts, goals, obs, vel * 0.25, T0, 0.1, 64, speed=5.0, connect_k=4, host=True)
    found = 0
    for w, p in enumerate(plans):
        assert p["goal_slice"] == rm.last_arrival["goal_slice"][w]
        if p["path"] is None:
            assert p["goal_slice"] == -1
            continue
        found += 1
        assert np.array_equal(p["path"][0], starts[w]) and np.array_equal(p["path"][-1], goals[w]) and p["node"][0] == rm.N and p["node"][-1] == rm.N + 1
        assert np.array_equal(p["path"][1:-1], nodes[p["node"][1:-1]]) and p["slice"][-1] == p["goal_slice"]
        assert np.array_equal(p["time"], T0[w] + p["slice"] * 0.1) and np.all(np.diff(p["time"]) > 0)
    assert found >= 1
    rm.close()


# ----------------------------------------------------------------------------------------------------------- refusals
def raw_slices(rm, host, W=1, O=1, obs=None, vel=None, t0=None, dt=0.1, K=4, Q=0, xw=None, xa=None, xb=None, handle=True):
    from armour_amd._lib import _dp
    box = np.array([[[0.5, 0.0, 0.5, 0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1]]])
    keep = [box if obs is None else obs, np.zeros((1, 1, 3)) if vel is None else vel, np.zeros(1) if t0 is None else t0]
    ptr = [None if a is False else _dp(a) for a in keep]
    ip = None if xw is None else xw.ctypes.data_as(C.POINTER(C.c_int32))
    args = [rm.h if handle else C.c_void_p(), W, O, ptr[0], ptr[1], ptr[2], dt, K, Q, ip, _dp(xa), _dp(xb), None, None, None, None]
    return rm.L.armour_roadmap_check_slices_host(*args) if host else rm.L.armour_roadmap_check_slices(*args, None)


def slices_refusals(rm, host):
    """every refusal of the sliced check's entries on `rm`: ARMOUR_EINVAL each, before a device is touched"""
    from armour_amd import _lib
    n = rm.n
    bad_box = np.array([[[0.5, 0.0, 0.5, 0.1, np.inf, 0, 0, 0.1, 0, 0, 0, 0.1]]])
    bad_vel = np.array([[[0.0, np.nan, 0.0]]])
    q, bad_q, w0 = np.zeros((1, n)), np.full((1, n), np.nan), np.zeros(1, dtype=np.int32)
    cases = dict(null_handle=dict(handle=False), negative_W=dict(W=-1), negative_O=dict(O=-1), too_many_obstacles=dict(O=257), null_obstacles=dict(obs=False),
                 obstacle_not_finite=dict(obs=bad_box), null_velocity=dict(vel=False), velocity_not_finite=dict(vel=bad_vel), null_t0=dict(t0=False),
                 t0_not_finite=dict(t0=np.array([np.nan])), K_zero=dict(K=0), K_negative=dict(K=-3), K_65=dict(K=65), dt_zero=dict(dt=0.0),
                 dt_negative=dict(dt=-0.1), dt_nan=dict(dt=float("nan")), dt_inf=dict(dt=float("inf")), last_boundary_overflows=dict(t0=np.array([1e308]), dt=1e307, K=64),
                 negative_Q=dict(Q=-1), null_extras=dict(Q=1), extra_world_negative=dict(Q=1, xw=w0 - 1, xa=q, xb=q), extra_world_W=dict(Q=1, xw=w0 + 1, xa=q, xb=q),
                 extra_a_not_finite=dict(Q=1, xw=w0, xa=bad_q, xb=q), extra_b_not_finite=dict(Q=1, xw=w0, xa=q, xb=bad_q))
    for tag, kw in cases.items():
        assert raw_slices(rm, host, **kw) == _lib.EINVAL, tag


def test_the_host_entries_refuse_bad_arguments():
    from armour_amd import _lib
    robot = _robot("kinova")
    nodes, edges, cont, box, vel = arriving_box_scene(robot)
    rm = _host(robot, nodes, edges, cont)
    slices_refusals(rm, host=True)
    slices_refusals(rm, host=False)                                      # the device entry's argument checks come before its device
    with pytest.raises(_lib.ArmourError) as ei:                          # no sliced check yet (every one above was refused)
        rm.arrival(0.1, 0, 0, host=True)
    assert ei.value.code == _lib.ESTATE
    with pytest.raises(_lib.ArmourError) as ei:                          # the device entries on a handle without a device
        rm.check_slices(box, vel, 0.0, 0.1, 4)
    assert ei.value.code == _lib.EDEVICE
    rm.check_slices(box, vel, 0.0, 0.1, 4, host=True)
    with pytest.raises(_lib.ArmourError) as ei:
        rm.arrival(0.1, 0, 0)
    assert ei.value.code == _lib.EDEVICE
    x = dict(x_world=[0], x_u=[3], x_v=[0], x_len=[0.1], x_mask=[15])
    assert rm.arrival(0.1, 0, 0, host=True, **x)["goal_slice"][0] == -1
    for tag, code, kw in (("step_len_zero", _lib.EINVAL, dict(step_len=0.0)), ("step_len_nan", _lib.EINVAL, dict(step_len=float("nan"))),
                          ("world_out_of_range", _lib.EINVAL, dict(x_world=[1])), ("end_out_of_range", _lib.EINVAL, dict(x_v=[5])),
                          ("negative_end", _lib.EINVAL, dict(x_u=[-1])), ("negative_length", _lib.EINVAL, dict(x_len=[-0.1])),
                          ("length_not_finite", _lib.EINVAL, dict(x_len=[np.inf]))):
        with pytest.raises(_lib.ArmourError) as ei:
            rm.arrival(kw.pop("step_len", 0.1), 0, 0, host=True, **{**x, **kw})
        assert ei.value.code == code, tag
    rm.close()
    rm = _host(robot, nodes, edges, cont)                                # two worlds: the extras must be sorted by world
    rm.check_slices(np.concatenate([box[None], box[None]]), np.stack([vel, vel]), 0.0, 0.1, 4, host=True)
    with pytest.raises(_lib.ArmourError) as ei:
        rm.arrival(0.1, 0, 0, host=True, x_world=[1, 0], x_u=[3, 3], x_v=[0, 0], x_len=[0.1, 0.1], x_mask=[15, 15])
    assert ei.value.code == _lib.EINVAL
    rm.close()
