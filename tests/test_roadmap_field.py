"""Cost-to-go fields of a roadmap (include/armour_hip.h armour_roadmap_field / armour_roadmap_descend, armour_amd/roadmap.py).

The field is restated below in numpy and heapq, adding in the library's order: a wrapped distance is accumulated joint by joint, the
seeds are the goal's connect_k nearest free nodes whose connecting edge is free by the numpy edge rule of test_roadmap.py, Dijkstra
runs from the seeds with one fp64 add per relaxation, and `next` follows the header's rule.  x -> fl(x + len) is monotone and never
decreases x, so the field is unique as a set of doubles whatever the relaxation order: the device is held to bit equality.
CPU tests: the exports, and the determinism claim itself.  GPU tests: the device against the restatement, and descend() against plan()."""
import ctypes as C
import heapq

import numpy as np
import pytest

from test_roadmap import _limits, _reference_obstacles, _robot, _wall_world, config_clearance, edge_free_np, geometry, link_boxes, robot_dict, wrap

NEXT_GOAL = -2
SOLVE = dict(tolerance=1e-7, max_iterations=100)      # tests/test_reference_scenes.py


# ----------------------------------------------------------------------------------------------------------- restatement
def wrapped_len(A, B, cont):
    """The library's wrapped distance of A -> B ([K,n] each, or broadcastable): acc += d * d joint by joint, then one square root."""
    A, B = np.broadcast_arrays(np.atleast_2d(np.asarray(A, dtype=np.float64)), np.atleast_2d(np.asarray(B, dtype=np.float64)))
    acc = np.zeros(A.shape[0])
    for j in range(A.shape[1]):
        d = B[:, j] - A[:, j]
        if cont[j]:
            d = wrap(d)
        acc = acc + d * d
    return np.sqrt(acc)


def dijkstra(N, edges, length, free, seed):
    """cost [N] from seed {node: value} over the edges with free[e], by heapq; one fp64 add per relaxation."""
    adj = [[] for _ in range(N)]
    for e in np.flatnonzero(free):
        a, b = int(edges[e][0]), int(edges[e][1])
        adj[a].append((b, float(length[e])))
        adj[b].append((a, float(length[e])))
    cost = np.full(N, np.inf)
    heap = []
    for v, s in seed.items():
        cost[v] = s
        heap.append((s, v))
    heapq.heapify(heap)
    while heap:
        d, v = heapq.heappop(heap)
        if d > cost[v]:
            continue
        for u, l in adj[v]:
            nd = d + l
            if nd < cost[u]:
                cost[u] = nd
                heapq.heappush(heap, (nd, u))
    return cost, adj


def successors(cost, adj, seed):
    """-1 unreachable, NEXT_GOAL where the seed attains the cost, else the smallest neighbour u with fl(cost[u] + len) == cost[v] and
    cost[u] < cost[v] (the header's rule; every roadmap here has lengths far above an ulp of the costs, so some u always qualifies)."""
    nxt = np.full(cost.size, -1, dtype=np.int32)
    for v in range(cost.size):
        if not np.isfinite(cost[v]):
            continue
        if v in seed and seed[v] == cost[v]:
            nxt[v] = NEXT_GOAL
            continue
        hit = [u for u, l in adj[v] if cost[u] + l == cost[v] and cost[u] < cost[v]]
        assert hit, v
        nxt[v] = min(hit)
    return nxt


def seeds_np(g, nodes, node_free, goal, obs, step, k, self_rule=None):
    """{node: wrapped distance goal -> node} of the goal's k nearest free nodes (ties: the smaller index) whose edge is free by the
    numpy rule.  No edge may be so close to an obstacle that rounding decides it."""
    idx = np.flatnonzero(node_free)
    dist = wrapped_len(goal[None], nodes[idx], g["cont"])
    seed = {}
    for o in np.lexsort((idx, dist))[:k]:
        free, cl = edge_free_np(g, goal, nodes[idx[o]], obs, step)
        assert abs(cl) > 1e-9, cl
        if free and self_rule is not None:
            free, margin = self_rule(goal, nodes[idx[o]])
            assert margin > 1e-9, margin
        if free:
            seed[int(idx[o])] = float(dist[o])
    return seed


def field_np(g, nodes, edges, node_free, edge_free, goal, obs, step, k, self_rule=None):
    """(cost, next, reached, seed) of one world by the restated rule; the masks are the device's."""
    N = nodes.shape[0]
    length = wrapped_len(nodes[edges[:, 0]], nodes[edges[:, 1]], g["cont"]) if len(edges) else np.zeros(0)
    seed = seeds_np(g, nodes, node_free, goal, obs, step, k, self_rule)
    cost, adj = dijkstra(N, edges, length, edge_free, seed)
    return cost, successors(cost, adj, seed), int(np.isfinite(cost).sum()), seed


def assert_field(f, w, want, tag):
    cost, nxt, reached, _ = want
    assert np.array_equal(f["cost"][w], cost), (tag, w, int((f["cost"][w] != cost).sum()))           # infinities included
    assert np.array_equal(f["next"][w], nxt), (tag, w)
    assert f["reached"][w] == reached and f["sweeps"][w] >= 1, (tag, w, f["reached"][w], reached, f["sweeps"][w])


# ----------------------------------------------------------------------------------------------------------- CPU
def test_the_library_exports_the_field_entries_and_refuses_a_null_handle():
    from armour_amd import _lib
    L = _lib.load()
    for name in ("armour_roadmap_field", "armour_roadmap_descend"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    goals = np.zeros(7)
    dp = C.POINTER(C.c_double)
    assert L.armour_roadmap_field(None, goals.ctypes.data_as(dp), 8, None, None, None, None, None) == _lib.EINVAL
    pts = C.c_int32(5)
    assert L.armour_roadmap_descend(None, 0, goals.ctypes.data_as(dp), 8, 0, None, C.byref(pts), None) == _lib.EINVAL
    from armour_amd import roadmap
    assert roadmap.NEXT_GOAL == NEXT_GOAL
    for name in ("RoadmapFieldHLP", "field_hlps"):
        assert hasattr(roadmap, name)
    assert hasattr(roadmap.Roadmap, "field") and hasattr(roadmap.Roadmap, "descend")


def test_in_place_sweeps_in_any_order_equal_heap_dijkstra_bit_for_bit():
    """The determinism claim: pull sweeps, in place, nodes in a fresh random order every sweep, end at the doubles of a heap Dijkstra --
    with lengths spread from far below one ulp of the costs to well above them, masked edges and several seeds."""
    rng = np.random.default_rng(17)
    absorbed = 0
    for trial in range(60):
        N = int(rng.integers(4, 40))
        E = int(rng.integers(1, 4 * N))
        edges = rng.integers(0, N, size=(E, 2))
        length = 10.0 ** rng.uniform(-18, 1, E)
        length[rng.random(E) < 0.05] = 0.0
        free = rng.random(E) < 0.8
        seed = {int(v): float(10.0 ** rng.uniform(-3, 1)) for v in rng.choice(N, size=int(rng.integers(1, 4)), replace=False)}
        want, adj = dijkstra(N, edges, length, free, seed)
        cost = np.full(N, np.inf)
        for v, s in seed.items():
            cost[v] = s
        sweeps = 0
        while True:
            changed = False
            for v in rng.permutation(N):
                best = cost[v]
                for u, l in adj[v]:
                    d = cost[u] + l
                    if d < best:
                        best = d
                if best < cost[v]:
                    cost[v] = best
                    changed = True
            sweeps += 1
            assert sweeps <= N + 1, (trial, sweeps)        # the kernel's cap is never the reason to stop
            if not changed:
                break
        assert np.array_equal(cost, want), trial
        absorbed += sum(1 for v in range(N) for u, l in adj[v] if l > 0 and np.isfinite(want[u]) and want[u] + l == want[u])
    assert absorbed > 50, absorbed                         # sums that a length below one ulp left unchanged took part


# ----------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def kinova():
    robot = _robot("kinova")
    return robot, geometry(robot_dict(robot)), _limits(robot)


@pytest.fixture(scope="module")
def worlds16():
    """The first 16 reference worlds: obstacles [16,O,12] and their own goals [16,7]."""
    from armour_amd.scenes import reference_worlds
    ws = reference_worlds()[:16]
    return _reference_obstacles()["obstacles"][:16], np.stack([np.asarray(p["goal"], dtype=np.float64) for _, p in ws])


def _roadmap(kinova, N, seed, step=0.1):
    from armour_amd.roadmap import Roadmap, uniform_roadmap
    robot, g, (lb, ub, cont) = kinova
    nodes, edges = uniform_roadmap(N, 2.5, 4, seed, lb, ub, cont)
    return Roadmap(robot, nodes, edges, continuous=cont, edge_step=step), nodes, edges


@pytest.mark.gpu
def test_field_parity_with_the_restatement_without_and_with_the_self_masks(kinova, worlds16):
    from armour_amd.self_check import calibrate_shrink
    from test_self_check import _reference_configs, edge_self_free_np
    robot, g, _ = kinova
    obs, goals = worlds16
    step = 0.1
    rm, nodes, edges = _roadmap(kinova, 800, 5, step)
    v = rm.check(obs)
    f = rm.field(goals, connect_k=8)
    want = [field_np(g, nodes, edges, v["node_free"][w], v["edge_free"][w], goals[w], obs[w], step, 8) for w in range(16)]
    for w in range(16):
        assert_field(f, w, want[w], "plain")
    reached = np.array([x[2] for x in want])
    assert reached.max() > 400 and (f["sweeps"] > 1).any(), (reached, f["sweeps"])            # the fields are not trivial
    assert any(np.isinf(x[0]).any() for x in want)
    # the same worlds with the self masks: the graph is what is free in both
    shrink = calibrate_shrink(robot, _reference_configs(), host=True)
    s = rm.check_self(shrink=shrink)
    rm.use_self(True)
    f2 = rm.field(goals, connect_k=8)
    rule = lambda a, b: edge_self_free_np(g, a, b, step, shrink=shrink)
    for w in range(16):
        both = field_np(g, nodes, edges, v["node_free"][w] & s["node_free"], v["edge_free"][w] & s["edge_free"], goals[w], obs[w], step, 8, rule)
        assert_field(f2, w, both, "self")
    assert not s["edge_free"].all() and not np.array_equal(f["cost"], f2["cost"])               # the self masks took edges away
    rm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 1023, 1024, 1025])
def test_field_at_the_block_stride_edges(kinova, worlds16, N):
    """One node and no edge; one node short of, exactly, and one node past a thread each."""
    from armour_amd.scenes import FAR_BOX
    robot, g, _ = kinova
    obs, goals = worlds16
    step = 0.1
    rm, nodes, edges = _roadmap(kinova, N, 31, step)
    assert (rm.E == 0) == (N == 1)
    two = np.stack([np.tile(FAR_BOX, (obs.shape[1], 1)), obs[0]])
    gl = np.stack([goals[0], goals[0]])
    v = rm.check(two)
    f = rm.field(gl, connect_k=8)
    for w in range(2):
        assert_field(f, w, field_np(g, nodes, edges, v["node_free"][w], v["edge_free"][w], gl[w], two[w], step, 8), N)
    assert v["edge_free"][0].all() and f["reached"][0] >= 1
    rm.close()


@pytest.mark.gpu
def test_a_shuffled_chain_takes_many_sweeps_and_sums_from_the_goal(kinova):
    from armour_amd.roadmap import Roadmap
    from armour_amd.scenes import FAR_BOX
    robot, g, (lb, ub, cont) = kinova
    K, delta = 300, 0.01
    base = np.array([-1.5, 0.6, 0.0, 1.2, 0.0, 0.6, 0.0])
    perm = np.random.default_rng(4).permutation(K)           # node perm[i] is the chain's i-th configuration
    nodes = np.zeros((K, 7))
    for i in range(K):
        nodes[perm[i]] = base
        nodes[perm[i], 0] += i * delta
    edges = np.array([[perm[i], perm[i + 1]] for i in range(K - 1)], dtype=np.int32)
    goal = base.copy()
    goal[0] -= 0.5 * delta
    rm = Roadmap(robot, nodes, edges, continuous=cont, edge_step=0.1)
    v = rm.check(FAR_BOX[None])
    assert v["node_free"].all() and v["edge_free"].all()
    f = rm.field(goal, connect_k=1)
    length = wrapped_len(nodes[edges[:, 0]], nodes[edges[:, 1]], cont)
    want = np.zeros(K)
    acc = float(wrapped_len(goal[None], nodes[perm[0]][None], cont)[0])
    for i in range(K):
        want[perm[i]] = acc
        if i < K - 1:
            acc = acc + float(length[i])
    assert np.array_equal(f["cost"][0], want)
    assert f["next"][0][perm[0]] == NEXT_GOAL and np.array_equal(f["next"][0][perm[1:]], perm[:-1])
    assert f["reached"][0] == K and 1 < f["sweeps"][0] <= K + 1, f["sweeps"]
    path, total = rm.descend(0, nodes[perm[K - 1]], connect_k=1)              # nothing in the way: the direct edge, not the chain
    assert path.shape == (2, 7) and total == wrapped_len(nodes[perm[K - 1]][None], goal[None], cont)[0]
    rm.close()


@pytest.mark.gpu
def test_degenerate_worlds(kinova, worlds16):
    from armour_amd.roadmap import Roadmap
    from armour_amd.scenes import FAR_BOX
    robot, g, (lb, ub, cont) = kinova
    obs, goals = worlds16
    step = 0.1
    rm, nodes, edges = _roadmap(kinova, 200, 8, step)
    goal = goals[0]
    _, _, x = link_boxes(g, goal[None])
    c = x[0, 5]
    inside = np.array([c[0], c[1], c[2], 0.06, 0, 0, 0, 0.06, 0, 0, 0, 0.06])       # a box about the goal's forearm
    assert config_clearance(g, goal[None], inside[None])[0] < -1e-3
    v = rm.check(np.stack([inside[None], FAR_BOX[None]]))
    assert v["node_free"][0].any()
    f = rm.field(np.stack([goal, goal]), connect_k=8)
    assert np.isinf(f["cost"][0]).all() and (f["next"][0] == -1).all() and f["reached"][0] == 0 and f["sweeps"][0] >= 1
    assert f["reached"][1] > 0
    assert rm.descend(0, nodes[np.flatnonzero(v["node_free"][0])[0]]) == (None, np.inf)
    f0 = rm.field(np.stack([goal, goal]), connect_k=0)                              # no seed in any world
    assert np.isinf(f0["cost"]).all() and (f0["next"] == -1).all() and (f0["reached"] == 0).all()
    rm.close()
    bare = Roadmap(robot, nodes, np.zeros((0, 2)), continuous=cont, edge_step=step)  # E = 0: the seeds and nothing else
    v = bare.check(obs[:2])
    f = bare.field(goals[:2], connect_k=8)
    for w in range(2):
        want = field_np(g, nodes, np.zeros((0, 2), dtype=np.int32), v["node_free"][w], v["edge_free"][w], goals[w], obs[w], step, 8)
        assert_field(f, w, want, "bare")
        assert set(np.flatnonzero(f["next"][w] == NEXT_GOAL)) == set(want[3]) and f["reached"][w] == len(want[3])
    bare.close()


@pytest.mark.gpu
def test_edges_that_join_equal_costs_never_make_the_successors_cycle(kinova):
    """A self loop and a pair of duplicate nodes (both of length 0; armour_roadmap_create accepts them): each end of such an edge attains
    the other's cost, so without the rule's cost[u] < cost[v] the two would name each other.  Costs fall strictly along next[]."""
    from armour_amd.roadmap import Roadmap
    from armour_amd.scenes import FAR_BOX
    robot, g, (lb, ub, cont) = kinova
    c = np.array([-1.5, 0.6, 0.0, 1.2, 0.0, 0.6, 0.0])
    a = c.copy()
    a[0] += 0.3
    goal = c.copy()
    goal[0] -= 0.05
    nodes = np.stack([a, a, c])                                            # 0 and 1 are one configuration
    edges = np.array([[0, 0], [0, 1], [1, 2]], dtype=np.int32)
    rm = Roadmap(robot, nodes, edges, continuous=cont, edge_step=0.1)
    v = rm.check(FAR_BOX[None])
    assert v["edge_free"].all()
    f = rm.field(goal, connect_k=1)                                        # the one seed is node 2
    cost, nxt = f["cost"][0], f["next"][0]
    d2 = wrapped_len(goal[None], c[None], cont)[0]
    d12 = wrapped_len(a[None], c[None], cont)[0]
    assert np.array_equal(cost, [d2 + d12, d2 + d12, d2]) and f["reached"][0] == 3
    assert nxt[2] == NEXT_GOAL and nxt[1] == 2                             # by the unrestricted rule node 1 would name node 0, and 0 itself
    assert nxt[0] == -1                                                    # the stated limitation: only a length-0 edge attains its cost
    for s in range(3):                                                     # every walk ends, at the goal or at -1, with falling costs
        w, steps = s, 0
        while nxt[w] >= 0:
            assert cost[nxt[w]] < cost[w]
            w, steps = nxt[w], steps + 1
            assert steps <= 3
    rm.close()


@pytest.mark.gpu
def test_field_refuses_a_goal_count_other_than_the_last_checks_worlds(kinova, worlds16):
    """The library takes W from the last check and has no argument for it, so the wrapper must not size its outputs from any other count."""
    obs, goals = worlds16
    rm, nodes, edges = _roadmap(kinova, 100, 3)
    rm.check(obs)
    for bad in (goals[0], goals[:1], goals[:15], np.concatenate([goals, goals[:1]])):
        with pytest.raises(ValueError):
            rm.field(bad)
    f = rm.field(goals)                                                    # a refused call changes nothing
    assert f["cost"].shape == (16, 100)
    rm.check(obs[:1])
    with pytest.raises(ValueError):
        rm.field(goals)
    assert np.array_equal(rm.field(goals[0])["cost"][0], f["cost"][0])     # [n] is one world's goal
    rm.close()


@pytest.mark.gpu
def test_a_batch_of_fields_equals_one_world_at_a_time(kinova, worlds16):
    obs, goals = worlds16
    rm, nodes, edges = _roadmap(kinova, 800, 9)
    rm.check(obs)
    f = rm.field(goals)
    for w in range(16):
        rm.check(obs[w:w + 1])
        one = rm.field(goals[w])
        assert np.array_equal(one["cost"][0], f["cost"][w]) and np.array_equal(one["next"][0], f["next"][w]), w
        assert one["reached"][0] == f["reached"][w]
    rm.close()


@pytest.fixture(scope="module")
def wall(kinova, worlds16):
    """The roadmap of test_roadmap.py's wall test (300 uniform nodes and the hand-placed detour) checked against the wall world, the empty
    world and the 16 reference worlds; goals: the wall world's for the first two, then every world's own."""
    from armour_amd.roadmap import Roadmap, uniform_roadmap
    from armour_amd.scenes import FAR_BOX, pad_obstacles
    robot, g, (lb, ub, cont) = kinova
    obs, goals = worlds16
    start, goal, wall_box, chain = _wall_world(g)
    rnd, redges = uniform_roadmap(300, 2.0, 4, 2, lb, ub, cont)
    nodes = np.vstack([rnd, np.array(chain)])
    k0 = len(rnd)
    edges = np.vstack([redges, np.array([[k0 + i, k0 + i + 1] for i in range(len(chain) - 1)], dtype=np.int32)])
    step = 0.05
    rm = Roadmap(robot, nodes, edges, continuous=cont, edge_step=step)
    O = obs.shape[1]
    worlds = np.concatenate([np.stack([pad_obstacles(wall_box[None], O), pad_obstacles(FAR_BOX[None], O)]), obs])
    gl = np.concatenate([np.stack([goal, goal]), goals])
    yield dict(rm=rm, nodes=nodes, edges=edges, step=step, worlds=worlds, goals=gl, start=start, goal=goal, wall_box=wall_box)
    rm.close()


def _path_length(path, cont):
    return float(wrapped_len(path[:-1], path[1:], cont).sum())


@pytest.mark.gpu
def test_descend_against_plan(kinova, wall):
    robot, g, (lb, ub, cont) = kinova
    rm, worlds, goals, step = wall["rm"], wall["worlds"], wall["goals"], wall["step"]
    rm.check(worlds)
    rm.field(goals, connect_k=4)
    rng = np.random.default_rng(12)
    cases = [(0, wall["start"])] + [(0, wall["start"] + rng.uniform(-0.02, 0.02, 7)) for _ in range(10)]      # behind the wall: detours
    while len(cases) < 61:                                                                                     # 50 free starts in the 16 worlds
        w = 2 + len(cases) % 16
        q = lb + (ub - lb) * rng.random(7)
        if config_clearance(g, q[None], worlds[w])[0] > 1e-6:
            cases.append((w, q))
    found = detours = 0
    for w, q in cases:
        want = rm.plan(w, q, goals[w], connect_k=4)
        path, total = rm.descend(w, q, connect_k=4)
        assert (path is None) == (want is None), w
        if path is None:
            assert total == np.inf
            continue
        found += 1
        detours += len(path) > 2
        assert np.array_equal(path[0], q) and np.array_equal(path[-1], goals[w])
        for a, b in zip(path[:-1], path[1:]):
            free, cl = edge_free_np(g, a, b, worlds[w], step)
            assert abs(cl) > 1e-9, (w, cl)                                # no edge so close to an obstacle that rounding decides it
            assert free, (w, cl)
        la, lb_ = _path_length(path, cont), _path_length(want, cont)
        assert abs(la - lb_) <= 1e-9 * lb_, (w, la, lb_)                  # both optimal over one graph: summation order and ties only
        assert abs(total - la) <= 1e-9 * la, (w, total, la)
    assert found >= 20 and detours >= 3, (found, detours)                 # the comparison is not of direct edges alone
    path, total = rm.descend(0, wall["start"], connect_k=4)
    assert len(path) > 2                                                  # around the wall
    direct, total = rm.descend(1, wall["start"], connect_k=4)             # the empty world: the direct two-point path
    assert direct.shape == (2, 7) and np.array_equal(direct[0], wall["start"]) and np.array_equal(direct[1], wall["goal"])
    assert total == wrapped_len(wall["start"][None], wall["goal"][None], cont)[0]


@pytest.mark.gpu
def test_state_rules(kinova, worlds16):
    from armour_amd import _lib
    obs, goals = worlds16
    rm, nodes, edges = _roadmap(kinova, 100, 3)

    def estate(call):
        with pytest.raises(_lib.ArmourError) as ei:
            call()
        assert ei.value.code == _lib.ESTATE

    estate(lambda: rm.field(goals[:2]))                    # before a check
    rm.check(obs[:2])
    estate(lambda: rm.descend(0, nodes[0]))                # before a field
    rm.field(goals[:2])
    rm.descend(0, nodes[0])
    rm.check(obs[:2])
    estate(lambda: rm.descend(0, nodes[0]))                # after a new check
    rm.field(goals[:2])
    rm.check_self()
    estate(lambda: rm.descend(0, nodes[0]))                # after a self check
    rm.field(goals[:2])
    rm.use_self(True)
    estate(lambda: rm.descend(0, nodes[0]))                # after a use_self change
    rm.field(goals[:2])
    rm.descend(1, nodes[0])
    with pytest.raises(_lib.ArmourError) as ei:
        rm.descend(2, nodes[0])
    assert ei.value.code == _lib.EINVAL
    with pytest.raises(_lib.ArmourError) as ei:
        rm.field(np.full((2, 7), np.nan))
    assert ei.value.code == _lib.EINVAL
    rm.descend(0, nodes[0])                                # a call refused for its arguments changes nothing
    fresh, _, _ = _roadmap(kinova, 100, 3)
    fresh.check(obs[:2])
    fresh.use_self(True)
    estate(lambda: fresh.field(goals[:2]))                 # self masks on and no self check yet
    fresh.close()
    rm.close()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_the_field_hlp_agrees_with_the_search_hlp_and_drives_the_trials(kinova, wall):
    from armour_amd.roadmap import RoadmapFieldHLP, RoadmapHLP, field_hlps
    from armour_amd.scenes import reference_worlds, straight_line_waypoint
    from armour_amd.trials import run_trials
    robot, g, (lb, ub, cont) = kinova
    rm, start, goal = wall["rm"], wall["start"], wall["goal"]
    ref = reference_worlds()
    worlds = [("wall", dict(q0=start, goal=goal, obstacles=wall["wall_box"][None], lookahead=0.1)), ref[0], ref[3]]
    make = field_hlps(rm, worlds, connect_k=4)
    hlp = make(0, None)
    assert isinstance(hlp, RoadmapFieldHLP)
    w1 = hlp.get_waypoint(start, 0.1)
    w0 = RoadmapHLP(rm, goal, world=0, connect_k=4).get_waypoint(start, 0.1)
    assert np.abs(w1 - w0).max() <= 1e-12                                             # the detour is the unique shortest path
    assert np.abs(w1 - straight_line_waypoint(start, goal, 0.1)).max() > 1e-3
    res = run_trials(worlds, hlp=make, T=100, solve_options=SOLVE, max_iterations=10)
    records = 0
    for i, wr in enumerate(res["worlds"]):
        assert wr["outcome"] != "collision", (wr["name"], wr["outcome"])
        la = worlds[i][1].get("lookahead", 1.0)
        for rec in wr["records"]:
            assert np.array_equal(rec["q_des"], make(i, None).get_waypoint(rec["q0"].copy(), la)), (wr["name"], rec["iteration"])
            records += 1
    assert records >= 3
