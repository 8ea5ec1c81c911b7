"""Batched workspace RRT*, CPU half (include/armour_hip.h armour_ws_tree_plan / armour_ws_tree_plan_host, armour_amd/ws_planner.py).

The rule -- point and edge tests, samples, nearest node, steer, candidates, parent choice, rewiring, cost re-derivation, best node -- is
restated below in numpy from the header's text, on top of the pair test of test_roadmap.py, and the library's host twin has to reproduce it
bit for bit: a node is a point and a test is an axis-aligned box against an obstacle, so no trigonometry is involved and the two can only
part where a clearance is within rounding of zero; every comparison first asserts that the RESTATEMENT's own margin is above 1e-9.  Then the
invariants of every returned tree (from the rule, not from the twin), the prefix property, rewiring, the statuses, the argument rules, path
capacity, batching, and the HLP layer.  The device is compared to the host twin in test_ws_tree_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from test_roadmap import _robot, dot3, pair_clearance
from test_tree_plan import _same_bits, _with, u
from test_trials import ScriptedPlanner

MARGIN = 1e-9
MAX_SEGMENTS = 1024
LB, UB = np.array([-0.1, -0.7, -0.1]), np.array([1.1, 0.7, 1.1])
START, GOAL = np.array([0.1, -0.3, 0.2]), np.array([0.9, 0.3, 0.8])
OPTS = dict(step=0.1, edge_step=0.01, rewire_radius=0.2, goal_rate=0.1, buffer=0.0, goal_tol=0.01, max_iterations=250, max_nodes=512)


def _box(c, h):
    return np.array([c[0], c[1], c[2], h[0], 0, 0, 0, h[1], 0, 0, 0, h[2]], dtype=np.float64)


def wall_with_window():
    """A wall at x = 0.5 over y in [-0.6, 0.6], z in [0, 1] with a 0.2 x 0.2 window about (0.5, 0, 0.5), and one box that is NOT axis-aligned
    behind it (the general obstacle [c g1 g2 g3])."""
    c, s = np.cos(0.5), np.sin(0.5)
    tilted = np.array([0.8, -0.3, 0.4, 0.1 * c, 0.1 * s, 0, -0.05 * s, 0.05 * c, 0, 0, 0, 0.15])
    return np.stack([_box((0.5, -0.35, 0.5), (0.02, 0.25, 0.5)), _box((0.5, 0.35, 0.5), (0.02, 0.25, 0.5)), _box((0.5, 0.0, 0.2), (0.02, 0.1, 0.2)),
                     _box((0.5, 0.0, 0.8), (0.02, 0.1, 0.2)), tilted])


FAR = _box((0.0, 0.0, -50.0), (0.005, 0.005, 0.005))
OPEN = FAR[None]


# ----------------------------------------------------------------------------------------------------------- numpy restatement
def boxes_clearance(x, h, Z):
    """[K]: per box (centre x [K,3], axes e_0 e_1 e_2, half-sizes h [K,3]) the minimum over the obstacles of the pair clearance"""
    if np.asarray(Z).size == 0:
        return np.full(len(x), np.inf)
    U = np.broadcast_to(np.eye(3), (len(x), 3, 3))
    return pair_clearance(np.asarray(x), U, np.asarray(h), Z).min(-1)


def diff(a, b):
    D = b - a
    return D, float(dot3(D, D))


def edge_boxes(a, b, es, buf):
    D, acc = diff(a, b)
    S = int(min(MAX_SEGMENTS, max(1.0, np.ceil(np.sqrt(acc) / es))))
    ts = (2.0 * np.arange(S) + 1.0) / float(2 * S)
    return a + ts[:, None] * D, np.broadcast_to(buf + np.abs(D) / float(2 * S), (S, 3))


def plan_ws_np(Z, start, goal, seed, lb=LB, ub=UB, init=None, step=0.1, edge_step=0.01, rewire_radius=0.2, goal_rate=0.1, buffer=0.0, goal_tol=0.01,
               max_iterations=250, max_nodes=512):
    """-> dict(status, iterations, count, rewires, chain_kept, nodes, parent, cost, path, path_cost, goal_dist, margin, most_rewires),
    the header's run of one world"""
    margin = [np.inf]

    def edges_free(pairs):
        """the verdicts of the edges a -> b of `pairs`, all boxes in one call; the margin over sub-segments 0 .. min(m, S - 1) of each"""
        bx = [edge_boxes(a, b, edge_step, buffer) for a, b in pairs]
        cl = boxes_clearance(np.concatenate([x for x, _ in bx]), np.concatenate([h for _, h in bx]), Z)
        out, at = [], 0
        for x, _ in bx:
            c = cl[at:at + len(x)]
            at += len(x)
            hit = np.flatnonzero(~(c > 0))
            m = int(hit[0]) if hit.size else len(x)
            margin[0] = min(margin[0], np.abs(c[:min(m, len(x) - 1) + 1]).min())
            out.append(m == len(x))
        return out

    out = dict(status=2, iterations=0, count=0, rewires=0, chain_kept=0, nodes=[], parent=[], cost=[], path=None, path_cost=0.0,
               goal_dist=float(np.sqrt(diff(start, goal)[1])), most_rewires=0)
    cl = boxes_clearance(start[None], np.full((1, 3), buffer), Z)[0]
    margin[0] = min(margin[0], abs(cl))
    if not cl > 0:
        return dict(out, margin=margin[0])
    nodes, par, ln, cost = [start.copy()], [-1], [0.0], [0.0]
    kept = 0
    for c in ([] if init is None else init):
        if len(nodes) >= max_nodes or not edges_free([(nodes[-1], c)])[0]:
            break
        d = float(np.sqrt(diff(nodes[-1], c)[1]))
        par.append(len(nodes) - 1)
        ln.append(d)
        cost.append(cost[-1] + d)
        nodes.append(np.array(c, dtype=np.float64))
        kept += 1
    rr2 = rewire_radius * rewire_radius
    iterations, rewires, most = max_iterations, 0, 0
    for i in range(max_iterations):
        if len(nodes) >= max_nodes:
            iterations = i
            break
        if u(seed, i, 3) < goal_rate:
            qr = goal.copy()
        else:
            qr = np.array([lb[j] + u(seed, i, j) * (ub[j] - lb[j]) for j in range(3)])
        X = np.stack(nodes)
        D = qr - X
        acc_all = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
        v = int(np.argmin(acc_all))                   # (the first of the smallest: the smaller index on a tie)
        acc = float(acc_all[v])
        if acc == 0.0:
            continue
        dist = np.sqrt(acc)
        qn = qr if dist <= step else X[v] + (step / dist) * D[v]
        Dn = qn - X
        acc_n = (Dn[:, 0] * Dn[:, 0] + Dn[:, 1] * Dn[:, 1]) + Dn[:, 2] * Dn[:, 2]
        cand = [c for c in range(len(nodes)) if acc_n[c] <= rr2 or c == v]
        free = [c for c, ok in zip(cand, edges_free([(X[c], qn) for c in cand])) if ok]
        if not free:
            continue
        d = {c: float(np.sqrt(acc_n[c])) for c in free}
        p = min(free, key=lambda c: (cost[c] + d[c], c))
        cost_qn = cost[p] + d[p]
        k = len(nodes)
        rewired = [c for c in free if c != p and cost_qn + d[c] < cost[c]]
        for c in rewired:
            par[c], ln[c] = k, d[c]
        nodes.append(qn)
        par.append(p)
        ln.append(d[p])
        cost.append(cost_qn)
        rewires += len(rewired)
        most = max(most, len(rewired))
        if rewired:
            cost = derive_costs(par, ln)
    X = np.stack(nodes)
    Dg = goal - X
    g2 = (Dg[:, 0] * Dg[:, 0] + Dg[:, 1] * Dg[:, 1]) + Dg[:, 2] * Dg[:, 2]
    g = np.sqrt(g2)
    within = [k for k in range(len(nodes)) if g[k] <= goal_tol]
    best = min(within, key=lambda k: (cost[k] + g[k], k)) if within else min(range(len(nodes)), key=lambda k: (g2[k], k))
    chain, x = [], best
    while x != -1:
        chain.append(nodes[x])
        x = par[x]
    return dict(status=1 if within else 0, iterations=iterations, count=len(nodes), rewires=rewires, chain_kept=kept, nodes=X, parent=par, cost=cost,
                path=np.stack(chain[::-1]), path_cost=cost[best], goal_dist=float(g[best]), margin=margin[0], most_rewires=most)


def derive_costs(par, ln):
    """cost_k = cost_parent(k) + len_k from the root down, by the definition (children after their parent, whatever their indices)"""
    kids = [[] for _ in par]
    for k, p in enumerate(par):
        if p >= 0:
            kids[p].append(k)
    cost, todo = [None] * len(par), [0]
    cost[0] = 0.0
    while todo:
        p = todo.pop()
        for k in kids[p]:
            cost[k] = cost[p] + ln[k]
            todo.append(k)
    assert None not in cost                           # every node hangs from the root: no cycle
    return cost


# ----------------------------------------------------------------------------------------------------------- helpers
def _plan(Z, seeds, host=True, starts=None, goals=None, **kw):
    from armour_amd.ws_planner import plan_workspace_trees
    Z = np.asarray(Z)
    Z = Z[None] if Z.ndim == 2 else Z
    W = Z.shape[0]
    o = dict(OPTS, lb=LB, ub=UB, trees=True)
    o.update(kw)
    return plan_workspace_trees(Z, np.stack([START] * W) if starts is None else starts, np.stack([GOAL] * W) if goals is None else goals, seeds, host=host, **o)


def assert_equals_restatement(res, w, ref):
    """world w of a plan_workspace_trees(trees=True) result against plan_ws_np's dict"""
    assert ref["margin"] > MARGIN, ref["margin"]
    got = (res.status[w], res.iterations[w], res.count[w], res.rewires[w], res.chain_kept[w])
    assert got == (ref["status"], ref["iterations"], ref["count"], ref["rewires"], ref["chain_kept"]), (got, ref)
    c = ref["count"]
    if c:
        assert _same_bits(res.nodes[w, :c], ref["nodes"]) and list(res.parent[w, :c]) == list(ref["parent"])
        assert _same_bits(res.node_cost[w, :c], np.array(ref["cost"]))
    assert (res.paths[w] is None) == (ref["path"] is None)
    if ref["path"] is not None:
        assert _same_bits(res.paths[w], ref["path"])
    assert _same_bits(res.path_cost[w], ref["path_cost"]) and _same_bits(res.goal_dist[w], ref["goal_dist"])


def assert_same_plans(a, wa, b, wb):
    """world wa of result a and world wb of result b (both with trees=True), bit for bit on every output"""
    for k in ("status", "iterations", "count", "rewires", "chain_kept"):
        assert getattr(a, k)[wa] == getattr(b, k)[wb], (k, getattr(a, k)[wa], getattr(b, k)[wb])
    c = a.count[wa]
    assert _same_bits(a.nodes[wa, :c], b.nodes[wb, :c]) and np.array_equal(a.parent[wa, :c], b.parent[wb, :c])
    assert _same_bits(a.node_cost[wa, :c], b.node_cost[wb, :c])
    assert _same_bits(a.path_cost[wa], b.path_cost[wb]) and _same_bits(a.goal_dist[wa], b.goal_dist[wb])
    assert (a.paths[wa] is None) == (b.paths[wb] is None)
    assert a.paths[wa] is None or _same_bits(a.paths[wa], b.paths[wb])


def assert_tree_invariants(res, w, Z, goal=GOAL, buffer=0.0, goal_tol=0.01):
    """What the rule promises of every returned tree, checked without the twin."""
    c = int(res.count[w])
    X, par, cost = res.nodes[w, :c], res.parent[w, :c], res.node_cost[w, :c]
    assert par[0] == -1 and cost[0] == 0.0 and ((par[1:] >= 0) & (par[1:] < c)).all()
    for k in range(c):                                # the root is reached within count steps: no cycle
        x, steps = k, 0
        while x != 0:
            x, steps = par[x], steps + 1
            assert steps < c, k
    for k in range(1, c):
        ln = np.sqrt(diff(X[par[k]], X[k])[1])
        assert cost[k] == cost[par[k]] + ln, k          # bit for bit
    t = (np.arange(200) + 0.5) / 200.0
    pts = np.concatenate([X[par[k]] + t[:, None] * (X[k] - X[par[k]]) for k in range(1, c)]) if c > 1 else X[:1]
    assert (boxes_clearance(pts, np.full(pts.shape, buffer), Z) > 0).all()          # the exact point rule on dense samples of every edge
    g2 = np.array([diff(X[k], goal)[1] for k in range(c)])
    g = np.sqrt(g2)
    within = np.flatnonzero(g <= goal_tol)
    best = min(within, key=lambda k: (cost[k] + g[k], k)) if within.size else min(range(c), key=lambda k: (g2[k], k))
    assert res.status[w] == (1 if within.size else 0)
    assert res.path_cost[w] == cost[best] and res.goal_dist[w] == g[best] and _same_bits(res.paths[w][-1], X[best]) and _same_bits(res.paths[w][0], X[0])


@pytest.fixture(scope="module")
def wall_refs():
    """The restatement's runs of the wall world, seeds 1, 2, 3, computed once and shared."""
    Z = wall_with_window()
    return Z, {seed: plan_ws_np(Z, START, GOAL, seed, **OPTS) for seed in (1, 2, 3)}


# ----------------------------------------------------------------------------------------------------------- the twin against the rule
def test_rrt_star_equals_the_restatement_and_rewires(wall_refs):
    Z, refs = wall_refs
    res = _plan(np.stack([Z] * 3), [1, 2, 3])
    assert (res.margin > MARGIN).all()
    for w, seed in enumerate((1, 2, 3)):
        assert_equals_restatement(res, w, refs[seed])
        assert_tree_invariants(res, w, Z)
        assert res.margin[w] == refs[seed]["margin"]
    # rewiring happened, and a rewired node hangs from a later one: the re-derivation is exercised
    assert (res.rewires > 0).all()
    assert any((res.parent[w, :res.count[w]] > np.arange(res.count[w])).any() for w in range(3))
    assert (res.status == 1).any()


def test_open_world_plain_rrt_and_buffer(wall_refs):
    Z, _ = wall_refs
    for seed in (1, 2, 3):
        ref = plan_ws_np(OPEN, START, GOAL, seed, **dict(OPTS, max_iterations=120))
        res = _plan(OPEN, [seed], max_iterations=120)
        assert_equals_restatement(res, 0, ref)
        assert_tree_invariants(res, 0, OPEN)
    for seed in (1, 2, 3):                            # plain RRT: no near set, no rewire
        o = dict(OPTS, rewire_radius=0.0, max_iterations=200)
        ref = plan_ws_np(Z, START, GOAL, seed, **o)
        res = _plan(Z, [seed], **{k: o[k] for k in ("rewire_radius", "max_iterations")})
        assert res.rewires[0] == 0
        assert_equals_restatement(res, 0, ref)
        assert_tree_invariants(res, 0, Z)
        assert (res.parent[0, :res.count[0]] < np.arange(res.count[0])).all()
    for seed in (1, 2, 3):                            # a buffer: the window (0.2 wide) is still open for a point grown by 0.03
        o = dict(OPTS, buffer=0.03, max_iterations=200)
        ref = plan_ws_np(Z, START, GOAL, seed, **o)
        res = _plan(Z, [seed], buffer=0.03, max_iterations=200)
        assert_equals_restatement(res, 0, ref)
        assert_tree_invariants(res, 0, Z, buffer=0.03)


def test_a_seeded_chain_ends_at_its_first_blocked_edge(wall_refs):
    Z, _ = wall_refs
    chain = np.array([[0.2, -0.2, 0.3], [0.4, 0.0, 0.5], [0.6, 0.3, 0.5], [0.8, 0.3, 0.7]])      # the third edge crosses the wall beside the window
    for seed in (1, 2, 3):
        ref = plan_ws_np(Z, START, GOAL, seed, init=chain, **dict(OPTS, max_iterations=60))
        res = _plan(Z, [seed], init=[chain], max_iterations=60)
        assert res.chain_kept[0] == 2 and list(res.parent[0, :3]) == [-1, 0, 1] and _same_bits(res.nodes[0, 1:3], chain[:2])
        assert_equals_restatement(res, 0, ref)
        assert_tree_invariants(res, 0, Z)
    through = np.array([[0.4, 0.0, 0.5], [0.6, 0.0, 0.5], GOAL])                                   # through the window: kept whole, REACHED at once
    res = _plan(Z, [1], init=[through], max_iterations=0)
    assert res.chain_kept[0] == 3 and res.status[0] == 1 and res.count[0] == 4 and _same_bits(res.paths[0], np.vstack([START[None], through]))
    assert_equals_restatement(res, 0, plan_ws_np(Z, START, GOAL, 1, init=through, **dict(OPTS, max_iterations=0)))
    res = _plan(Z, [1], init=[through], max_iterations=50, max_nodes=3)                            # a chain that fills the tree stops there
    assert res.chain_kept[0] == 2 and res.count[0] == 3 and res.iterations[0] == 0


def test_more_iterations_extend_the_same_tree_and_never_cost_more(wall_refs):
    """goal_tol = 0: only a node AT the goal counts, so path_cost is the smallest cost of such a node, and costs can only fall."""
    Z, _ = wall_refs
    fell = 0
    for seed in (1, 5, 6):
        runs = [_plan(Z, [seed], max_iterations=it, goal_tol=0.0) for it in (120, 160, 200, 250)]
        for a, b in zip(runs, runs[1:]):
            ca = a.count[0]
            assert b.count[0] >= ca and _same_bits(a.nodes[0, :ca], b.nodes[0, :ca])                 # the same first nodes (parents may be rewired later)
            if a.status[0] == 1:
                assert b.status[0] == 1 and b.path_cost[0] <= a.path_cost[0]
                fell += b.path_cost[0] < a.path_cost[0]
        assert runs[-1].status[0] == 1 and runs[-1].goal_dist[0] == 0.0
        assert_tree_invariants(runs[-1], 0, Z, goal_tol=0.0)
    assert fell >= 2                                                                                 # rewiring did shorten a found path


def test_the_three_statuses_and_a_full_tree(wall_refs):
    Z, _ = wall_refs
    inside = np.array([0.5, 0.35, 0.5])                                                           # inside the wall
    res = _plan(np.stack([Z] * 3), [1, 1, 1], starts=np.stack([START, inside, START]), goals=np.stack([GOAL, GOAL, inside]))
    assert list(res.status) == [1, 2, 0]
    assert res.count[1] == 0 and res.iterations[1] == 0 and res.paths[1] is None and res.path_cost[1] == 0.0 and res.rewires[1] == 0
    assert res.goal_dist[1] == np.sqrt(diff(inside, GOAL)[1])
    assert res.goal_dist[2] > 0.02 and res.iterations[2] == OPTS["max_iterations"]               # PARTIAL: the path to the node nearest the goal
    assert_tree_invariants(res, 2, Z, goal=inside)
    full = _plan(Z, [1], max_nodes=8)
    ref = plan_ws_np(Z, START, GOAL, 1, **dict(OPTS, max_nodes=8))
    assert full.count[0] == 8 and 7 <= full.iterations[0] < OPTS["max_iterations"]
    assert_equals_restatement(full, 0, ref)
    one = _plan(Z, [1], max_nodes=1)                                                              # the root alone
    assert one.count[0] == 1 and one.iterations[0] == 0 and one.status[0] == 0 and _same_bits(one.paths[0], START[None])
    none = _plan(Z, [1], max_iterations=0)
    assert none.count[0] == 1 and none.iterations[0] == 0 and none.path_cost[0] == 0.0


# ----------------------------------------------------------------------------------------------------------- the C ABI
def _raw(host, W=1, O=None, max_points=512, with_init=False, **kw):
    """armour_ws_tree_plan(_host) itself on W copies of the wall world (seeds 1 .. W), every argument replaceable -> (rc, points [W], path)"""
    from armour_amd import _lib
    L = _lib.load()
    rows = max(W, 1)
    Z = wall_with_window()
    a = dict(OPTS, lb=LB, ub=UB, obstacles=np.stack([Z] * rows), starts=np.stack([START] * rows), goals=np.stack([GOAL] * rows), max_init=2,
             init=np.tile(np.array([[0.2, -0.2, 0.3], [0.3, -0.2, 0.3]]), (rows, 1, 1)), init_count=np.full(rows, 2))
    a.update(kw)
    O = Z.shape[0] if O is None else O
    seeds = np.arange(1, rows + 1, dtype=np.uint64)
    ints = [np.zeros(rows, dtype=np.int32) for _ in range(5)]
    reals = [np.zeros(rows) for _ in range(2)]
    path = np.zeros((rows, max(max_points, 1), 3))
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lb, ub, obstacles, starts, goals, init = (np.ascontiguousarray(a[k], dtype=np.float64) for k in ("lb", "ub", "obstacles", "starts", "goals", "init"))
    init_count = np.ascontiguousarray(a["init_count"], dtype=np.int32)
    fn = L.armour_ws_tree_plan_host if host else L.armour_ws_tree_plan
    rc = fn(lb.ctypes.data_as(f64), ub.ctypes.data_as(f64), W, O, obstacles.ctypes.data_as(f64), starts.ctypes.data_as(f64), goals.ctypes.data_as(f64),
            seeds.ctypes.data_as(C.POINTER(C.c_uint64)), int(a["max_init"]), init.ctypes.data_as(f64) if with_init else None,
            init_count.ctypes.data_as(i32) if with_init else None, *(float(a[k]) for k in ("step", "edge_step", "rewire_radius", "goal_rate", "buffer", "goal_tol")),
            int(a["max_iterations"]), int(a["max_nodes"]), int(max_points), *(x.ctypes.data_as(i32) for x in ints), *(x.ctypes.data_as(f64) for x in reals),
            path.ctypes.data_as(f64), None, None, None, None, None)
    return rc, ints[2], path


@pytest.mark.parametrize("host", [False, True])
def test_bad_arguments_are_refused_before_a_device_is_touched(host):
    """The device entry too answers EINVAL, not EDEVICE, on a machine without a device: the checks come first."""
    from armour_amd import _lib
    Z = wall_with_window()
    bad = [dict(O=257, obstacles=np.zeros((1, 257, 12))), dict(W=-1), dict(max_nodes=0), dict(max_nodes=_lib.WS_MAX_NODES + 1), dict(max_iterations=-1),
           dict(max_iterations=_lib.TREE_MAX_ITERATIONS + 1), dict(max_points=-1)]
    for k in ("step", "edge_step"):
        bad += [{k: 0.0}, {k: -0.1}, {k: np.nan}, {k: np.inf}]
    for k in ("rewire_radius", "buffer", "goal_tol"):
        bad += [{k: -1e-3}, {k: np.nan}, {k: np.inf}]
    bad += [dict(goal_rate=-0.1), dict(goal_rate=1.1), dict(goal_rate=np.nan)]
    bad += [dict(lb=_with(LB, 1, UB[1] + 0.1)), dict(lb=_with(LB, 2, -np.inf)), dict(ub=_with(UB, 0, np.nan)), dict(starts=_with(START[None], 1, np.nan)),
            dict(goals=_with(GOAL[None], 2, np.inf)), dict(obstacles=_with(Z[None], 7, np.nan))]
    bad += [dict(step=0.1, rewire_radius=0.0, edge_step=0.1 / (_lib.WS_MAX_SEGMENTS + 1)), dict(rewire_radius=1.0, edge_step=1.0 / (_lib.WS_MAX_SEGMENTS + 1))]      # too many sub-segments
    for kw in bad:
        rc, _, _ = _raw(host, **kw)
        assert rc == _lib.EINVAL, kw
    chain = np.array([[[0.2, -0.2, 0.3], [0.3, -0.2, 0.3]]])
    bad_init = [dict(init_count=[3]), dict(init_count=[-1]), dict(max_init=0), dict(init=_with(chain, 4, np.nan)), dict(init=_with(chain, 3, 20.0))]    # the last: a 20 m chain edge
    for kw in bad_init:
        rc, _, _ = _raw(host, with_init=True, **kw)
        assert rc == _lib.EINVAL, kw
    if host:
        rc, _, _ = _raw(True, with_init=True, init=_with(chain, 4, np.nan), init_count=[1])       # the padding of a chain is not read
        assert rc == _lib.OK
    rc, _, _ = _raw(host, W=0)                         # no world: a success that does nothing, with or without a device
    assert rc == _lib.OK
    if host:
        rc, _, _ = _raw(True, step=0.1, rewire_radius=0.05, edge_step=0.1 / _lib.WS_MAX_SEGMENTS, max_iterations=3)   # at the cap: accepted
        assert rc == _lib.OK


def test_a_path_longer_than_max_points_is_ecapacity_with_the_points_complete():
    from armour_amd import _lib
    rc, points, path = _raw(True, W=3)
    assert rc == _lib.OK and (points > 2).all() and len(set(points)) > 1
    rc2, points2, path2 = _raw(True, W=3, max_points=int(points.max()) - 1)
    assert rc2 == _lib.ECAPACITY and np.array_equal(points, points2)
    for w in range(3):
        if points[w] == points.max():
            assert not path2[w].any()                                                   # unwritten
        else:
            assert _same_bits(path2[w, :points[w]], path[w, :points[w]])
    rc3, points3, path3 = _raw(True, W=3, max_points=int(points.max()))
    assert rc3 == _lib.OK and all(_same_bits(path3[w, :points[w]], path[w, :points[w]]) for w in range(3))


def test_a_batch_of_four_equals_four_calls(wall_refs):
    Z, _ = wall_refs
    obs = np.stack([Z] * 3 + [np.vstack([FAR[None]] * Z.shape[0])])
    seeds = [1, 2, 3, 1]
    batch = _plan(obs, seeds)
    for w in range(4):
        one = _plan(obs[w:w + 1], [seeds[w]])
        assert_same_plans(batch, w, one, 0)
        assert one.margin[0] == batch.margin[w]
    assert len({int(c) for c in batch.count[:3]} | {float(c) for c in batch.path_cost[:3]}) > 2     # the seeds matter


# ----------------------------------------------------------------------------------------------------------- the HLP layer
def test_waypoint_along_points_against_a_direct_restatement():
    from armour_amd.ws_planner import waypoint_along_points
    rng = np.random.default_rng(5)
    path = np.cumsum(rng.uniform(-0.2, 0.3, (7, 3)), 0)
    path = np.vstack([path[:3], path[2:]])            # a repeated vertex: a segment of length zero
    seg = np.linalg.norm(np.diff(path, axis=0), axis=1)
    cum = np.concatenate([[0.0], np.cumsum(seg)])
    fine = np.linspace(0.0, cum[-1], 200001)
    dense = np.stack([np.interp(fine, cum, path[:, j]) for j in range(3)], 1)
    for _ in range(20):
        z = path[rng.integers(len(path))] + rng.normal(0, 0.1, 3)
        la = rng.uniform(0.0, 0.5)
        d = fine[np.argmin(((dense - z) ** 2).sum(1))]                                  # the distance along the path of the nearest point, by brute force
        want = np.array([np.interp(min(d + la, cum[-1]), cum, path[:, j]) for j in range(3)])
        assert np.abs(waypoint_along_points(path, z, la) - want).max() < 2e-5
    assert _same_bits(waypoint_along_points(path, path[0], 100.0), path[-1])
    assert _same_bits(waypoint_along_points(path[:1], path[3], 0.1), path[0])
    two = np.array([[0.0, 0, 0], [1.0, 0, 0]])
    assert np.allclose(waypoint_along_points(two, [0.25, 0.3, 0], 0.5), [0.75, 0, 0], atol=1e-15)


def _marked(worlds):
    """reference worlds with the far box the scripted backend knows a world by as their first obstacle"""
    out = []
    for w, (name, p) in enumerate(worlds):
        p = dict(p)
        p["obstacles"] = np.vstack([_box((100.0 + w, 0, 0), (0.01, 0.01, 0.01))[None], np.asarray(p["obstacles"]).reshape(-1, 12)])
        out.append((name, p))
    return out


def test_trials_take_their_waypoints_from_the_workspace_trees():
    from armour_amd import ik
    from armour_amd.scenes import pad_obstacles, reference_worlds
    from armour_amd.tree_planner import call_seed
    from armour_amd.trials import run_trials
    from armour_amd.ws_planner import plan_workspace_trees, waypoint_along_points, workspace_box, workspace_hlps
    robot = _robot("kinova")
    worlds = _marked(reference_worlds()[:3])
    k = np.zeros(7)
    k[1] = 0.4
    scripts = {w: [(True, k), (True, k), (False, None)] for w in range(3)}
    opts = dict(max_iterations=150, max_nodes=256)
    res, makes = {}, {}
    for batched in (True, False):
        makes[batched] = workspace_hlps(worlds, robot, seed=11, lookahead=0.15, host=True, batched=batched, ik_options=dict(S=8), **opts)
        assert hasattr(makes[batched], "get_waypoints") == batched
        res[batched] = run_trials(worlds, backend=ScriptedPlanner(scripts), audit_on_host=True, hlp=makes[batched], max_iterations=3, stop_threshold=5)
    O = max(p["obstacles"].shape[0] for _, p in worlds)
    lb, ub = workspace_box(robot)
    from_ik = 0
    for i, (wa, wb) in enumerate(zip(res[True]["worlds"], res[False]["worlds"])):
        assert len(wa["records"]) == len(wb["records"]) == 3
        goal, obs = worlds[i][1]["goal"], pad_obstacles(worlds[i][1]["obstacles"], O)
        for c, (ra, rb) in enumerate(zip(wa["records"], wb["records"])):
            assert _same_bits(ra["q_des"], rb["q_des"]) and _same_bits(ra["q0"], rb["q0"]), (i, c)      # batched equals per-world
            z = ik.end_effector(robot, ra["q0"])
            own = plan_workspace_trees(obs, [z], [ik.end_effector(robot, goal)], [call_seed(11, i, c)], lb, ub, host=True, **opts)
            assert own.margin[0] > MARGIN
            point = waypoint_along_points(own.paths[0], z, 0.15)                       # metres: the world's own lookahead is not used
            sol = ik.solve_ik(robot, point[None], 0.5 * (ra["q0"] + goal), obs, [0], [call_seed(11, i, c)], S=8, host=True)
            want = sol.q[0] if sol.status[0] == ik.FOUND else goal
            assert _same_bits(ra["q_des"], want), (i, c)
            from_ik += sol.status[0] == ik.FOUND
            if sol.status[0] == ik.FOUND:
                assert np.abs(ik.end_effector(robot, ra["q_des"]) - point).max() < 1e-6
    assert from_ik >= 6
    assert sum(h.fallbacks for h in makes[True].hlps.values()) == 9 - from_ik


def test_a_waypoint_out_of_reach_falls_back_to_the_goal_configuration_and_seed_mode_offers_the_last_path():
    from armour_amd import ik
    from armour_amd.scenes import reference_worlds
    from armour_amd.ws_planner import WorkspaceTreeHLP
    robot = _robot("kinova")
    name, p = reference_worlds()[0]
    q0, goal = np.asarray(p["q0"]), np.asarray(p["goal"])
    hlp = WorkspaceTreeHLP(robot, p["obstacles"], goal, seed=3, host=True, lb=np.full(3, -5.0), ub=np.full(3, 5.0), goal_rate=1.0, step=3.0, edge_step=0.05,
                           rewire_radius=0.0, max_iterations=3, max_nodes=8, ik_options=dict(S=4, max_iterations=50))
    hlp.goal_point = np.full(3, 4.5)                                                    # a workspace goal metres outside the reach: so is the waypoint
    q = hlp.get_waypoint(q0, 10.0)
    assert hlp.ik_status != ik.FOUND and hlp.fallbacks == 1 and _same_bits(q, goal)
    assert np.linalg.norm(hlp.waypoint) > 3.0
    seeded = WorkspaceTreeHLP(robot, p["obstacles"], goal, seed=3, host=True, mode="seed", max_iterations=150, max_nodes=256, ik_options=dict(S=8))
    seeded.get_waypoint(q0, 0.1)
    first = seeded.path
    seeded.get_waypoint(q0, 0.1)                                                        # from the same place: [z] + the rest of the last path is the chain
    assert len(first) > 2 and _same_bits(seeded.path[:1], first[:1])
    with pytest.raises(ValueError):
        WorkspaceTreeHLP(robot, p["obstacles"], goal, mode="keep")
