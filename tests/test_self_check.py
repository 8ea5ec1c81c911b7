"""Self-collision checks (include/armour_hip.h armour_self_*, armour_roadmap_check_self, armour_path_audit_self; armour_amd/self_check.py).

The pair rule is restated below in numpy, in the library's order of operations, on top of the roadmap's restated frames
(tests/test_roadmap.py) and the audit's restated pieces (tests/test_path_audit.py); the restatement is itself checked against an
independent LP ("the two boxes share a point").  CPU tests run the library's _host entries: the restatement, the finding on the
reference's own start and goal configurations, the motion bound, the soundness of edges and pieces.  GPU tests: the device entries
against the host entries and the restatement, batched against one-by-one, the roadmap's masks and the search with them."""
import numpy as np
import pytest

from test_path_audit import CL_TOL, D, K_RANGE, q_des, random_pieces, speed_bound
from test_roadmap import DEGENERATE, _limits, _robot, cross3, dot3, geometry, link_boxes, robot_dict, wrap

FOLDED = np.array([0.0, 2.1, 0.0, 2.5, 0.0, 1.0, 0.0])      # the Kinova folded onto itself: its last link 3.9 cm inside its first


# ----------------------------------------------------------------------------------------------------------- numpy restatement
def box_pair_clearance(xa, Ua, sa, xb, Ub, sb):
    """Clearance of box a (centre [...,3], unit axes U[..., k, :], half-sizes [...,3]) against box b by the 15 axes, in the library's order."""
    d = xb - xa
    vals = []
    for k in range(3):
        u = Ua[..., k, :]
        vals.append(np.abs(dot3(u, d)) - (sa[..., k] + ((sb[..., 0] * np.abs(dot3(u, Ub[..., 0, :])) + sb[..., 1] * np.abs(dot3(u, Ub[..., 1, :])))
                                                        + sb[..., 2] * np.abs(dot3(u, Ub[..., 2, :])))))
    for k in range(3):
        u = Ub[..., k, :]
        vals.append(np.abs(dot3(u, d)) - (((sa[..., 0] * np.abs(dot3(u, Ua[..., 0, :])) + sa[..., 1] * np.abs(dot3(u, Ua[..., 1, :])))
                                           + sa[..., 2] * np.abs(dot3(u, Ua[..., 2, :]))) + sb[..., k]))
    for i in range(3):
        i1, i2 = [x for x in range(3) if x != i]
        for k in range(3):
            k1, k2 = [x for x in range(3) if x != k]
            m = cross3(Ua[..., i, :], Ub[..., k, :])
            m2 = dot3(m, m)
            ok = ~(m2 <= DEGENERATE)
            num = np.abs(dot3(m, d)) - ((sa[..., i1] * np.abs(dot3(m, Ua[..., i1, :])) + sa[..., i2] * np.abs(dot3(m, Ua[..., i2, :])))
                                        + (sb[..., k1] * np.abs(dot3(m, Ub[..., k1, :])) + sb[..., k2] * np.abs(dot3(m, Ub[..., k2, :]))))
            vals.append(np.where(ok, num / np.where(ok, np.sqrt(m2), 1.0), -np.inf))
    return np.max(np.stack(vals, -1), -1)


def pair_list(g, pairs=None):
    """The pairs the rule tests, in its order: a < b listed (None: b - a >= 2), both links with a non-zero half-size."""
    J = g["J"]
    sized = [bool(np.any(g["h"][l] != 0.0)) for l in range(J)]
    return [(a, b) for a in range(J) for b in range(a + 1, J)
            if (b - a >= 2 if pairs is None else pairs[a][b]) and sized[a] and sized[b]]


def motion_radius(g, a, b, delta):
    r = 0.0
    for j in range(a + 1, min(b, g["n"] - 1) + 1):
        r = r + g["rho"][j, b] * delta[j]
    return r


def self_clearances(g, Q, pairs=None, shrink=None, delta=None):
    """[K, number of pairs]: the pair clearances at configurations Q [K,n], box b of pair (a, b) with half-sizes max(h_b - shrink_ab, 0) + r_ab
    (delta [n]: how far every joint may be from Q)."""
    _, R, x = link_boxes(g, np.asarray(Q, dtype=np.float64))
    U = np.swapaxes(R, -1, -2)
    out = []
    for a, b in pair_list(g, pairs):
        r = 0.0 if delta is None else motion_radius(g, a, b, delta)
        sh = 0.0 if shrink is None else shrink[a][b]
        sb = np.maximum(g["h"][b] - sh, 0.0) + r
        K = x.shape[0]
        out.append(box_pair_clearance(x[:, a], U[:, a], np.broadcast_to(g["h"][a], (K, 3)), x[:, b], U[:, b], np.broadcast_to(sb, (K, 3))))
    return np.stack(out, -1) if out else np.zeros((np.asarray(Q).shape[0], 0))


def self_check_np(g, Q, pairs=None, shrink=None):
    """(clearance [K], worst pair of the minimum [K], first colliding pair or -1 [K])."""
    pl = pair_list(g, pairs)
    cl = self_clearances(g, Q, pairs, shrink)
    code = np.array([a * g["J"] + b for a, b in pl], dtype=np.int32)
    K = cl.shape[0]
    if not pl:
        return np.full(K, np.inf), np.full(K, -1, dtype=np.int32), np.full(K, -1, dtype=np.int32)
    hit = cl <= 0
    first = np.where(hit.any(1), code[np.argmax(hit, 1)], -1)
    return cl.min(1), code[np.argmin(cl, 1)], first


def edge_items(g, a, b, edge_step):
    """Midpoints [S,n] and the per-joint radius delta [n] of the edge a -> b."""
    Dj = np.where(g["cont"], wrap(b - a), b - a)
    S = max(1, int(np.ceil(np.abs(Dj).max() / edge_step)))
    t = (2 * np.arange(S) + 1).astype(np.float64) / float(2 * S)
    return a + t[:, None] * Dj, np.abs(Dj) / float(2 * S), Dj


def edge_self_free_np(g, a, b, edge_step, pairs=None, shrink=None):
    q, delta, _ = edge_items(g, a, b, edge_step)
    cl = self_clearances(g, q, pairs, shrink, delta)
    return bool(np.all(cl > 0)), (np.abs(cl).min() if cl.size else np.inf)


def piece_points(g, piece, k_range, dur, step, tube=None):
    q0, qd0, qdd0, k, ta, tb = piece
    n = g["n"]
    ka = k_range[:n] * k
    v = speed_bound(q0, qd0, qdd0, ka, dur)
    w = tb - ta
    S = max(1, int(np.ceil((v * w).max() / step)))
    t = ta + ((2 * np.arange(S) + 1).astype(np.float64) * w) / float(2 * S)
    q = q_des(q0[None], (qd0 * dur)[None], (qdd0 * dur * dur)[None], ka[None], (t / dur)[:, None])
    return t, q, v * (w / float(2 * S)) + (np.zeros(n) if tube is None else tube)


def audit_self_np(g, piece, k_range, dur, step, tube=None, pairs=None, shrink=None):
    """(verdict, t_hit, clearance, margin) of one piece by the rule."""
    t, q, dev = piece_points(g, piece, k_range, dur, step, tube)
    sample = self_clearances(g, q, pairs, shrink)
    tubed = self_clearances(g, q, pairs, shrink, dev)
    if sample.shape[1] == 0:
        return 0, np.nan, np.inf, np.inf
    margin = min(np.abs(sample).min(), np.abs(tubed).min())
    hit = (sample <= 0).any(1)
    if hit.any():
        return 1, t[np.argmax(hit)], sample.min(), margin
    return (0 if np.all(tubed > 0) else 2), np.nan, sample.min(), margin


# ----------------------------------------------------------------------------------------------------------- helpers
def _configs(robot, rng, N):
    lb, ub, _ = _limits(robot)
    return lb + (ub - lb) * rng.random((N, robot.num_factors))


def _reference_configs():
    """The 214 start and goal configurations of the reference's 107 worlds: starts, then goals."""
    from armour_amd.scenes import reference_worlds
    ws = reference_worlds()
    return np.stack([p["q0"] for _, p in ws] + [p["goal"] for _, p in ws])


def _variants(robot, rng):
    """(pairs, shrink) tables to test with: the defaults, and a table of its own with a shrink."""
    J = robot.num_joints
    pairs = np.triu(rng.random((J, J)) < 0.6, 2).astype(np.uint8)
    pairs[0, J - 1] = 1
    shrink = np.triu(rng.choice([0.0, 0.01, 0.2], (J, J)), 1)
    return [(None, None), (pairs, shrink)]


# ----------------------------------------------------------------------------------------------------------- CPU
def test_numpy_rule_agrees_with_an_lp():
    """The 15 axes separate two boxes exactly when the boxes share no point (an LP over both boxes' coordinates)."""
    from scipy.optimize import linprog
    from armour_amd.robot_geometry import rpy_matrix
    rng = np.random.default_rng(7)
    checked = sep = 0
    for _ in range(200):
        Ra, Rb = rpy_matrix(*rng.uniform(-np.pi, np.pi, 3)), rpy_matrix(*rng.uniform(-np.pi, np.pi, 3))
        if rng.random() < 0.3:
            Rb = Ra @ rpy_matrix(0.0, 0.0, rng.uniform(-np.pi, np.pi))       # a shared axis: three degenerate cross products
        sa, sb = rng.uniform(0.02, 0.3, 3), rng.uniform(0.02, 0.3, 3)
        xa, xb = rng.normal(size=3) * 0.2, rng.normal(size=3) * 0.2
        cl = box_pair_clearance(xa, Ra.T, sa, xb, Rb.T, sb)
        if abs(cl) <= 1e-9:
            continue
        lp = linprog(np.zeros(6), A_eq=np.concatenate([Ra * sa, -(Rb * sb)], axis=1), b_eq=xb - xa, bounds=[(-1, 1)] * 6, method="highs")
        assert lp.status in (0, 2), lp.message
        assert (lp.status == 0) == (cl <= 0), (cl, lp.status)
        checked += 1
        sep += cl > 0
    assert checked >= 190 and 20 <= sep <= checked - 20, (checked, sep)


def test_default_pairs_and_the_links_the_rule_skips():
    from armour_amd.self_check import default_pairs
    for name, J in (("kinova", 7), ("gripper", 8), ("fetch", 9)):
        robot = _robot(name)
        dp = default_pairs(robot)
        assert dp.shape == (J, J) and np.array_equal(dp, np.triu(np.ones((J, J), dtype=np.uint8), 2))
    g = geometry(robot_dict(_robot("fetch")))
    sized = np.any(g["h"] != 0, axis=1)
    assert not sized.all() and sized.sum() >= 3                  # Fetch has zero-size links: they are in no pair
    assert all(sized[a] and sized[b] for a, b in pair_list(g))


@pytest.mark.parametrize("name", ["kinova", "gripper", "fetch"])
def test_host_entry_equals_the_restatement(name):
    from armour_amd.self_check import check
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    rng = np.random.default_rng(31)
    Q = _configs(robot, rng, 400)
    if name != "fetch":
        Q[:20] = FOLDED + rng.normal(size=(20, 7)) * 0.1
    hits = 0
    for pairs, shrink in _variants(robot, rng):
        cl, worst, first = self_check_np(g, Q, pairs, shrink)
        full = check(robot, Q, pairs=pairs, shrink=shrink, clearance=True, host=True)
        fast = check(robot, Q, pairs=pairs, shrink=shrink, host=True)
        sure = np.abs(self_clearances(g, Q, pairs, shrink)).min(1) > 1e-9
        assert np.abs(full.clearance - cl).max() <= CL_TOL
        assert np.array_equal(full.free[sure], (cl > 0)[sure]) and np.array_equal(fast.free[sure], (cl > 0)[sure])
        assert np.array_equal(fast.worst_pair[sure], first[sure])
        gap = np.sort(self_clearances(g, Q, pairs, shrink), axis=1)
        clear_min = (gap[:, 1] - gap[:, 0] > 1e-9) if gap.shape[1] > 1 else np.ones(len(Q), dtype=bool)
        assert np.array_equal(full.worst_pair[clear_min], worst[clear_min])
        hits += int((~fast.free).sum())
    assert hits >= (5 if name != "fetch" else 0)
    # one configuration, no pair at all: free, +inf, -1
    none = check(robot, Q[:1], pairs=np.zeros((robot.num_joints,) * 2), clearance=True, host=True)
    assert none.free[0] and none.clearance[0] == np.inf and none.worst_pair[0] == -1


# the configurations of _reference_configs() (0..106 starts, 107..213 goals) where a non-adjacent pair of link boxes overlaps
KINOVA_OVERLAPS = [15, 41, 43, 63, 71, 169, 172, 179, 195, 201]
GRIPPER_OVERLAPS = [15, 41, 43, 63, 71, 151, 169, 172, 179, 195, 201, 206]


def test_the_reference_worlds_own_configurations_overlap_and_calibration_clears_them():
    from armour_amd.self_check import calibrate_shrink, check
    Q = _reference_configs()
    assert Q.shape == (214, 7)
    for name, want in (("kinova", KINOVA_OVERLAPS), ("gripper", GRIPPER_OVERLAPS)):
        robot = _robot(name)
        g = geometry(robot_dict(robot))
        cl, _, _ = self_check_np(g, Q)
        assert np.abs(self_clearances(g, Q)).min() > 1e-9
        res = check(robot, Q, host=True)
        print(f"{name}: overlapping {np.flatnonzero(cl <= 0).tolist()}, deepest {cl.min():.4f} m")
        assert np.array_equal(np.flatnonzero(~res.free), np.flatnonzero(cl <= 0))
        assert np.flatnonzero(~res.free).tolist() == want
        shrink = calibrate_shrink(robot, Q, host=True)
        deepest = -self_clearances(g, Q).min(0)
        for (a, b), p in zip(pair_list(g), deepest):
            assert shrink[a, b] == (p + 1e-3 if p >= 0 else 0.0), (a, b, p, shrink[a, b])
        assert check(robot, Q, shrink=shrink, host=True).free.all()
        folded = check(robot, FOLDED, shrink=shrink, clearance=True, host=True)
        assert not folded.free[0] and folded.clearance[0] < -0.01, folded.clearance
    assert len(KINOVA_OVERLAPS) == 10 and len(GRIPPER_OVERLAPS) == 12


def test_fetch_has_no_overlapping_pair_on_random_configurations():
    from armour_amd.self_check import check
    robot = _robot("fetch")
    assert check(robot, _configs(robot, np.random.default_rng(3), 2000), host=True).free.all()


@pytest.mark.parametrize("name", ["kinova", "gripper", "fetch"])
def test_the_motion_bound_holds_in_the_frame_of_the_first_link(name):
    """With every joint within delta_j of a midpoint, no point of box b, seen from frame a, is further than r_ab from where it is at the midpoint."""
    g = geometry(robot_dict(_robot(name)))
    n, J = g["n"], g["J"]
    rng = np.random.default_rng(41)
    corners = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], dtype=np.float64)
    worst = 0.0
    for _ in range(200):
        a = int(rng.integers(0, J - 2))
        b = int(rng.integers(a + 2, J))
        mid = rng.uniform(-np.pi, np.pi, n)
        delta = rng.choice([0.01, 0.05, 0.3]) * rng.random(n)
        Q = np.concatenate([mid[None], mid + delta * rng.uniform(-1, 1, (500, n))])
        Q[1:, :a + 1] = rng.uniform(-np.pi, np.pi, (500, a + 1))[:, :min(a + 1, n)]      # joints <= a move the pair rigidly: anywhere
        P, R, _ = link_boxes(g, Q)
        pts = P[:, b, None, :] + np.einsum("kij,cj->kci", R[:, b], g["c"][b] + corners * g["h"][b])      # [501,8,3] in the world
        rel = np.einsum("kji,kcj->kci", R[:, a], pts - P[:, a, None, :])                                  # in frame a
        disp = np.linalg.norm(rel[1:] - rel[:1], axis=-1).max()
        r = motion_radius(g, a, b, delta)
        assert disp <= r * (1 + 1e-12) + 1e-14, (name, a, b, disp, r)
        worst = max(worst, disp / max(r, 1e-300))
    assert worst > 0.05, worst      # the bound is not vacuous


EDGE_STEP = 0.02


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_self_free_edges_are_self_free_everywhere(name):
    from armour_amd.self_check import calibrate_shrink, edges_free_host
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    n = g["n"]
    rng = np.random.default_rng(43)
    shrink = calibrate_shrink(robot, _reference_configs(), host=True) if name == "kinova" else None
    E = 120
    qa = _configs(robot, rng, E)
    qb = qa + rng.uniform(-0.4, 0.4, (E, n))
    free = edges_free_host(robot, qa, qb, edge_step=EDGE_STEP, continuous=g["cont"], shrink=shrink)
    undecided = hit = 0
    for e in range(E):
        want, margin = edge_self_free_np(g, qa[e], qb[e], EDGE_STEP, shrink=shrink)
        if margin > 1e-9:
            assert free[e] == want, (name, e)
        Dj = np.where(g["cont"], wrap(qb[e] - qa[e]), qb[e] - qa[e])
        dense = self_clearances(g, qa[e] + np.linspace(0, 1, 200)[:, None] * Dj, shrink=shrink).min(1)
        if free[e]:
            assert dense.min() > 0, (name, e)
        elif dense.min() > 0:
            undecided += 1
        else:
            hit += 1
    print(f"{name}: {int(free.sum())} self-free edges, {hit} with a colliding sample, {undecided} undecided of {E} at edge_step {EDGE_STEP}")
    assert free.sum() >= 10 and undecided <= E // 2, (free.sum(), undecided)


AUDIT_STEP = 0.005


@pytest.mark.parametrize("name", ["kinova", "gripper", "fetch"])
def test_host_audit_equals_the_restatement_and_its_verdicts_are_sound(name):
    from armour_amd.path_audit import audit_self
    from armour_amd.self_check import calibrate_shrink
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    n = g["n"]
    kr = K_RANGE[:n]
    rng = np.random.default_rng(47)
    shrink = calibrate_shrink(robot, _reference_configs(), host=True) if name != "fetch" else None
    P = 90
    arrs = list(random_pieces(robot, rng, P, still=0.3))
    if name != "fetch":
        arrs[0][:15] = FOLDED + rng.normal(size=(15, 7)) * 0.15
    tube = rng.choice([0.0, 0.002, 0.01], (P, 1)) * rng.random((P, n))
    res = audit_self(robot, *arrs[:4], kr, D, arrs[4], arrs[5], tube=tube, step=AUDIT_STEP, shrink=shrink, clearance=True, host=True)
    fast = audit_self(robot, *arrs[:4], kr, D, arrs[4], arrs[5], tube=tube, step=AUDIT_STEP, shrink=shrink, host=True)
    assert np.array_equal(res.verdict, fast.verdict) and np.array_equal(res.t_hit, fast.t_hit, equal_nan=True)
    bare = audit_self(robot, *arrs[:4], kr, D, arrs[4], arrs[5], step=AUDIT_STEP, shrink=shrink, host=True)
    assert np.all(bare.verdict[res.verdict == 0] == 0) and np.array_equal(bare.verdict == 1, res.verdict == 1)
    counts = [0, 0, 0]
    for p in range(P):
        piece = tuple(a[p] for a in arrs)
        q0, qd0, qdd0, k, ta, tb = piece
        v, th, cl, margin = audit_self_np(g, piece, kr, D, AUDIT_STEP, tube[p], shrink=shrink)
        if margin > 1e-9:
            assert res.verdict[p] == v, (name, p, res.verdict[p], v)
            assert (np.isnan(th) and np.isnan(res.t_hit[p])) or res.t_hit[p] == th, (name, p)
        assert abs(res.clearance[p] - cl) <= CL_TOL
        counts[res.verdict[p]] += 1
        if res.verdict[p] == 0:
            t = ta + (tb - ta) * rng.random(200)
            Q = q_des(q0[None], (qd0 * D)[None], (qdd0 * D * D)[None], (kr * k)[None], (t / D)[:, None])
            assert self_clearances(g, Q, shrink=shrink).min() > 0, (name, p)
            assert self_clearances(g, Q + tube[p] * rng.uniform(-1, 1, Q.shape), shrink=shrink).min() > 0, (name, p)
        elif res.verdict[p] == 1:
            Q = q_des(q0, qd0 * D, qdd0 * D * D, kr * k, res.t_hit[p] / D)[None]
            assert ta <= res.t_hit[p] <= tb and self_clearances(g, Q, shrink=shrink).min() <= 0, (name, p)
    print(f"{name}: proved self-free / proved self-hit / undecided = {counts} at step {AUDIT_STEP}")
    assert counts[0] >= 10 and counts[2] <= P // 2, counts
    if name != "fetch":
        assert counts[1] >= 5, counts


def test_entries_refuse_bad_arguments_before_touching_a_device():
    from armour_amd import _lib
    from armour_amd.path_audit import audit_self
    from armour_amd.self_check import check
    robot = _robot("kinova")
    z = np.zeros((1, 7))
    bad = np.zeros((7, 7))
    bad[1, 4] = -0.01
    for kw in (dict(q=np.full((1, 7), np.nan)), dict(shrink=bad)):
        with pytest.raises(_lib.ArmourError) as ei:     # (the device entry: refused although this machine may have no device)
            check(robot, kw.get("q", z), shrink=kw.get("shrink"))
        assert ei.value.code == _lib.EINVAL, kw
    for kw in (dict(step=0.0), dict(ta=0.6, tb=0.5), dict(tube=-np.ones(7)), dict(shrink=bad)):
        with pytest.raises(_lib.ArmourError) as ei:
            audit_self(robot, z, z, z, z, K_RANGE, D, kw.get("ta", 0.0), kw.get("tb", 0.5), tube=kw.get("tube"), step=kw.get("step", 0.02), shrink=kw.get("shrink"))
        assert ei.value.code == _lib.EINVAL, kw


# ----------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kinova", "gripper", "fetch"])
def test_device_configurations_equal_the_host_entry_and_the_restatement(name):
    from armour_amd.self_check import check
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    rng = np.random.default_rng(53)
    Q = _configs(robot, rng, 257)
    if name != "fetch":
        Q[::8] = FOLDED + rng.normal(size=(33, 7)) * 0.1
    for pairs, shrink in _variants(robot, rng):
        cl, _, _ = self_check_np(g, Q, pairs, shrink)
        for N in (1, 255, 256, 257):
            dev, host = check(robot, Q[:N], pairs=pairs, shrink=shrink), check(robot, Q[:N], pairs=pairs, shrink=shrink, host=True)
            assert np.array_equal(dev.free, host.free) and np.array_equal(dev.worst_pair, host.worst_pair), (name, N)
            devc, hostc = check(robot, Q[:N], pairs=pairs, shrink=shrink, clearance=True), check(robot, Q[:N], pairs=pairs, shrink=shrink, clearance=True, host=True)
            assert np.array_equal(devc.free, hostc.free) and np.array_equal(devc.worst_pair, hostc.worst_pair), (name, N)
            assert np.abs(devc.clearance - cl[:N]).max() <= CL_TOL, (name, N)
        one = [check(robot, Q[i], pairs=pairs, shrink=shrink, clearance=True) for i in range(257)]
        assert np.array_equal(devc.clearance, np.array([o.clearance[0] for o in one]))
        assert np.array_equal(devc.worst_pair, np.array([o.worst_pair[0] for o in one])) and np.array_equal(devc.free, np.array([o.free[0] for o in one]))
    assert name == "fetch" or (~dev.free).sum() >= 5


def _small_roadmap(robot, seed, radius):
    from armour_amd.roadmap import uniform_roadmap
    lb, ub, cont = _limits(robot)
    return uniform_roadmap(300, radius, 6, seed, lb, ub, cont) + (cont,)


@pytest.mark.gpu
@pytest.mark.parametrize("name,radius", [("kinova", 2.6), ("fetch", 2.3)])
def test_roadmap_self_masks_equal_the_host_rule(name, radius):
    from armour_amd.roadmap import Roadmap
    from armour_amd.self_check import check, edges_free_host
    from test_roadmap import _reference_obstacles
    robot = _robot(name)
    nodes, edges, cont = _small_roadmap(robot, 5, radius)
    assert 200 <= len(edges) <= 1500, len(edges)
    obs = _reference_obstacles()["obstacles"][:3]
    rm = Roadmap(robot, nodes, edges, continuous=cont, edge_step=0.05)
    before = rm.check(obs, clearance=True)
    s1 = rm.check_self(clearance=True)
    s2 = rm.check_self(clearance=True)
    after = rm.check(obs, clearance=True)
    for key in ("node_free", "edge_free", "node_clearance"):
        assert np.array_equal(s1[key], s2[key]) and np.array_equal(before[key], after[key]), key
    host = check(robot, nodes, clearance=True, host=True)
    assert np.array_equal(s1["node_free"], host.free) and np.abs(s1["node_clearance"] - host.clearance).max() <= CL_TOL
    assert np.array_equal(s1["edge_free"], edges_free_host(robot, nodes[edges[:, 0]], nodes[edges[:, 1]], edge_step=0.05, continuous=cont))
    fe = edges[s1["edge_free"]]
    assert s1["node_free"][fe].all()                 # a free edge has free endpoints
    print(f"{name}: {len(edges)} edges, {int(s1['edge_free'].sum())} self-free, {int(s1['node_free'].sum())} of 300 nodes self-free, {s1['ms']:.3f} ms")
    rm.close()


@pytest.mark.gpu
def test_plan_with_the_self_masks_avoids_the_fold_and_is_unchanged_without_them():
    from armour_amd import _lib
    from armour_amd.roadmap import Roadmap
    from armour_amd.scenes import FAR_BOX
    from armour_amd.self_check import calibrate_shrink, check, edges_free_host
    robot = _robot("kinova")
    g = geometry(robot_dict(robot))
    nodes, edges, cont = _small_roadmap(robot, 9, 2.8)
    shrink = calibrate_shrink(robot, _reference_configs(), host=True)
    rng = np.random.default_rng(59)
    ends = [(_configs(robot, rng, 1)[0], _configs(robot, rng, 1)[0]) for _ in range(6)]
    # a direct edge that folds the arm through itself: from one side of the fold to the other
    lo, hi = FOLDED.copy(), FOLDED.copy()
    lo[5], hi[5] = 0.3, 1.7
    ends.append((lo, hi))
    plain = Roadmap(robot, nodes, edges, continuous=cont)
    plain.check(FAR_BOX[None])
    want = [plain.plan(0, s, t) for s, t in ends]
    plain.close()
    assert want[-1] is not None and len(want[-1]) == 2          # nothing in the world: the straight line through the fold
    rm = Roadmap(robot, nodes, edges, continuous=cont)
    rm.check(FAR_BOX[None])
    rm.use_self(True)
    with pytest.raises(_lib.ArmourError) as ei:
        rm.plan(0, *ends[0])
    assert ei.value.code == _lib.ESTATE
    rm.use_self(False)
    masks = rm.check_self(shrink=shrink)
    got = [rm.plan(0, s, t) for s, t in ends]                     # off: the paths of a roadmap that never saw a self call
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(got, want))
    rm.use_self(True)
    routed = 0
    for s, t in ends:
        if not (check(robot, np.stack([s, t]), shrink=shrink, host=True).free.all()):
            continue
        path = rm.plan(0, s, t)
        if path is None:
            continue
        routed += 1
        assert check(robot, path, shrink=shrink, host=True).free.all()
        assert edges_free_host(robot, path[:-1], path[1:], continuous=cont, shrink=shrink).all()
        for a, b in zip(path[:-1], path[1:]):
            Dj = np.where(g["cont"], wrap(b - a), b - a)
            assert self_clearances(g, a + np.linspace(0, 1, 100)[:, None] * Dj, shrink=shrink).min() > 0
    fold = rm.plan(0, lo, hi)
    assert fold is None or len(fold) > 2                          # routed around or refused, never straight through
    assert routed >= 2 and masks["edge_free"].sum() > 0
    rm.close()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_device_audit_equals_the_host_audit_and_one_call_equals_forty():
    from armour_amd import scenes
    from armour_amd.path_audit import audit_self
    from armour_amd.planner import ArmourNLP
    from armour_amd.self_check import calibrate_shrink
    robot = _robot("kinova")
    g = geometry(robot_dict(robot))
    shrink = calibrate_shrink(robot, _reference_configs(), host=True)
    bp = scenes.as_batch(scenes.reference_worlds()[:20])
    nlp = ArmourNLP(robot=robot, T=40).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    k_opt = np.nan_to_num(np.stack([s["k_opt"] for s in nlp.solve()]))
    k_range = np.array(nlp.params.k_range[:7])
    nlp.close()
    rng = np.random.default_rng(61)
    rnd = list(random_pieces(robot, rng, 20, still=0.3))
    rnd[0][:6] = FOLDED + rng.normal(size=(6, 7)) * 0.15
    z = np.zeros((20, 7))
    planned = (bp["q0"], z, z, k_opt, np.zeros(20), np.full(20, 0.5 * D))
    arrs = tuple(np.concatenate([a, b]) for a, b in zip(rnd, planned))
    tube = rng.choice([0.0, 0.005], (40, 1)) * rng.random((40, 7))
    for tb_ in (None, tube):
        kw = dict(tube=tb_, step=0.01, shrink=shrink)
        dev = audit_self(robot, *arrs[:4], k_range, D, arrs[4], arrs[5], clearance=True, **kw)
        fast = audit_self(robot, *arrs[:4], k_range, D, arrs[4], arrs[5], **kw)
        host = audit_self(robot, *arrs[:4], k_range, D, arrs[4], arrs[5], clearance=True, host=True, **kw)
        assert np.array_equal(dev.verdict, host.verdict) and np.array_equal(dev.t_hit, host.t_hit, equal_nan=True)
        assert np.array_equal(fast.verdict, host.verdict) and np.array_equal(fast.t_hit, host.t_hit, equal_nan=True)
        want = np.array([audit_self_np(g, tuple(a[p] for a in arrs), k_range, D, 0.01, None if tb_ is None else tb_[p], shrink=shrink)[2] for p in range(40)])
        assert np.abs(dev.clearance - want).max() <= CL_TOL
        one = [audit_self(robot, *(a[p:p + 1] for a in arrs[:4]), k_range, D, arrs[4][p:p + 1], arrs[5][p:p + 1], clearance=True,
                          **dict(kw, tube=None if tb_ is None else tb_[p:p + 1])) for p in range(40)]
        assert np.array_equal(dev.verdict, [o.verdict[0] for o in one]) and np.array_equal(dev.clearance, [o.clearance[0] for o in one])
        assert np.array_equal(dev.t_hit, [o.t_hit[0] for o in one], equal_nan=True)
        if tb_ is None:
            bare = dev
    assert np.all(bare.verdict[dev.verdict == 0] == 0) and np.array_equal(bare.verdict == 1, dev.verdict == 1)
    print(f"verdicts with the tube {np.bincount(dev.verdict, minlength=3).tolist()}, without {np.bincount(bare.verdict, minlength=3).tolist()}")
    assert (dev.verdict == 1).sum() >= 1 and (bare.verdict == 0).sum() >= 5
