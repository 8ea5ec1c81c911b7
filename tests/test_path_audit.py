"""Path audit (include/armour_hip.h armour_path_audit, armour_amd/path_audit.py).

The audit rule is restated below in numpy, in the library's order of operations, on top of the roadmap's restated node rule
(tests/test_roadmap.py).  CPU tests: the speed bound, the soundness of verdicts 0 and 1 of the restatement, the library's host audit
against the restatement.  GPU tests: the device audit against the restatement on the reference's worlds for three robots, batched against
one-by-one, and a piece driven through a box."""
import numpy as np
import pytest

from test_roadmap import _limits, _robot, config_clearance, geometry, link_boxes, robot_dict

K_RANGE = np.full(7, np.pi / 48)
D = 1.0
CL_TOL = 1e-12            # tests/test_roadmap.py: the same arithmetic, device sin / cos against numpy's


# ----------------------------------------------------------------------------------------------------------- numpy restatement
def _p2(x):
    return x * x


def _p3(x):
    return x * x * x


def _p4(x):
    y = x * x
    return y * y


def _p5(x):
    y = x * x
    return y * y * x


def q_des(q0, a, b, ka, t):
    """bezier.h q_des, term by term."""
    u = t - 1
    B0, B1, B2, B3, B4, B5 = -_p5(u), 5 * t * _p4(u), -10 * _p2(t) * _p3(u), 10 * _p3(t) * _p2(u), -5 * _p4(t) * u, _p5(t)
    b0, b1, b2, b3 = q0, q0 + a / 5, q0 + (2 * a) / 5 + b / 20, q0 + ka
    return B0 * b0 + B1 * b1 + B2 * b2 + B3 * b3 + B4 * b3 + B5 * b3


def speed_bound(q0, qd0, qdd0, ka, dur):
    a, b = qd0 * dur, qdd0 * dur * dur
    P1, P2, P3 = q0 + a / 5, q0 + (2 * a) / 5 + b / 20, q0 + ka
    return np.maximum(np.maximum(np.abs(5 * (P1 - q0)), np.abs(5 * (P2 - P1))), np.abs(5 * (P3 - P2))) / dur


def piece_items(g, piece, k_range, dur, step, tube=None):
    """(t [S], q [S,n], r [S,J]) of one piece (q0, qd0, qdd0, k, ta, tb): sub-interval midpoints and the tube test's enlargements."""
    q0, qd0, qdd0, k, ta, tb = piece
    n, J = g["n"], g["J"]
    ka = k_range[:n] * k
    v = speed_bound(q0, qd0, qdd0, ka, dur)
    w = tb - ta
    S = max(1, int(np.ceil((v * w).max() / step)))
    t = ta + ((2 * np.arange(S) + 1).astype(np.float64) * w) / float(2 * S)
    half = w / float(2 * S)
    q = q_des(q0[None], (qd0 * dur)[None], (qdd0 * dur * dur)[None], ka[None], (t / dur)[:, None])
    dev = v * half + (np.zeros(n) if tube is None else tube)
    r = np.zeros(J)
    for l in range(J):
        acc = 0.0
        for j in range(min(l + 1, n)):
            acc = acc + g["rho"][j, l] * dev[j]
        r[l] = acc
    return t, q, np.broadcast_to(r, (S, J)).copy()


def audit_np(g, Z, piece, k_range, dur, step, tube=None):
    """(verdict, t_hit, clearance, margin) of one piece by the rule; margin = how far the decisive quantities are from zero."""
    t, q, r = piece_items(g, piece, k_range, dur, step, tube)
    sample = config_clearance(g, q, Z)
    tube_cl = config_clearance(g, q, Z, r)
    hit = sample <= 0
    margin = min(np.abs(sample).min(), np.abs(tube_cl).min())
    if hit.any():
        return 1, t[np.argmax(hit)], sample.min(), margin
    return (0 if np.all(tube_cl > 0) else 2), np.nan, sample.min(), margin


# ----------------------------------------------------------------------------------------------------------- helpers
def _worlds():
    from armour_amd.scenes import as_batch, reference_worlds
    return as_batch(reference_worlds())["obstacles"]


def random_pieces(robot, rng, P, still=0.0):
    """Random plans within the robot's limits and windows that are the first or the braking half of the plan, or a random sub-window."""
    lb, ub, _ = _limits(robot)
    n = robot.num_factors
    q0 = lb + (ub - lb) * rng.random((P, n))
    qd0 = rng.uniform(-0.6, 0.6, (P, n)) * (rng.random((P, 1)) >= still)
    qdd0 = rng.uniform(-1.5, 1.5, (P, n)) * (rng.random((P, 1)) >= still)
    k = rng.uniform(-1, 1, (P, n))
    kind = rng.integers(0, 3, P)
    a, b = np.sort(rng.random((2, P)), axis=0) * D
    ta = np.where(kind == 0, 0.0, np.where(kind == 1, 0.5 * D, a))
    tb = np.where(kind == 0, 0.5 * D, np.where(kind == 1, D, b))
    return q0, qd0, qdd0, k, ta, tb


def _piece(arrs, p):
    return tuple(a[p] for a in arrs)


def _compare(res, g, obs, world, arrs, k_range, step, tube, tag):
    """A library result against the restatement, piece by piece; returns the verdict counts."""
    counts = [0, 0, 0]
    for p in range(len(world)):
        v, th, cl, margin = audit_np(g, obs[world[p]], _piece(arrs, p), k_range, D, step, None if tube is None else tube[p])
        if margin > 1e-9:          # (a decisive quantity within rounding of zero may fall either way)
            assert res.verdict[p] == v, (tag, p, res.verdict[p], v)
            assert (np.isnan(th) and np.isnan(res.t_hit[p])) or res.t_hit[p] == th, (tag, p, res.t_hit[p], th)
        if res.clearance is not None:
            assert abs(res.clearance[p] - cl) <= CL_TOL, (tag, p, res.clearance[p], cl)
        counts[v] += 1
    return counts


# ----------------------------------------------------------------------------------------------------------- CPU
def test_speed_bound_bounds_the_joint_velocity():
    from armour_amd.planner import desired_trajectory
    rng = np.random.default_rng(1)
    robot = _robot("kinova")
    arrs = random_pieces(robot, rng, 60)
    worst = 0.0
    for p in range(60):
        q0, qd0, qdd0, k, _, _ = _piece(arrs, p)
        v = speed_bound(q0, qd0, qdd0, K_RANGE * k, D)
        qd = np.stack([desired_trajectory(q0, qd0, qdd0, k, t, k_range=K_RANGE, duration=D)[1] for t in np.linspace(0, D, 201)])
        assert np.all(np.abs(qd).max(0) <= v * (1 + 1e-12) + 1e-15), p
        worst = max(worst, (np.abs(qd).max(0) / np.maximum(v, 1e-300)).max())
    assert worst > 0.5, worst     # the bound is not vacuous
    # a longer duration scales the bound with the curve
    q0, qd0, qdd0, k, _, _ = _piece(arrs, 0)
    qd = np.stack([desired_trajectory(q0, qd0, qdd0, k, t, k_range=K_RANGE, duration=2.5)[1] for t in np.linspace(0, 2.5, 201)])
    assert np.all(np.abs(qd).max(0) <= speed_bound(q0, qd0, qdd0, K_RANGE * k, 2.5) * (1 + 1e-12))


@pytest.mark.parametrize("name", ["kinova", "fetch"])
def test_verdicts_of_the_rule_are_sound(name):
    """Verdict 0: 200 dense samples of the piece are free by the exact node rule, also with every joint moved by a random offset within the
    tube.  Verdict 1: the configuration at t_hit collides."""
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    n = g["n"]
    kr = K_RANGE[:n]
    obs = _worlds()
    rng = np.random.default_rng(17)
    P = 150
    arrs = random_pieces(robot, rng, P, still=0.3)
    world = rng.integers(0, obs.shape[0], P)
    tube = rng.choice([0.0, 0.005, 0.02], (P, 1)) * rng.random((P, n))
    counts = [0, 0, 0]
    for p in range(P):
        piece = _piece(arrs, p)
        q0, qd0, qdd0, k, ta, tb = piece
        v, th, _, _ = audit_np(g, obs[world[p]], piece, kr, D, rng.choice([0.01, 0.05]), tube[p])
        counts[v] += 1
        if v == 0:
            t = ta + (tb - ta) * rng.random(200)
            Q = q_des(q0[None], (qd0 * D)[None], (qdd0 * D * D)[None], (kr * k)[None], (t / D)[:, None])
            assert config_clearance(g, Q, obs[world[p]]).min() > 0, (name, p)
            assert config_clearance(g, Q + tube[p] * rng.uniform(-1, 1, Q.shape), obs[world[p]]).min() > 0, (name, p)
        elif v == 1:
            Q = q_des(q0, qd0 * D, qdd0 * D * D, kr * k, th / D)[None]
            assert ta <= th <= tb and config_clearance(g, Q, obs[world[p]])[0] <= 0, (name, p)
    print(f"{name}: proved free / proved hit / undecided = {counts}")
    assert counts[0] >= 10 and counts[1] >= 10, counts


@pytest.mark.parametrize("name", ["kinova", "gripper", "fetch"])
def test_host_audit_equals_the_restatement(name):
    from armour_amd.path_audit import audit, audit_items
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    n = g["n"]
    obs = _worlds()[::9]
    rng = np.random.default_rng(23)
    P = 80
    arrs = random_pieces(robot, rng, P, still=0.3)
    world = rng.integers(0, obs.shape[0], P).astype(np.int32)
    tube = rng.choice([0.0, 0.01], (P, 1)) * rng.random((P, n))
    total = [0, 0, 0]
    for step, tb_ in ((0.02, None), (0.05, tube)):
        res = audit(robot, obs, world, *arrs[:4], K_RANGE[:n], D, arrs[4], arrs[5], tube=tb_, step=step, clearance=True, host=True)
        fast = audit(robot, obs, world, *arrs[:4], K_RANGE[:n], D, arrs[4], arrs[5], tube=tb_, step=step, host=True)
        assert np.array_equal(res.verdict, fast.verdict) and np.array_equal(res.t_hit, fast.t_hit, equal_nan=True)   # early exit changes nothing
        counts = _compare(res, g, obs, world, arrs, K_RANGE[:n], step, tb_, (name, step))
        S = audit_items(robot, *arrs[:4], K_RANGE[:n], D, arrs[4], arrs[5], step=step)
        assert np.array_equal(S, [piece_items(g, _piece(arrs, p), K_RANGE[:n], D, step)[0].size for p in range(P)])
        total = [a + b for a, b in zip(total, counts)]
    assert min(total) > 0, total


def test_audit_refuses_bad_arguments_before_touching_a_device():
    from armour_amd import _lib
    from armour_amd.path_audit import audit
    robot = _robot("kinova")
    z = np.zeros((1, 7))
    box = np.array([[5.0, 0, 0, 0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1]])
    for kw in (dict(step=0.0), dict(ta=0.6, tb=0.5), dict(tb=1.5), dict(world=1), dict(tube=-np.ones(7)), dict(q0=np.full((1, 7), np.nan))):
        with pytest.raises(_lib.ArmourError) as ei:     # (the device entry: refused although this machine may have no device)
            audit(robot, box, kw.get("world", 0), kw.get("q0", z), z, z, z, K_RANGE, D, kw.get("ta", 0.0), kw.get("tb", 0.5), tube=kw.get("tube"),
                  step=kw.get("step", 0.02))
        assert ei.value.code == _lib.EINVAL, kw
    res = audit(robot, box, 0, z, z, z, z, K_RANGE, D, 0.0, 0.5, host=True)     # a far box, an arm at rest: one item, proved free
    assert res.verdict[0] == 0 and np.isnan(res.t_hit[0])


def test_both_audits_hold_their_pieces_to_the_same_rules():
    """Every single bad piece argument that both audits check: the same code from audit and audit_self, and the same message after the
    entry's name (the device entries as well: refused before a device is touched)."""
    from armour_amd import _lib
    from armour_amd.path_audit import audit, audit_self
    robot = _robot("kinova")
    z = np.zeros((1, 7))
    one = np.ones((1, 7))
    nan = np.full((1, 7), np.nan)
    box = np.array([[5.0, 0, 0, 0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1]])
    bad = [(dict(step=0.0), _lib.EINVAL), (dict(duration=0.0), _lib.EINVAL), (dict(ta=0.6, tb=0.5), _lib.EINVAL), (dict(tb=1.5), _lib.EINVAL),
           (dict(tube=-np.ones(7)), _lib.EINVAL), (dict(q0=nan), _lib.EINVAL), (dict(qd0=nan), _lib.EINVAL), (dict(qdd0=nan), _lib.EINVAL),
           (dict(k=nan), _lib.EINVAL), (dict(k_range=np.full(7, np.nan)), _lib.EINVAL), (dict(k=one, step=1e-12), _lib.ECAPACITY)]
    for kw, code in bad:
        for host in (False, True):
            pieces = (kw.get("q0", z), kw.get("qd0", z), kw.get("qdd0", z), kw.get("k", z), kw.get("k_range", K_RANGE), kw.get("duration", D),
                      kw.get("ta", 0.0), kw.get("tb", 0.5))
            rest = dict(tube=kw.get("tube"), step=kw.get("step", 0.02), host=host)
            said = []
            for entry, call in (("armour_path_audit", lambda: audit(robot, box, 0, *pieces, **rest)),
                                ("armour_path_audit_self", lambda: audit_self(robot, *pieces, **rest))):
                with pytest.raises(_lib.ArmourError) as ei:
                    call()
                assert ei.value.code == code, (kw, host, entry, str(ei.value))
                head = f"armour error {code}: {entry}{'_host' if host else ''}: "
                assert str(ei.value).startswith(head), (kw, host, str(ei.value))
                said.append(str(ei.value)[len(head):])
            assert said[0] == said[1] and said[0], (kw, host, said)


# ----------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(1200)
@pytest.mark.parametrize("name", ["kinova", "gripper", "fetch"])
def test_device_audit_equals_the_restatement_on_the_reference_worlds(name):
    """Random pieces and planned pieces (the first and the braking half of armour_solve's plan of every world's first iteration)."""
    from armour_amd import scenes
    from armour_amd.path_audit import audit
    from armour_amd.planner import ArmourNLP
    robot = _robot(name)
    g = geometry(robot_dict(robot))
    n = g["n"]
    bp = scenes.as_batch(scenes.reference_worlds())
    obs = bp["obstacles"]
    Wn = obs.shape[0]
    rng = np.random.default_rng(29)
    nlp = ArmourNLP(robot=robot, T=32).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], obs)
    k_opt = np.nan_to_num(np.stack([s["k_opt"] for s in nlp.solve()]))        # (whatever the verdict: a plan to audit)
    k_range = np.array(nlp.params.k_range[:n])
    nlp.close()
    z = np.zeros((Wn, n))
    rnd = random_pieces(robot, rng, 2 * Wn, still=0.3)
    planned = (np.tile(bp["q0"], (2, 1)), np.tile(z, (2, 1)), np.tile(z, (2, 1)), np.tile(k_opt, (2, 1)),
               np.repeat([0.0, 0.5 * D], Wn), np.repeat([0.5 * D, D], Wn))
    arrs = tuple(np.concatenate([a, b]) for a, b in zip(rnd, planned))
    world = np.concatenate([rng.integers(0, Wn, 2 * Wn), np.tile(np.arange(Wn), 2)]).astype(np.int32)
    tube = rng.choice([0.0, 0.01], (4 * Wn, 1)) * rng.random((4 * Wn, n))
    total = [0, 0, 0]
    for step, tb_ in ((0.02, None), (0.05, tube)):
        res = audit(robot, obs, world, *arrs[:4], k_range, D, arrs[4], arrs[5], tube=tb_, step=step, clearance=True)
        fast = audit(robot, obs, world, *arrs[:4], k_range, D, arrs[4], arrs[5], tube=tb_, step=step)
        host = audit(robot, obs, world, *arrs[:4], k_range, D, arrs[4], arrs[5], tube=tb_, step=step, clearance=True, host=True)
        assert np.array_equal(res.verdict, fast.verdict) and np.array_equal(res.t_hit, fast.t_hit, equal_nan=True)
        assert np.abs(res.clearance - host.clearance).max() <= CL_TOL
        counts = _compare(res, g, obs, world, arrs, k_range, step, tb_, (name, step))
        print(f"{name} step {step}: proved free / proved hit / undecided = {counts}, device {res.ms:.3f} ms")
        total = [a + b for a, b in zip(total, counts)]
    assert min(total) > 0, total


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_sixteen_worlds_in_one_call_equal_sixteen_calls():
    from armour_amd.path_audit import audit
    robot = _robot("gripper")
    obs = _worlds()[:16]
    rng = np.random.default_rng(31)
    P = 160
    arrs = random_pieces(robot, rng, P, still=0.2)
    world = rng.integers(0, 16, P).astype(np.int32)
    tube = 0.01 * rng.random((P, 7))
    res = audit(robot, obs, world, *arrs[:4], K_RANGE, D, arrs[4], arrs[5], tube=tube, step=0.02, clearance=True)
    assert len(set(res.verdict.tolist())) == 3
    for w in range(16):
        sel = np.flatnonzero(world == w)
        one = audit(robot, obs[w], 0, *(a[sel] for a in arrs[:4]), K_RANGE, D, arrs[4][sel], arrs[5][sel], tube=tube[sel], step=0.02, clearance=True)
        assert np.array_equal(one.verdict, res.verdict[sel]) and np.array_equal(one.t_hit, res.t_hit[sel], equal_nan=True)
        assert np.array_equal(one.clearance, res.clearance[sel])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_a_piece_driven_through_a_box_is_a_proved_hit():
    from armour_amd.path_audit import audit
    robot = _robot("kinova")
    g = geometry(robot_dict(robot))
    q0 = np.array([0.0, 0.6, 0.0, 1.2, 0.0, 0.6, 0.0])
    k = np.array([1.0, 0, 0, 0, 0, 0, 0])
    k_range = np.full(7, 0.8)                                    # a long move of the base joint
    q_mid = q_des(q0, 0 * q0, 0 * q0, k_range * k, 0.5)
    c = link_boxes(g, q_mid[None])[2][0, 5]                      # the forearm's box centre half way
    box = np.array([[c[0], c[1], c[2], 0.05, 0, 0, 0, 0.05, 0, 0, 0, 0.05]])
    z = np.zeros(7)
    res = audit(robot, box, 0, q0, z, z, k, k_range, D, 0.0, D, step=0.01, clearance=True)
    assert res.verdict[0] == 1 and 0.0 < res.t_hit[0] <= 0.5 and res.clearance[0] < 0
    v, th, cl, _ = audit_np(g, box, (q0, z, z, k, 0.0, D), k_range, D, 0.01)
    assert v == 1 and res.t_hit[0] == th and abs(res.clearance[0] - cl) <= CL_TOL
    far = box.copy()
    far[0, 2] += 3.0
    res = audit(robot, far, 0, q0, z, z, k, k_range, D, 0.0, D, step=0.01)
    assert res.verdict[0] == 0 and np.isnan(res.t_hit[0])


def _round_trip_case():
    """(robot, worlds, world_of_piece, pieces, k_range, step) of the smallest audit whose bookkeeping can go wrong: five pieces of 1, 255,
    256, 257 and 1 items in the caller's order [1, 0, 1, 0, 1] of two one-box worlds.  World 0's run (255 + 257 items) crosses a 256-item
    block boundary and ends on one, world 1's (1 + 256 + 1) crosses one; pieces 1 and 3 drive the forearm through world 0's box; piece 4 is
    an arm folded onto itself at rest."""
    from armour_amd.path_audit import audit_items
    robot = _robot("kinova")
    g = geometry(robot_dict(robot))
    q_move = np.array([0.0, 0.6, 0.0, 1.2, 0.0, 0.6, 0.0])
    k_move = np.array([1.0, 0, 0, 0, 0, 0, 0])
    k_range = np.full(7, 0.8)                                    # a long move of the base joint: v_0 = 5 * 0.8 / D = 4
    c = link_boxes(g, q_des(q_move, 0 * q_move, 0 * q_move, k_range * k_move, 0.5)[None])[2][0, 5]      # the forearm's box centre half way
    way = np.array([[c[0], c[1], c[2], 0.05, 0, 0, 0, 0.05, 0, 0, 0, 0.05]])
    far = way.copy()
    far[0, 2] += 3.0
    step = 4.0 * D / 256.5                                       # S = ceil(4 w / step): 257 on [0, D], S on a window of (S - 0.5) / 256.5
    q0 = np.stack([q_move] * 4 + [np.array([0.0, 2.1, 0.0, 2.5, 0.0, 1.0, 0.0])])
    k = np.stack([k_move] * 4 + [np.zeros(7)])
    z = np.zeros((5, 7))
    ta = np.array([0.3, 0.0, 0.002, 0.0, 0.0])
    tb = ta + np.array([0.0, 254.5 / 256.5, 255.5 / 256.5, 1.0, 0.5]) * D
    pieces = (q0, z, z, k, ta, tb)
    assert audit_items(robot, *pieces[:4], k_range, D, ta, tb, step=step).tolist() == [1, 255, 256, 257, 1]
    return robot, np.stack([way, far]), np.array([1, 0, 1, 0, 1], dtype=np.int32), pieces, k_range, step


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_the_shared_round_trip_keeps_its_books_across_blocks_and_worlds():
    """audit and audit_self on the device against their host entries: verdicts and t_hit identical, clearances to CL_TOL, in verdict
    mode and in clearance mode; no piece at all is an empty result and no launch."""
    from armour_amd.path_audit import audit, audit_self
    robot, worlds, world, (q0, qd0, qdd0, k, ta, tb), k_range, step = _round_trip_case()
    seen = set()
    for tag, run in (("world", lambda **kw: audit(robot, worlds, world, q0, qd0, qdd0, k, k_range, D, ta, tb, step=step, **kw)),
                     ("self", lambda **kw: audit_self(robot, q0, qd0, qdd0, k, k_range, D, ta, tb, step=step, **kw))):
        for clearance in (False, True):
            dev, host = run(clearance=clearance), run(clearance=clearance, host=True)
            print(tag, clearance, dev.verdict, dev.t_hit, dev.clearance, host.clearance)
            assert np.array_equal(dev.verdict, host.verdict), (tag, clearance, dev.verdict, host.verdict)
            assert np.array_equal(dev.t_hit, host.t_hit, equal_nan=True), (tag, clearance, dev.t_hit, host.t_hit)
            if clearance:
                assert np.abs(dev.clearance - host.clearance).max() <= CL_TOL, (tag, dev.clearance, host.clearance)
            seen.add((tag, tuple(host.verdict)))
    assert ("world", (0, 1, 0, 1, 0)) in seen and any(t == "self" and v[4] == 1 for t, v in seen), seen     # first_hit was exercised in both
    e = np.zeros((0, 7))
    for res in (audit(robot, worlds, np.zeros(0, dtype=np.int32), e, e, e, e, k_range, D, np.zeros(0), np.zeros(0), step=step, clearance=True),
                audit_self(robot, e, e, e, e, k_range, D, np.zeros(0), np.zeros(0), step=step, clearance=True)):
        assert res.verdict.shape == (0,) and res.t_hit.shape == (0,) and res.clearance.shape == (0,) and res.ms == 0.0
