"""State carried in a handle: one planner handle and one roadmap handle taken up and down in size across every lazily grown device buffer
(table, relevance, sweep, bounds, solver and reach-set buffers; the roadmap's world buffers).  A buffer is fresh on the first problem set,
grown on the second, and large enough -- kept -- on the third.  Every output must equal, bit for bit, that of a fresh handle given only
that problem set: the expected values are the same library's, parity with the oracle stays in test_p1_parity / test_sweep /
test_row_relevance / test_solve."""
import numpy as np
import pytest

T = 8
SETS = [(1, 1), (3, 4), (1, 1)]   # (B, O); the third set is the first one again


def _problems(B, O):
    from armour_amd.worlds import random_batch
    return random_batch(500 + 10 * B + O, B, O)


def _outputs(nlp, bp):
    """armour_eval_violations on the relevant rows, armour_sweep over two tiles and one candidate, armour_solve in its culled device form."""
    from armour_amd import _lib
    from armour_amd.planner import sweep_candidates
    from armour_amd.worlds import random_k
    nlp.set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    out = {}
    viol = nlp.eval_violations(random_k(7, nlp.B, nlp.n) * 0.5)
    for key in viol[0]:
        out["viol." + key] = np.array([v[key] for v in viol])
    sw = nlp.sweep(sweep_candidates(nlp.n, 2 * _lib.load().armour_sweep_tile() + 1))
    out["sweep.records"], out["sweep.best"] = sw["records"], sw["best"]
    for key in ("k_opt", "cost", "max_violation", "feasible", "iterations", "evaluations", "status"):   # (not time_ms)
        out["solve." + key] = np.array([r[key] for r in nlp.solve(device_qp=True)])
    return out


def _new_planner():
    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP
    return ArmourNLP(T=T).set_option(_lib.OPT_CULL_ROWS, 1).set_option(_lib.OPT_SOLVE_CULL, 1)


def _same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, key)


@pytest.mark.gpu
def test_planner_handle_up_and_down_in_size():
    kept = _new_planner()
    got = []
    for i, (B, O) in enumerate(SETS):
        bp = _problems(B, O)
        got.append(_outputs(kept, bp))
        fresh = _new_planner()
        _same(got[-1], _outputs(fresh, bp), "set %d (B = %d, O = %d) against a fresh handle" % (i, B, O))
        fresh.close()
    _same(got[2], got[0], "the third set against the first")
    kept.close()   # armour_destroy returns, and a handle made afterwards works
    again = _new_planner()
    _same(_outputs(again, _problems(*SETS[0])), got[0], "a handle made after armour_destroy")
    again.close()


def _worlds(W):
    from armour_amd.worlds import random_problem
    return np.stack([random_problem(900 + w, 3)["obstacles"] for w in range(W)])


@pytest.mark.gpu
def test_roadmap_handle_up_and_down_in_worlds():
    from armour_amd.planner import kinova_robot
    from armour_amd.roadmap import Roadmap
    robot = kinova_robot()
    n = robot.num_factors
    nodes = np.random.default_rng(5).uniform(-1.5, 1.5, (8, n))
    edges = [[0, 1], [1, 2], [2, 5], [3, 7], [4, 6]]
    kept = Roadmap(robot, nodes, edges, edge_step=0.1)
    for i, (W, clearance) in enumerate([(1, False), (3, True), (1, False)]):
        obs = _worlds(W)
        got = kept.check(obs, clearance=clearance)
        fresh = Roadmap(robot, nodes, edges, edge_step=0.1)
        want = fresh.check(obs, clearance=clearance)
        fresh.close()
        assert got["node_free"].shape == (W, 8) and got["edge_free"].shape == (W, len(edges))
        for key in ("node_free", "edge_free") + (("node_clearance",) if clearance else ()):
            assert got[key].tobytes() == want[key].tobytes(), (i, W, key)
    kept.close()   # armour_roadmap_destroy returns, and a handle made afterwards works
    again = Roadmap(robot, nodes, edges, edge_step=0.1)
    assert again.check(_worlds(1))["node_free"].shape == (1, 8)
    again.close()
