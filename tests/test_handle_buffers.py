"""State carried in a handle: one planner handle and one roadmap handle taken up and down in size across every lazily grown device buffer
(table, relevance, sweep, bounds, solver and reach-set buffers, on the device and page-locked; the roadmap's world buffers).  A buffer is fresh on the first problem set,
grown on the second, and large enough -- kept -- on the third.  Every output must equal, bit for bit, that of a fresh handle given only
that problem set: the expected values are the same library's, parity with the oracle stays in test_p1_parity / test_sweep /
test_row_relevance / test_solve."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8
SETS = [(1, 1), (3, 4), (1, 1)]   # (B, O); the third set is the first one again


def _problems(B, O):
    from armour_amd.worlds import random_batch
    return random_batch(500 + 10 * B + O, B, O)


def _put_solve(out, name, results):
    for key in ("k_opt", "cost", "max_violation", "feasible", "iterations", "evaluations", "status"):   # (not time_ms)
        out[name + "." + key] = np.array([r[key] for r in results])


def _put_violations(out, name, viol):
    for key in viol[0]:
        out[name + "." + key] = np.array([v[key] for v in viol])


def _outputs(nlp, bp):
    """armour_eval_violations on the relevant rows, armour_sweep over two tiles and one candidate, armour_solve in its culled device form.
    Then the two solve forms in turn -- device, host, host with a row buffer of two rows per segment (the overflow fallback: the whole g and
    jac come over), device again -- so that the page-locked buffers of each form are taken up after the other form's, twice; and
    armour_eval_violations at a k outside the box, which takes every row."""
    from armour_amd import _lib
    from armour_amd.planner import sweep_candidates
    from armour_amd.worlds import random_k
    nlp.set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    out = {}
    k = random_k(7, nlp.B, nlp.n) * 0.5
    _put_violations(out, "viol", nlp.eval_violations(k))
    sw = nlp.sweep(sweep_candidates(nlp.n, 2 * _lib.load().armour_sweep_tile() + 1))
    out["sweep.records"], out["sweep.best"] = sw["records"], sw["best"]
    _put_solve(out, "solve", nlp.solve(device_qp=True))
    _put_solve(out, "solve_device_1", nlp.solve(device_qp=True))
    _put_solve(out, "solve_host", nlp.solve(host_qp=True))
    nlp.set_option(_lib.OPT_SOLVE_ROW_CAP, 2)
    _put_solve(out, "solve_host_overflow", nlp.solve(host_qp=True))
    nlp.set_option(_lib.OPT_SOLVE_ROW_CAP, 0)
    _put_solve(out, "solve_device_2", nlp.solve(device_qp=True))
    k_out = k.copy()
    k_out[-1, 0] = 1.5
    _put_violations(out, "viol_outside_box", nlp.eval_violations(k_out))
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


def _both_forms():
    """the device form and then the host form of armour_solve on one handle, B = 2"""
    nlp = _new_planner()
    bp = _problems(2, 4)
    nlp.set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    out = {}
    _put_solve(out, "device", nlp.solve(device_qp=True))
    _put_solve(out, "host", nlp.solve(host_qp=True))
    nlp.close()
    return {key: np.ascontiguousarray(v).tobytes().hex() for key, v in out.items()}


def _timing_child():
    print("both forms: " + json.dumps(_both_forms()), flush=True)


@pytest.mark.gpu
def test_solve_timing_trace_changes_no_result():
    """ARMOUR_SOLVE_TIMING (read once per process, hence the child): the device form's phase stamps go into a page-locked buffer of their
    own beside the host form's mirrors; the results of both forms are those of a process without the variable."""
    want = _both_forms()
    env = dict(os.environ, ARMOUR_SOLVE_TIMING="1")
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_handle_buffers as t; t._timing_child()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("both forms: ")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    assert "[armour_solve, device form]" in r.stderr and "[armour_solve] B=2" in r.stderr, r.stderr[-3000:]   # (the trace was on, in both forms)
    assert json.loads(lines[0][len("both forms: "):]) == want


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
