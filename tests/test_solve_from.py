"""armour_solve_from: armour_solve from a start point of the caller's.  NULL / zeros reproduce armour_solve; the host form, the device form and its
culled variant give the same iterates from any start; a start at a converged optimum stays there; bad starts are refused."""
import numpy as np
import pytest

T = 40
FIELDS = ("feasible", "iterations", "evaluations", "status", "cost", "max_violation")


def _same(a, c):
    return np.array_equal(a["k_opt"], c["k_opt"]) and all(a[f] == c[f] for f in FIELDS)


def _agrees_with_full_g(nlp, res):
    g, _ = nlp.eval_g_jac(np.stack([r["k_opt"] for r in res]))
    feas = nlp.finalize_solution(g)
    for b, r in enumerate(res):
        assert bool(feas[b]) == r["feasible"], (b, r)


def test_solve_from_is_declared_and_exported():
    import ctypes as C

    from armour_amd import _lib
    L = _lib.load()
    assert hasattr(L, "armour_solve_from") and "armour_solve_from" in _lib.EXPORTS
    assert L.armour_solve_from.argtypes[2] == C.POINTER(C.c_double)
    import inspect

    from armour_amd.planner import ArmourNLP
    assert list(inspect.signature(ArmourNLP.solve).parameters)[-1] == "k_start"


@pytest.mark.gpu
@pytest.mark.parametrize("seed,B,O", [(5300, 1, 1), (5100, 3, 7), (8, 3, 20)])
def test_null_and_zero_start_equal_armour_solve(seed, B, O):
    import ctypes as C

    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP, _solve_dicts, _solve_options
    from armour_amd.worlds import random_batch
    bp = random_batch(seed, B, O)
    nlp = ArmourNLP(T=T).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    for kw in (dict(), dict(host_qp=True), dict(device_qp=True)):
        ref = nlp.solve(**kw)
        opt = _solve_options(nlp.L, None, None, None, kw.get("host_qp", False), kw.get("device_qp", False))
        res = (_lib.ArmourSolveResult * B)()
        _lib.check(nlp.L.armour_solve_from(nlp.h, C.byref(opt), None, res))          # NULL
        for a, c in zip(ref, _solve_dicts(res, nlp.n)):
            assert _same(a, c), (kw, a, c)
        for a, c in zip(ref, nlp.solve(k_start=np.zeros((B, nlp.n)), **kw)):          # +0.0
            assert _same(a, c), (kw, a, c)
        _agrees_with_full_g(nlp, ref)
    nlp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,B,O", [(5300, 1, 1), (5100, 3, 7), (8, 3, 20)])
def test_forms_agree_from_halton_starts(seed, B, O):
    """The invariant of tests/test_solve.py, from starts other than 0: host form = device form = culled device form, bit for bit."""
    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP, sweep_candidates
    from armour_amd.worlds import random_batch
    bp = random_batch(seed, B, O)
    nlp = ArmourNLP(T=T).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    cand = sweep_candidates(nlp.n, 1 + 3 * B)
    moved = False
    for trial in range(3):
        start = cand[1 + trial * B:1 + (trial + 1) * B]
        host = nlp.solve(host_qp=True, k_start=start)
        nlp.set_option(_lib.OPT_SOLVE_CULL, 0)
        dev = nlp.solve(device_qp=True, k_start=start)
        nlp.set_option(_lib.OPT_SOLVE_CULL, 1)
        cul = nlp.solve(device_qp=True, k_start=start)
        nlp.set_option(_lib.OPT_SOLVE_CULL, -1)
        for a, c, d in zip(host, dev, cul):
            assert _same(a, c) and _same(a, d), (trial, a, c, d)
        _agrees_with_full_g(nlp, host)
        zero = nlp.solve(host_qp=True)
        moved = moved or any(a["evaluations"] != z["evaluations"] or not np.array_equal(a["k_opt"], z["k_opt"]) for a, z in zip(host, zero))
    assert moved   # (the start is really taken: some solve differs from the one that starts at 0)
    # the extreme corner of the box is a legal start
    corner = np.ones((B, nlp.n))
    for a, c in zip(nlp.solve(host_qp=True, k_start=corner), nlp.solve(device_qp=True, k_start=corner)):
        assert _same(a, c), (a, c)
    nlp.close()


@pytest.mark.gpu
def test_start_at_a_converged_optimum_stays_there():
    from armour_amd import scenes
    from armour_amd.planner import ArmourNLP
    worlds = scenes.reference_worlds()[:3]
    bt = scenes.as_batch(worlds)
    nlp = ArmourNLP(T=T).set_parameters(bt["q0"], bt["qd0"], bt["qdd0"], bt["q_des"], bt["obstacles"])
    tol = 1e-4                                                       # the solver's default tolerance (armour_solve_options_default)
    first = nlp.solve()
    assert all(r["feasible"] and r["status"] == 1 for r in first)
    again = nlp.solve(k_start=np.stack([r["k_opt"] for r in first]))
    for a, c in zip(first, again):
        assert c["feasible"] and c["iterations"] <= 2, c
        assert abs(c["cost"] - a["cost"]) <= tol * max(1.0, abs(a["cost"])), (a["cost"], c["cost"])
    _agrees_with_full_g(nlp, again)
    nlp.close()


@pytest.mark.gpu
def test_bad_starts_are_refused():
    from armour_amd import _lib
    from armour_amd.planner import ArmourNLP
    from armour_amd.worlds import random_batch
    bp = random_batch(5300, 1, 1)
    nlp = ArmourNLP(T=T).set_parameters(bp["q0"], bp["qd0"], bp["qdd0"], bp["q_des"], bp["obstacles"])
    for bad in (1.0 + 1e-12, -1.5, np.nan, np.inf):
        start = np.zeros((1, nlp.n))
        start[0, 3] = bad
        for kw in (dict(host_qp=True), dict(device_qp=True)):
            with pytest.raises(_lib.ArmourError) as ei:
                nlp.solve(k_start=start, **kw)
            assert ei.value.code == _lib.EINVAL
    assert _same(nlp.solve()[0], nlp.solve(k_start=np.zeros((1, nlp.n)))[0])   # the handle still solves
    nlp.close()
