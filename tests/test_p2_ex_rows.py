"""The exact-layout (EX) kernels' rows, bit for bit against a recording (tests/golden/p2_ex_rows.npz, made by tests/golden/make_p2_ex_rows.py).

tests/test_p2_role_rows.py records O = 1 and O = 3, where no launch is an EX launch; the shapes here are (see the generator).  Where the
collision block gets its addresses from -- the launch plan's scalars or its own arithmetic, 32 or 64 bits -- and how it sorts its wave-uniform
choices must leave every double as it was: the comparison is on the uint64 view, through the asynchronous device entry, a prepared 3-step
graph, the two-point launch (either point) and the synchronous host call.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_p2_ex_rows as gen  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "p2_ex_rows.npz")


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_fixture_matches_the_generators_declaration(recorded):
    assert os.path.getsize(FIXTURE) < (1 << 20)
    want = {}
    for name in gen.CASES:
        want.update(gen.declared_shapes(name))
    assert set(recorded) == set(want)
    for key, shape in want.items():
        assert recorded[key].shape == shape and recorded[key].dtype == np.float64, key
    for name in gen.CASES:
        z = f"{name}__z__"
        assert not recorded[z + "k"].any() and not recorded[z + "qd0"].any() and not recorded[z + "qdd0"].any()
        a = recorded[f"{name}__a__k"]
        assert np.all(a[1] == 1.0) and np.all(a[2] == -1.0) and np.abs(a[0]).max() < 1.0
        assert not np.isnan(recorded[f"{name}__a__g"]).any() and not np.isnan(recorded[z + "jac"]).any()


@pytest.fixture(scope="module")
def handles(recorded):
    """One handle per (case, problem set), built from the recorded inputs and shared by the entries."""
    made = {}

    def get(name, s):
        if (name, s) not in made:
            inputs = {key: recorded[f"{name}__{s}__{key}"] for key in gen.INPUT_KEYS}
            made[(name, s)] = gen.make_nlp(name, inputs)
        return made[(name, s)]

    yield get
    for nlp in made.values():
        nlp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(gen.CASES))
def test_the_cases_are_ex_launches(handles, name):
    """What the recording is for: every case takes the EX kernel, with the mask shared and by value, and the d column as the case says."""
    for s in gen.SETS:
        v, f = gen.plan_verdict(handles(name, s))
        assert v["exact"] == 1 and v["six"] == 1 and v["shared"] == 1 and v["by_value"] == 1 and v["dfc"] == int(gen.CASES[name][4]), (name, s, v)
        assert f[0] > 0 and f[4] > 0 and f[5] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("entry", gen.ENTRIES)
@pytest.mark.parametrize("name", list(gen.CASES))
def test_rows_are_the_recorded_bits(recorded, handles, name, entry):
    for s in gen.SETS:
        pre = f"{name}__{s}__"
        nlp = handles(name, s)
        g, jac = gen.role.evaluate(nlp, recorded[pre + "k"], entry)
        for what, got, ref in (("g", g, recorded[pre + "g"]), ("jac", jac, recorded[pre + "jac"])):
            bad = np.argwhere(np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(ref).view(np.uint64))
            assert got.shape == ref.shape and len(bad) == 0, f"{name}/{s} {entry}: {len(bad)} entries of {what} differ, first at {bad[:4].tolist()}"
