"""Numbers read from the reference checkout, recorded so that the tests comparing against them run without it.

tests/golden/reference_constants.json: the robot tables of RT/KinovaWithoutGripperInfo.h, RT/KinovaInfo.h, CMP/FetchInfo.h
and the planner parameters of RT/Parameters.h (+ t_plan of RT/armour_main.cu:80), as oracle/gen_robot_tables.py parses them.
tests/golden/reference_inputs.json: the SHA-256 of every saved random world (kinova_src/saved_worlds/random/*.csv) and
start / goal of every hard scenario, the (uncommented) MATLAB statements of KSI/kinova_scenarios/get_kinova_scenario_info.m
read as text and evaluated.

tests/test_robot_constants.py and tests/test_reference_scenes.py check the repository against these files everywhere, and
these files against a fresh reading of the reference where its checkout exists.  Run there:
python tests/golden/make_reference_fixtures.py
"""
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import gen_robot_tables as g  # noqa: E402

REF_SCENARIOS = "/root/reference/kinova_src/kinova_simulator_interfaces/kinova_scenarios/get_kinova_scenario_info.m"
REF_SCENES = "/root/reference/kinova_src/saved_worlds/random"
CONSTANTS = os.path.join(HERE, "reference_constants.json")
INPUTS = os.path.join(HERE, "reference_inputs.json")


def constants_from_reference():
    return {"robots": {name: g.robot_from_header(name) for name in g.HEADERS}, "params": g.params_from_reference()}


def inputs_from_reference():
    names = sorted(f for f in os.listdir(REF_SCENES) if f.endswith(".csv"))
    digests = {f: hashlib.sha256(open(os.path.join(REF_SCENES, f), "rb").read()).hexdigest() for f in names}
    text = open(REF_SCENARIOS).read()
    blocks = re.split(r"\n\s*case (\d) %", text)
    scenarios = {}
    for k in range(1, len(blocks), 2):
        case, body = blocks[k], blocks[k + 1]
        scenarios[case] = {}
        for field in ("start", "goal"):
            m = [ln for ln in body.splitlines() if re.match(rf"\s*{field} = \[", ln)]     # (commented alternatives start with %)
            vec = re.search(r"\[(.*?)\]", m[0]).group(1)
            scenarios[case][field] = [float(eval(x.strip(), {"pi": np.pi})) for x in re.split(r"[;,]", vec) if x.strip()]
    return {"saved_worlds_sha256": digests, "hard_scenarios": scenarios}


def load(path):
    with open(path) as f:
        return json.load(f)


if __name__ == "__main__":
    for path, data in ((CONSTANTS, constants_from_reference()), (INPUTS, inputs_from_reference())):
        with open(path, "w") as f:
            json.dump(data, f, indent=1)
            f.write("\n")
        print("wrote", path)
