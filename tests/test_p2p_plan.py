"""CPU test of the P2P launch planner (ggrs_amd/csrc/p2p_plan.h): a host program built around the
header (tests/native/p2p_plan_host.cpp) plans every case of tests/p2p_plan_cases.json, and its
launch sequences must be the ones recorded from the commit before the planner existed (that
commit with a logging line at each launch site, run on an MI355X; the fixture says which cases
were worked out from its source instead).  Independent of the fixture: every advance's launches
sum to its calls, no launch exceeds the limit its form states, none takes more LDS than a CU has,
and planning an input twice gives the same launch."""
import json
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = json.load(open(os.path.join(HERE, "p2p_plan_cases.json")))
CASES = FIXTURE["cases"]
CUS = FIXTURE["num_cus"]

# ggrs_amd/csrc/p2p_plan.h
CHAIN_LDS_ROWS = 16 * 1024
CHAIN_FAST_LDS = 40 * 1024
CHAIN_MAX_CALLS = 2000
LDS_PER_CU = 160 * 1024


def case_line(c):
    adv = [len(c["advances"])] + c["advances"]
    if c["mode"] == "fixed":
        dbg = {"none": 0, "armed": 1, "disarmed": 2}[c["dbg"]]
        f = ["fixed", c["sessions"], c["players"], c["local_mask"], c["latency"], c["delay"], c["max_prediction"],
             c["capacity"], c["predictor"], int(c["sparse"]), int(c["trace"]), int(c["desync"] > 0), dbg, c["form"], CUS]
    else:
        env = [c["env"].get(k, "-") for k in ("GGRS_SCHED_SPLIT", "GGRS_SCHED_CHAINS", "GGRS_SCHED_K")]
        f = ["sched", c["sessions"], c["players"], c["local_mask"], c["delay"], c["max_prediction"], c["capacity"],
             c["predictor"], int(c["sparse"]), int(c["desync"] > 0), int(c["peer_reports"]), int(c["trace"]), CUS] + env
    return " ".join(str(x) for x in f + adv)


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """every case's output lines, from one run of the host program"""
    exe = str(tmp_path_factory.mktemp("plan") / "p2p_plan_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "ggrs_amd", "csrc"), os.path.join(HERE, "native", "p2p_plan_host.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], input="".join(case_line(c) + "\n" for c in CASES), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    per_case = [blk.strip().split("\n") for blk in r.stdout.split("CASE\n")[1:]]
    assert len(per_case) == len(CASES)
    return {c["name"]: lines for c, lines in zip(CASES, per_case)}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_matches_the_recorded_launches(planned, case):
    assert planned[case["name"]] == case["expected"]


def fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_invariants(planned, case):
    lines = planned[case["name"]]
    assert "UNSTABLE" not in lines  # the same input planned twice
    pp = {1: 1, 2: 2, 3: 4, 4: 4}[case["players"]]
    frame = 0
    for n in case["advances"]:
        assert lines[0] == "ADVANCE %d" % n
        lines = lines[1:]
        ran = 0
        while lines and not lines[0].startswith("ADVANCE"):
            line, lines = lines[0], lines[1:]
            if line.startswith("ERROR"):
                assert not lines  # an error ends the case
                return
            f = fields(line)
            assert f["f0"] == frame + ran and f["n"] >= 1
            assert f["lds"] <= LDS_PER_CU
            kind = line.split()[0]
            if kind == "chains":  # the launch's input rows in LDS; the fast form's whole budget
                rows = f["n"] + 2 * case["latency"] + case["delay"]
                assert rows * f["spw"] * pp <= CHAIN_LDS_ROWS
                if f["fast"]:
                    assert f["lds"] <= CHAIN_FAST_LDS
            if kind == "sched_chains":
                assert f["n"] <= CHAIN_MAX_CALLS
            if kind in ("sched", "sched_chains"):
                assert f["n"] <= case["capacity"]
            ran += f["n"]
        assert ran == n
        frame += n
    assert not lines
