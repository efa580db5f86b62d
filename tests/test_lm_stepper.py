"""LmStepper of csrc/register_host.h -- the damped iteration as a resumable stepper, which dslam_track_camera_sdf_starts
advances for many starts in lock-step -- against lm_iterate, without a GPU.
tests/stubs/lm_stepper_check.cpp is compiled with g++ against the header alone; it runs lm_check.cpp's kind of synthetic
problems by lm_iterate, by a stepper driven alone and by steppers interleaved round by round, and prints for each run the
evaluation count, the stop reason, the conditioning and, per evaluation, the damping, the verdict and the accepted state,
all as hexadecimal doubles.  Equal text is equal bits."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "denseslam-global-consistency-h_amd", "csrc")
PROBLEMS = ("zero_residual", "max_evaluations", "never_cheaper", "too_few_valid", "at_the_truth", "second", "far_gated")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lm_stepper") / "lm_stepper_check")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                          os.path.join(ROOT, "tests", "stubs", "lm_stepper_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, "register_host.h does not compile alone:\n" + res.stderr
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = {}
    for line in res.stdout.splitlines():
        words = line.split()
        if words[0] == "rounds":
            out["rounds"] = int(words[1])
            continue
        name, how = words[:2]
        fields = dict(zip(words[2:10:2], words[3:10:2]))
        assert words[10] == "trail"
        out[name, how] = dict(evaluations=int(fields["evaluations"]), stop=int(fields["stop"]), accepted_any=int(fields["accepted_any"]),
                              conditioning=fields["conditioning"], trail=[] if words[11] == "-" else words[11:], text=line.split(" ", 2)[2])
    return out


@pytest.mark.parametrize("name", PROBLEMS)
def test_a_stepper_driven_alone_repeats_lm_iterate_bit_for_bit(runs, name):
    assert runs[name, "alone"]["text"] == runs[name, "iterate"]["text"]
    r = runs[name, "alone"]
    assert r["evaluations"] == 1 + len(r["trail"])


@pytest.mark.parametrize("name", PROBLEMS)
def test_interleaved_steppers_keep_each_problem_on_its_own_trajectory(runs, name):
    assert runs[name, "interleaved"]["text"] == runs[name, "iterate"]["text"]


def test_the_problems_cover_every_stop_reason_and_different_lengths(runs):
    """What makes the comparison mean something: every stop reason occurs, rejected steps occur between adopted ones, and
    the problems stop after different numbers of evaluations, so the interleaved rounds run with problems that have already
    stopped next to ones that still move."""
    by = {n: runs[n, "iterate"] for n in PROBLEMS}
    assert {r["stop"] for r in by.values()} == {0, 1, 2, 3}
    assert by["max_evaluations"]["evaluations"] == 3 and by["max_evaluations"]["stop"] == 1
    assert by["never_cheaper"]["evaluations"] == 8 and by["never_cheaper"]["stop"] == 2 and by["never_cheaper"]["accepted_any"] == 0
    assert by["too_few_valid"]["evaluations"] == 1 and by["too_few_valid"]["stop"] == 3 and by["too_few_valid"]["trail"] == []
    assert float.fromhex(by["too_few_valid"]["conditioning"]) == 0.0 < float.fromhex(by["zero_residual"]["conditioning"]) <= 1.0
    verdicts = "".join(step.split(",")[0][-1] for step in by["far_gated"]["trail"])
    assert "A" in verdicts and "R" in verdicts, verdicts
    assert len({r["evaluations"] for r in by.values()}) >= 4
    assert runs["rounds"] == max(r["evaluations"] for r in by.values()) - 1
    # the damping follows the rules: from 1, a tenth after an adopted step (not below 1e-6), tenfold after a rejected one
    for r in by.values():
        lam = 1.0
        for step in r["trail"]:
            head = step.split(",")[0]
            assert float.fromhex(head[:-2]) == lam
            lam = max(lam / 10.0, 1e-6) if head[-1] == "A" else lam * 10.0
