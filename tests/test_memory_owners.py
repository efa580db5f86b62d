"""The owners of csrc/dslam_memory.h (device buffer, page-locked buffer, event) on their failure paths, without a GPU:
tests/stubs/hip_stub/owners_check.cpp is compiled with g++ against the header and a counting stand-in for the HIP calls
it makes (tests/stubs/hip_stub/hip/hip_runtime.h: live allocations counted, abort on a double free or a foreign pointer,
the n-th allocating call made to fail).  For every n up to the group size the program checks that a group of five buffers
and an event allocated the way the handles do it -- built aside, move-assigned when complete -- leaves the handle and the
live count untouched when allocation n fails, that a retry succeeds and that destruction frees everything; the same for
both kinds of regrow (old buffer and size kept / buffer empty and size 0), for move and swap (nothing allocated or freed)
and for a scene on borrowed voxels (the caller's pointer never reaches hipFree)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "stubs", "hip_stub")
CSRC = os.path.join(ROOT, "denseslam-global-consistency-h_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("owners") / "owners_check")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", STUB, "-I", CSRC,
                          os.path.join(STUB, "owners_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, "dslam_memory.h does not compile alone against the HIP stand-in:\n" + res.stderr
    return exe


def test_owners_survive_every_failed_allocation(program):
    res = subprocess.run([program], capture_output=True, text=True)
    assert res.returncode == 0 and "owners ok" in res.stdout, res.stdout + res.stderr


def test_the_check_would_notice_the_old_guard(program):
    """Not vacuous: the guard batch_scratch had before the owners (raw pointers, the group's first pointer tested for all
    of it) fails the same group check -- a failed allocation leaves the handle holding part of the group."""
    res = subprocess.run([program, "parent-guard"], capture_output=True, text=True)
    assert res.returncode == 1 and "held(h) == 0" in res.stderr, res.stdout + res.stderr
