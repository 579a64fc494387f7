"""CPU tests of tests/walk_frames.py: the counters' names against the sources that define the slots, and the variant child runner
on targets that touch neither the library nor torch, against a stand-in for the variant library."""
import os
import re

import numpy as np
import pytest

from tests.walk_frames import CSRC, PROF_SLOTS, run_in_variant


def echo(n):
    """a child target: its string argument as a range, and the library path the child was given"""
    return {"x": np.arange(int(n)), "so": np.array(os.environ["MINIPATH_HIP_SO"])}


def broken(n):
    raise ValueError(f"no frame number {n}")


def test_one_name_per_slot():
    with open(os.path.join(CSRC, "family_launch.h")) as f:
        slots = int(re.search(r"constexpr int kProfSlots = (\d+);", f.read()).group(1))
    with open(os.path.join(CSRC, "prof_counters.h")) as f:
        listed = re.findall(r"^//\s+\[(\d+)\] ", f.read(), re.M)
    assert len(PROF_SLOTS) == slots and len(set(PROF_SLOTS)) == slots
    assert [int(i) for i in listed] == list(range(slots)), listed


@pytest.fixture
def stand_in(tmp_path):
    """a directory with a file of the name a variant `standin` would have"""
    so = tmp_path / "libminipath_hip_standin.so"
    so.write_bytes(b"")
    return str(tmp_path), str(so)


def test_child_round_trip(stand_in, tmp_path):
    csrc, so = stand_in
    got = run_in_variant("standin", "tests.test_walk_frames_cpu:echo", tmp_path, "7", timeout=120, csrc=csrc)
    assert sorted(got) == ["so", "x"]
    assert np.array_equal(got["x"], np.arange(7)) and got["x"].dtype == np.arange(7).dtype
    assert str(got["so"]) == so


def test_child_failure_shows_its_traceback(stand_in, tmp_path):
    with pytest.raises(AssertionError, match=r"ValueError: no frame number 3"):
        run_in_variant("standin", "tests.test_walk_frames_cpu:broken", tmp_path, "3", timeout=120, csrc=stand_in[0])


def test_missing_variant_library(tmp_path):
    with pytest.raises(pytest.fail.Exception, match=r"libminipath_hip_absent\.so missing: run build\(\) first"):
        run_in_variant("absent", "tests.test_walk_frames_cpu:echo", tmp_path, "1", timeout=120, csrc=str(tmp_path))
    with pytest.raises(pytest.fail.Exception, match=re.escape(os.path.join(CSRC, "libminipath_hip_absent.so"))):
        run_in_variant("absent", "tests.test_walk_frames_cpu:echo", tmp_path, "1", timeout=120)
