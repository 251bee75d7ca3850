"""The commit decision of a deep round is a function of the round's reports that needs no order (csrc/mpp_commit.hpp).

tests/commit_walk.hip is compiled for the host with -fsanitize=address,undefined and run as a program: on random windows of
1 .. 256 packed reports it takes the decision twice -- with the serial loop the kernel ran before (one iteration per
committed changing step) and in the form phase C of csrc/mpp_deep.hip has now (the relevant changing steps dealt to eight
waves, their first conflicts combined by minimum) -- and compares ``committed``, the error, the population, the commit mask
and whether a second pass is needed.  Both call the pair test of the header, the one the kernel calls."""
import os
import re
import subprocess

import pytest

from mpp_cnn_rs_object_detection_amd import build as mpp_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("commit") / "commit_walk")
    cmd = [mpp_build.HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(HERE, "commit_walk.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode in (0, 1), (r.stdout[-500:], r.stderr[-4000:])
    out = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}
    assert out.get("windows", 0) > 0, (r.stdout[-500:], r.stderr[-4000:])
    return out, r.stderr


def test_split_decision_equals_the_serial_loop(walk):
    out, err = walk
    assert out["windows"] >= 50000
    assert out["mismatches"] == 0, err[-2000:]


def test_every_way_a_round_ends_is_covered(walk):
    """a lopsided generator would hide a branch: each of the three ends takes at least 5 % of the windows"""
    out, _ = walk
    for k in ("end_conflict", "end_invalid", "end_T"):
        assert out[k] >= 0.05 * out["windows"], (k, out)
    # ... and the rarer outcomes occur: the three errors, a second pass, more than 8 committed changing steps (every wave
    # has tested at least one, some two)
    for k in ("err_point", "err_cell", "err_bad", "any_apply", "committed_over8", "end_none"):
        assert out[k] > 0, (k, out)
