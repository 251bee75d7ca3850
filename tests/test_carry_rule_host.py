"""Which reports of a deep round stay trustworthy for the next one (csrc/mpp_commit.hpp, ``carry_keeps``; option
``deep_carry``).

tests/carry_walk.hip is compiled for the host with -fsanitize=address,undefined and run as a program: on random windows of
1 .. 256 packed reports it forms the kept mask twice -- by the definition, a plain double loop over the outcome of the serial
commit loop, and in the form phase C of csrc/mpp_deep.hip has (the relevant changing steps dealt to eight waves, each testing
its steps against all later reports and noting per report the lowest step that conflicts with it, the rule applied once the
committed count is known) -- and compares them report for report; the committed count and the population of the dealt form
must be the serial loop's, as in tests/commit_walk.hip.  Both call the pair test and the rule of the header, the ones the
kernel calls."""
import os
import re
import subprocess

import pytest

from mpp_cnn_rs_object_detection_amd import build as mpp_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("carry") / "carry_walk")
    cmd = [mpp_build.HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(HERE, "carry_walk.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode in (0, 1), (r.stdout[-500:], r.stderr[-4000:])
    out = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}
    assert out.get("windows", 0) > 0, (r.stdout[-500:], r.stderr[-4000:])
    return out, r.stderr


def test_dealt_kept_mask_equals_the_definition(walk):
    out, err = walk
    assert out["windows"] >= 50000
    assert out["mismatches"] == 0, err[-2000:]


def test_commit_count_is_the_serial_loops(walk):
    out, err = walk
    assert out["commit_mismatches"] == 0, err[-2000:]


def test_every_reason_to_drop_a_report_is_covered(walk):
    """a lopsided generator would hide a clause of the rule: reports are kept in at least a quarter of the windows, and of the
    valid reports behind a round's end each clause drops some -- a conflict with a committed change, the report the round ended
    at, a committed birth / death, a report that changes the state"""
    out, _ = walk
    assert out["windows_kept"] >= 0.25 * out["windows"], out
    assert out["kept"] >= 0.1 * out["behind"], out
    for k in ("lost_conflict", "lost_S", "lost_pop", "lost_chg"):
        assert out[k] >= 1000, (k, out)
