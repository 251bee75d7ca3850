"""The book of one round of the local descent (csrc/mpp_round.hpp, ``descent_book``: the function ``k_descent_round`` calls, for
``mpp_descend`` and -- births only -- for ``mpp_birth_complete``) against the two kernels and the two records per chain it
replaced.

tests/round_walk.hip is compiled for the host with -fsanitize=address,undefined and run as a program: random sequences of rounds
(capacity 1 .. 16, round limit 1 .. 6, deaths, births or both, a start count of 0 .. capacity or -1, the error state; values
+-m 2^e, so that the order of the additions shows in the bits) are walked through the header's function and through a
transcription of the former ``k_complete_round`` + ``k_descent_round`` pair, and after every round every field of the report,
the chain's count and its error word are compared, the doubles by their bits."""
import os
import re
import subprocess

import pytest

from mpp_cnn_rs_object_detection_amd import build as mpp_build

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("round") / "round_walk")
    cmd = [mpp_build.HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(HERE, "round_walk.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode in (0, 1), (r.stdout[-500:], r.stderr[-4000:])
    out = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout)}
    assert out.get("sequences", 0) > 0, (r.stdout[-500:], r.stderr[-4000:])
    return out, r.stderr


def test_the_one_book_equals_the_two_kernels(walk):
    out, err = walk
    assert out["sequences"] >= 50000
    assert out["mismatches"] == 0, err[-2000:]
    assert out["still_open"] == 0, out          # (max_rounds changing rounds and the one that closes: the host loop's bound)


def test_the_completions_record_is_the_descent_reports(walk):
    """what = births: status, rounds, n_added, n_after and gain as mpp_birth_complete takes them from the descent report are
    those the former second record held"""
    out, _ = walk
    assert out["complete_mismatches"] == 0, out


def test_every_clause_of_the_rule_is_walked(walk):
    """a lopsided generator would hide a clause: every final status ends sequences, rounds change the chain in both halves,
    births that do not fit follow booked deaths, the births' gain is summed across rounds, and the error state is a start"""
    out, _ = walk
    for k in ("end0", "end1", "end2", "both_halves", "full_after_deaths", "births_two_rounds", "from_error"):
        assert out[k] >= 1000, (k, out)
