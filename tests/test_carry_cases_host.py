"""The host walk of kept reports (tests/carry_cases.py) on the chain bench.py times and on the chains of
tests/test_gpu_deep_carry.py.  No GPU is used.

The bench chain's counts are the ones profiles/deep_carry.md sets the kernel's fresh evaluations against: they are pinned.
The GPU cases are held to floors counted on the oracle alone: a case without rounds that end by a same-slot and by a distance
conflict, without reports kept over several rounds, or without kept reports that a later commit invalidates, would compare
two runs that agree whatever the kernel does with its kept bit."""
import pytest

import carry_cases as cc


def test_bench_chain_counts():
    """steps 2 694 .. 100 000 of the bench chain at deep_gain 12: the walk's rule is harsher than commit_conflict (the full
    interaction range for every pair), so it has more and shorter rounds than the kernel (1 589 rounds, 157 122 window steps)"""
    w = cc.bench_chain_walk()
    assert (w["rounds"], w["window_steps"], w["fresh"]) == (1864, 165157, 113017), w
    assert w["ends"] == {"slot": 528, "distance": 712, "cell": 5, "birth_death": 217, "none": 402}, w
    assert sum(w["ends"].values()) == w["rounds"]
    # what keeping saves: a third of the windows' steps are not evaluated again
    assert 0.30 < 1.0 - w["fresh"] / w["window_steps"] < 0.33


@pytest.mark.parametrize("name", cc.CASES)
def test_gpu_cases_meet_the_floors(name):
    w = cc.case_walk(name)
    print(name, w)
    assert w["ends"]["slot"] >= cc.FLOORS["slot"], w
    assert w["ends"]["distance"] >= cc.FLOORS["distance"], w
    assert w["kept_twice"] >= cc.FLOORS["kept_twice"], w
    assert w["kept_lost"] >= cc.FLOORS["kept_lost"], w
    assert w["fresh"] < w["window_steps"]


def test_a_fixed_depth_walks_too():
    """the walk at the fixed depths of the GPU cases: deeper windows hold more steps behind the end, hence more to keep"""
    import same_value_cases as sv
    b = sv.build("tile112")
    out, props, _ = sv.oracle_chain("tile112")
    res, r2 = cc.geometry(b)
    kept = {}
    for fixed in (8, 64):
        w = cc.walk(props, out, b.xy, b.mk, 0, res, r2, fixed=fixed)
        assert w["window_steps"] >= b.steps and sum(w["ends"].values()) == w["rounds"]
        kept[fixed] = w["window_steps"] - w["fresh"]
    assert kept[64] > kept[8] > 0
