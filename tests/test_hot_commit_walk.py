"""The hot start's commit rule that goes on past an accepted birth or death (csrc/mpp_chain_body.inc, MPP_HOT_PAST; option
``hot_past_births``), walked on the host over the C oracle's trace of the sequential chain (tests/hot_commit_walk.py).

For every record either rule commits, the walk asserts from the sequentially tracked state that the record's speculative
target is the sequential chain's and that no point changed earlier in its round shares a cell with one of its points or lies
within ``conflict_d2`` of it: the two things a record evaluated against the round's first state needs to be the sequential
step (its accept test, taken again with the new population, is the third; dE, the densities, the geometry and the stash do
not depend on n).  The round counts of both rules are pinned: they are what the kernel's gain was estimated from
(profiles/hot_past_births.md).  No GPU."""
import functools

import numpy as np
import pytest

import hot_commit_walk as hw


@functools.lru_cache(maxsize=None)
def traced(tile, n_obj, n_steps):
    props, out, xy0, res, d2 = hw.oracle_trace(tile, n_obj, n_steps, seed=0, T0=1.0, alpha=0.999)
    w2 = hw.target_words(props, out, len(xy0), np.random.default_rng(1))
    assert (res, d2) == (32, 4097)                      # mpp_hrcM: max_inter 32
    return props, out, xy0, w2, res, d2


# (tile, objects, steps walked): rounds under the parent's rule, under the new one, rounds of the new rule that hold a
# committed birth / death, and that hold two or more
PINNED = {(256, 50, 3000): (1261, 1136, 477, 77),
          (512, 200, 2700): (798, 704, 420, 68)}     # the bench tile's hot start


@pytest.mark.parametrize("case", sorted(PINNED))
def test_round_counts_and_every_committed_record(case):
    tile, n_obj, n_steps = case
    props, out, xy0, w2, res, d2 = traced(tile, n_obj, 6000 if tile == 512 else n_steps)
    parent = hw.walk(props, out, xy0, w2, False, res, d2, n_steps=n_steps)
    past = hw.walk(props, out, xy0, w2, True, res, d2, n_steps=n_steps)
    for r in (parent, past):                                # (walk() asserts target and reach for each of them)
        assert r["steps"] == n_steps and r["checked"] == n_steps
    assert max(parent["bd_per_round"]) == 1
    bd = np.array(past["bd_per_round"])
    assert (parent["rounds"], past["rounds"], int((bd > 0).sum()), int((bd >= 2).sum())) == PINNED[case]


def test_handover_statistic_keeps_its_meaning():
    """fed with the steps up to the round's first committed birth / death, the smoothed statistic reaches the default
    handover_at (1 280 / 256 = 5 of 8) where the parent's did, within a few rounds"""
    props, out, xy0, w2, res, d2 = traced(512, 200, 6000)
    parent = hw.walk(props, out, xy0, w2, False, res, d2, handover_at=1280)
    past = hw.walk(props, out, xy0, w2, True, res, d2, handover_at=1280)
    assert (parent["handover"], parent["rounds"]) == (2686, 796)
    assert (past["handover"], past["rounds"]) == (2694, 703)


def test_the_walk_catches_a_rule_that_keeps_a_stale_target():
    """the checks are live: with target words that do not reproduce the traced targets the walk must object"""
    props, out, xy0, w2, res, d2 = traced(256, 50, 3000)
    with pytest.raises(AssertionError):
        hw.walk(props, out, xy0, np.roll(w2, 1), True, res, d2)
