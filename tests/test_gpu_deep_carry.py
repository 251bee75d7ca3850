"""Queue rounds of the deep-round kernel keep the reports behind a round's end that no change the round committed conflicts
with (csrc/mpp_commit.hpp, ``carry_keeps``; option ``deep_carry``, default 1): the lane that gets such a step in the next
round does not evaluate it again and leaves the report as it is.

None of it may change the chain or a round: every case runs the same call with the option on and off and compares the final
configurations byte for byte with each other and with the C oracle's chain, and the rounds, evaluated and committed steps
and rounds with a change of ``deep_stats()`` with each other.  A report kept that should not have been makes a round commit
a step evaluated against a state that is no longer there: the chain, or at least a round count, differs.

The cases (tests/carry_cases.py) are chains in which, on the oracle, rounds end by a same-slot and by a distance conflict, and
reports are kept over several rounds and lost again (tests/test_carry_cases_host.py holds them to floors); all run eight
waves in queue rounds."""
import functools

import numpy as np
import pytest

import carry_cases as cc
import same_value_cases as sv
from mpp_cnn_rs_object_detection_amd import hip_api

pytestmark = pytest.mark.gpu

STAT_KEYS = ("rounds", "evaluated", "committed", "rounds_with_change")
# depth: (deep, deep_fixed)
DEPTHS = {"adaptive": (128, 0), "fixed-8": (128, 8), "fixed-64": (128, 64), "fixed-256": (256, 256)}


def make_ctx(b, depth, carry, **caps):
    deep, fixed = DEPTHS[depth]
    caps.setdefault("point_capacity", 256)
    ctx = hip_api.MppContext(0, spec_waves=8, deep=deep, **caps)
    ctx.set_maps(b.det, b.marks)
    ctx.set_model(b.model, b.maps)
    ctx.set_kernels(b.kd, intensity=np.full(1, float(b.kd.intensity)))
    ctx.set_points(0, b.xy, b.mk)
    ctx.set_schedule(b.T0, b.alpha, 0.0)
    ctx.set_option("handover", 0)
    ctx.set_option("deep_fixed", fixed)
    assert ctx.get_option("deep_carry") == 1                          # (the default)
    ctx.set_option("deep_carry", carry)
    assert ctx.get_option("deep_carry") == carry
    return ctx


def state(ctx):
    xy, m = ctx.get_points(0)
    return xy.tobytes(), m.tobytes(), ctx.step_index(0)


@functools.lru_cache(maxsize=None)
def oracle_state(name):
    """the final configuration of the case's chain on the C oracle, in the form of state()"""
    b = sv.build(name)
    _, _, (xy, mk) = sv.oracle_chain(name)
    return (np.asarray(xy, np.int32).reshape(-1, 2).tobytes(), np.asarray(mk, np.float64).reshape(-1, 3).tobytes(), b.steps)


def stats(ctx):
    st = ctx.deep_stats()
    return {k: st[k] for k in STAT_KEYS}


def deep_run(name, depth, carry):
    b = sv.build(name)
    ctx = make_ctx(b, depth, carry)
    ctx.run(b.steps, b.seed, chain0=b.chain)
    res, st, used = state(ctx), stats(ctx), ctx.get_option("prepass_queues_used")
    ctx.close()
    assert used == 1 and st["committed"] == b.steps and st["rounds"] > 0, (used, st)
    return res, st


def both_ways(name, depth):
    (on, st_on), (off, st_off) = deep_run(name, depth, 1), deep_run(name, depth, 0)
    print(name, depth, "on", st_on, "off", st_off)
    assert on == off, "the option changes the chain"
    assert st_on == st_off, "the option changes the rounds"
    assert on == oracle_state(name), "deep rounds differ from the oracle"
    return st_on


@pytest.mark.parametrize("depth", list(DEPTHS))
def test_small_tile(depth):
    st = both_ways("tile112", depth)
    if depth == "fixed-8":
        assert st["evaluated"] <= 8 * st["rounds"]


@pytest.mark.parametrize("depth", ["adaptive", "fixed-64", "fixed-256"])
def test_packed_tile_with_second_passes(depth):
    """30 overlapping rectangles at T0 = 5: steps that change more than two neighbours (DI_NBOV, a second pass) and steps
    that re-reduce one (DI_RESC) -- reports that conflict at twice the range"""
    st = both_ways("packed", depth)
    assert st["rounds_with_change"] > 0


@pytest.mark.parametrize("depth", ["adaptive", "fixed-64"])
def test_from_the_empty_configuration(depth):
    both_ways("empty", depth)


def test_cell_capacity_stop_in_mid_chain_and_a_continued_call():
    b = sv.build("capacity")
    runs = {}
    for carry in (1, 0):
        ctx = make_ctx(b, "adaptive", carry, cell_capacity=3)
        ctx.set_option("auto_grow", 0)
        with pytest.raises(hip_api.MppError) as e:
            ctx.run(b.steps, b.seed, chain0=b.chain)
        assert e.value.code == -11 and "cell" in str(e.value)
        stopped, st0, at_stop = ctx.step_index(), stats(ctx), state(ctx)
        assert 0 < stopped < b.steps
        pxy, pm = ctx.get_points()
        ctx.set_option("cell_capacity", 32)
        ctx.set_points(0, pxy, pm)                                    # (clears the sticky error; step and temperature stay)
        ctx.run(b.steps - stopped, b.seed, chain0=b.chain)
        runs[carry] = at_stop, st0, state(ctx), stats(ctx)
        ctx.close()
    assert runs[1] == runs[0]
    assert runs[1][2] == oracle_state("capacity")


def test_hot_start_hands_over_in_mid_table():
    """the deep launch starts at the hot start's handover: its first window begins in the middle of the pre-pass table"""
    b = sv.build("hot-start")
    runs = {}
    for carry in (1, 0):
        ctx = make_ctx(b, "adaptive", carry)
        ctx.set_option("handover", 1)
        ctx.set_option("handover_at", 256)                            # (the hot launch ends after its first 48 rounds)
        ctx.run(b.steps, b.seed, chain0=b.chain)
        st = stats(ctx)
        assert ctx.get_option("hot_table_used") == 1 and 0 < st["committed"] < b.steps, st
        runs[carry] = state(ctx), st
        ctx.close()
    assert runs[1] == runs[0]
    assert runs[1][0] == oracle_state("hot-start")


def test_three_calls_on_one_context():
    """every launch starts without a kept report, wherever the one before stopped"""
    b = sv.build("tile112")
    parts = (1000, 700, b.steps - 1700)
    runs = {}
    for carry in (1, 0):
        ctx = make_ctx(b, "adaptive", carry)
        per_call = []
        for n in parts:
            ctx.run(n, b.seed, chain0=b.chain)
            per_call.append((state(ctx), stats(ctx)))
        runs[carry] = per_call
        ctx.close()
    assert runs[1] == runs[0]
    assert runs[1][-1][0] == oracle_state("tile112")


@pytest.mark.parametrize("name", ["tile112", "packed"])
def test_a_traced_chain_never_keeps(name):
    b = sv.build(name)
    o_out, o_props, _ = sv.oracle_chain(name)
    rec = {}
    for carry in (1, 0):
        ctx = make_ctx(b, "adaptive", carry)
        out, props = ctx.run(b.steps, b.seed, chain0=b.chain, trace_tile=0)
        rec[carry] = out.tobytes(), props.tobytes(), state(ctx), stats(ctx)
        ctx.close()
    assert rec[1] == rec[0]
    out = np.frombuffer(rec[1][0], dtype=out.dtype)
    np.testing.assert_array_equal(out["accepted"], o_out["accepted"])
    np.testing.assert_array_equal(out["n_after"], o_out["n_after"])
    assert rec[1][2] == oracle_state(name)
    # ... and the untraced chain of the same call has the traced one's rounds: keeping changes none
    (_, st) = deep_run(name, "adaptive", 1)
    assert st == rec[1][3]


def test_cases_are_the_walked_ones():
    assert set(cc.CASES) == {"tile112", "packed", "empty", "capacity", "hot-start"}
