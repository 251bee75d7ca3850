"""The hot start's rounds go on past an accepted birth or death (csrc/mpp_chain_body.inc, MPP_HOT_PAST in ``mpp_hot_kernel``;
option ``hot_past_births``, default 1): the commit wave edits n and order[] itself, draws every later record's target again,
drops the records within reach of the born / killed rectangle and takes the accept test of the others again with the new n.
None of it may change the chain.  Every case runs the same call four ways -- the new rule, ``hot_past_births`` 0 (the round ends
with the birth / death, as before), ``hot_table`` 0 (the hot start of mpp_chain_kernel, which this does not touch) and
``handover`` 0 (deep rounds alone) -- and compares final configuration, step index and temperature byte for byte; one case also
against the C oracle.  The cases are the smallest that reach the new paths; where a case is about what a round holds, the
host walk (tests/hot_commit_walk.py) counts it first on the oracle's trace of the same chain."""
import re

import numpy as np
import pytest

import hot_commit_walk as hw
from test_gpu_chain import setup_case
from test_gpu_prepass_queue import multi_ctx

pytestmark = pytest.mark.gpu

# (hot_table, handover, hot_past_births)
FORMS = {"past": (1, 1, 1), "ends": (1, 1, 0), "drawn": (0, 1, 1), "deep": (1, 0, 1)}


def set_form(ctx, form, handover_at=None):
    hot_table, handover, past = FORMS[form]
    ctx.set_option("hot_table", hot_table)
    ctx.set_option("handover", handover)
    ctx.set_option("hot_past_births", past)
    if handover_at is not None:
        ctx.set_option("handover_at", handover_at)


def final(ctx, n_chains, seed):
    """per chain (pixels, marks, step index); then the temperature of chain 0 and of the last chain: a traced call of one
    step reports the temperature its step ran at"""
    res = [ctx.get_points(i) + (ctx.step_index(i),) for i in range(n_chains)]
    temps = [float(ctx.run(1, seed, trace_tile=i)[0]["T"][0]) for i in sorted({0, n_chains - 1})]
    return res, temps


def assert_same(a, b):
    (ra, ta), (rb, tb) = a, b
    assert len(ra) == len(rb)
    for i, (p, q) in enumerate(zip(ra, rb)):
        assert p[0].tobytes() == q[0].tobytes() and p[1].tobytes() == q[1].tobytes() and p[2] == q[2], f"chain {i}"
    assert np.array(ta).tobytes() == np.array(tb).tobytes()


def single(form, n_steps, seed, handover_at=2048, tile=128, n_obj=40, T0=1.0, alpha=0.9995, prepare=None, cap=512):
    """one chain of eight waves (a call of 4 096 steps or more starts hot); handover_at 2048 is never reached: the whole call
    runs in the hot kernel"""
    _, o, ctx = setup_case(tile, n_obj, "legacy", spec=8, deep=128, cap=cap)
    if prepare is not None:
        prepare(ctx, o)
    set_form(ctx, form, handover_at)
    ctx.set_schedule(T0, alpha, 0.0)
    ctx.run(n_steps, seed)
    assert ctx.step_index() == n_steps
    info = dict(hot=ctx.get_option("hot_table_used"), deep_committed=ctx.deep_stats()["committed"],
                grow=ctx.get_option("grow_events"), cap=ctx.get_option("point_capacity"), cell=ctx.get_option("cell_capacity"))
    res = final(ctx, 1, seed)
    ctx.close()
    return res, info, o


def four_ways(n_steps, seed, **kw):
    past, info, o = single("past", n_steps, seed, **kw)
    assert info["hot"] == 1
    for form in ("ends", "drawn", "deep"):
        other, info_o, _ = single(form, n_steps, seed, **kw)
        assert_same(past, other)
        if form != "deep":
            assert info_o["grow"] == info["grow"]
    return past, info, o


def oracle_walk(o, n_steps, seed, T0, alpha):
    """the walk of the new rule over the oracle's trace of the chain `o` is about to run, with the steps' own target words"""
    xy0 = o.get_points()[0]
    o.set_temperature(T0, alpha, 0.0)
    out, props = o.run(n_steps, seed, chain=0, trace=True)
    return hw.walk(props, out, xy0, hw.philox_target_words(n_steps, seed), True), out


def empty(ctx, o):
    ctx.set_points(0, np.zeros((0, 2), np.int32), np.zeros((0, 3), np.float64))
    o.set_points(np.zeros((0, 2), np.int32), np.zeros((0, 3), np.float64))


def test_from_the_empty_configuration_against_the_oracle():
    """a 64 x 64 tile at T0 = 5 from no point at all: n passes 0 and 1 (steps drawn without a target lose their trust with the
    first birth), and with so few points every birth and death moves most target indices"""
    n_steps, seed, T0, alpha = 4400, 3, 5.0, 0.9995
    kw = dict(tile=64, n_obj=6, T0=T0, alpha=alpha, prepare=empty)
    past, info, o = four_ways(n_steps, seed, **kw)
    assert info["deep_committed"] == 0
    r, out = oracle_walk(o, n_steps, seed, T0, alpha)        # (o: emptied by `prepare`, at step 0)
    assert min(r["n_start"]) == 0 and 1 in r["n_start"] and max(r["bd_per_round"]) >= 2
    oxy, om = o.get_points()
    (gxy, gm, gstep), = past[0]
    assert len(gxy) > 0 and gstep == n_steps
    np.testing.assert_array_equal(gxy, oxy)
    np.testing.assert_allclose(gm, om, rtol=1e-9, atol=1e-9)
    assert int(out["n_after"][-1]) == len(gxy)


def one_cell(ctx, o):
    """six rectangles inside one 32-px cell of a 64 x 64 tile"""
    rng = np.random.default_rng(7)
    xy = rng.integers(34, 62, (6, 2)).astype(np.int32)
    marks = np.stack([rng.uniform(8.0, 14.0, 6), rng.uniform(0.3, 0.6, 6), rng.uniform(0.0, np.pi, 6)], axis=1)
    ctx.set_points(0, xy, marks)
    o.set_points(xy, marks)


def test_a_handful_of_points_in_one_cell():
    """births and deaths within reach of the later records' points: those records must be dropped, not committed"""
    four_ways(4400, 5, tile=64, n_obj=6, T0=5.0, prepare=one_cell)


def test_rounds_with_two_and_three_births_and_deaths():
    n_steps, seed, T0, alpha = 4400, 21, 5.0, 0.9995
    kw = dict(tile=256, n_obj=80, T0=T0, alpha=alpha)
    _, o, probe = setup_case(256, 80, "legacy", spec=8, deep=128)
    probe.close()
    r, _ = oracle_walk(o, n_steps, seed, T0, alpha)
    bd = np.array(r["bd_per_round"])
    assert int((bd == 2).sum()) >= 10 and int((bd >= 3).sum()) >= 10
    four_ways(n_steps, seed, **kw)


def test_point_capacity_one_above_the_start():
    """the walk finds a round that starts at capacity and commits a death, then a birth (which fits the RUNNING population
    only), before the first birth that does not fit: there the chain stops, auto_grow doubles the capacity and the launch is
    issued again"""
    n_steps, seed, T0, alpha = 4400, 34, 2.0, 0.9995
    _, o, probe = setup_case(128, 40, "legacy", spec=8, deep=128)
    n0 = len(probe.get_points()[0])
    probe.close()
    cap = n0 + 1
    r, _ = oracle_walk(o, n_steps, seed, T0, alpha)
    hit = stop = None
    for i, (kinds, n) in enumerate(zip(r["kinds"], r["n_start"])):
        at_cap = n == cap
        for ch in kinds:
            if ch == "b" and n >= cap:
                stop = i
                break
            n += 1 if ch == "b" else -1
        if stop is not None:
            break
        if at_cap and re.search("d.*b", kinds):
            hit = i
    assert hit is not None and stop is not None and hit < stop
    past, info, _ = four_ways(n_steps, seed, tile=128, n_obj=40, T0=T0, alpha=alpha, cap=cap)
    assert info["grow"] >= 1 and info["cap"] > cap
    big, info_b, _ = single("past", n_steps, seed, tile=128, n_obj=40, T0=T0, alpha=alpha)
    assert info_b["grow"] == 0
    assert_same(past, big)


def test_cell_capacity_that_a_birth_fills():
    """six points in one cell that holds six: after a death a birth fills the cell again, and the next point that wants in
    (the oracle's chain has up to seven there) stops the chain before its step; auto_grow doubles the cells"""
    def tight(ctx, o):
        one_cell(ctx, o)
        ctx.set_option("cell_capacity", 6)
    past, info, _ = four_ways(4400, 5, tile=64, n_obj=6, T0=5.0, prepare=tight)
    assert info["grow"] >= 1 and info["cell"] > 6
    assert_same(past, single("past", 4400, 5, tile=64, n_obj=6, T0=5.0, prepare=one_cell)[0])


def many(form, n_chains):
    """keyed chains on 8 tiles' maps: they hand over at different steps"""
    ctx = multi_ctx("queues", n_chains)
    set_form(ctx, form)
    ctx.run(5000, 0)
    used = ctx.get_option("hot_table_used")
    res = final(ctx, n_chains, 0)
    ctx.close()
    assert all(r[2] == 5000 for r in res[0])
    return res, used


@pytest.mark.parametrize("n_chains", [1, 16, 64])
def test_keyed_chains_that_hand_over_at_different_steps(n_chains):
    past, used = many("past", n_chains)
    assert used == 1
    for form in ("ends", "drawn", "deep"):
        assert_same(past, many(form, n_chains)[0])


def test_handover_at_the_first_chance():
    """handover_at 256: the hot launch ends after its 48 rounds, the deep launch continues"""
    n_steps, seed = 5000, 77
    past, info, _ = four_ways(n_steps, seed, handover_at=256, T0=1.0, alpha=0.9985)
    assert 0 < info["deep_committed"] < n_steps
