"""The table form of the hot start (csrc/mpp_hot.hip, option ``hot_table``): the one-wave-per-step launch that starts a
chain of eight waves takes every step's draw from a pre-pass table of its own -- a birth its whole record, any other step
the head of its proposal -- instead of Philox, the kernel search, Box-Muller and the births' CDF search, mark rows and unit
terms.  None of it may change the chain: final configurations equal, byte for byte, the ones with ``hot_table`` 0 (the hot
start draws for itself) and with ``handover`` 0 (deep rounds alone), and the C oracle's where a test says so.  Every run is
untraced: a traced call has no hot start."""
import functools

import numpy as np
import pytest

from test_gpu_chain import setup_case
from test_gpu_prepass_queue import multi_ctx

pytestmark = pytest.mark.gpu

# (hot_table, handover): the table form, the hot start that draws for itself, deep rounds alone
FORMS = {"table": (1, 1), "drawn": (0, 1), "deep": (1, 0)}


def set_form(ctx, form, handover_at=None):
    hot_table, handover = FORMS[form]
    ctx.set_option("hot_table", hot_table)
    ctx.set_option("handover", handover)
    if handover_at is not None:
        ctx.set_option("handover_at", handover_at)


def final(ctx, n_chains=1):
    return [ctx.get_points(i) + (ctx.step_index(i),) for i in range(n_chains)]


def assert_same(a, b):
    assert len(a) == len(b)
    for i, (p, q) in enumerate(zip(a, b)):
        assert p[0].tobytes() == q[0].tobytes() and p[1].tobytes() == q[1].tobytes() and p[2] == q[2], f"chain {i}"


def single(form, n_steps, seed, handover_at=None, setup_name="legacy", tile=128, n_obj=40, T0=1.0, alpha=0.9985, calls=1,
           prepare=None, cap=512):
    """one chain of eight waves, `calls` calls of n_steps; returns (finals, ctx, hot_table_used and deep commits per call)"""
    _, o, ctx = setup_case(tile, n_obj, setup_name, spec=8, deep=128, cap=cap)
    if prepare is not None:
        prepare(ctx)
    set_form(ctx, form, handover_at)
    ctx.set_schedule(T0, alpha, 0.0)
    used = []
    for _ in range(calls):
        ctx.run(n_steps, seed)
        used.append((ctx.get_option("hot_table_used"), ctx.deep_stats()["committed"]))
    assert ctx.step_index() == calls * n_steps
    return final(ctx), ctx, used, o


@pytest.mark.parametrize("setup_name,T0,alpha", [("legacy", 1.0, 0.998), ("no-calibration", 2.0, 0.997)])
def test_whole_chain_in_the_hot_kernel(setup_name, T0, alpha):
    """handover_at 2048 (8 of 8 steps per round, smoothed) is never reached: all 6 001 steps -- the last round is partial --
    and all eight kernel types run in the table kernel; against the oracle and the two other forms"""
    n_steps, seed = 6001, 1234
    tab, ctx, used, o = single("table", n_steps, seed, 2048, setup_name, T0=T0, alpha=alpha)
    assert used == [(1, 0)]                                    # the table was read, no deep round committed a step
    o.set_temperature(T0, alpha, 0.0)
    o.run(n_steps, seed, chain=0)
    oxy, om = o.get_points()
    np.testing.assert_array_equal(tab[0][0], oxy)
    np.testing.assert_allclose(tab[0][1], om, rtol=1e-9, atol=1e-9)
    drawn, _, used_d, _ = single("drawn", n_steps, seed, 2048, setup_name, T0=T0, alpha=alpha)
    assert used_d == [(0, 0)]
    assert_same(tab, drawn)
    assert_same(tab, single("deep", n_steps, seed, None, setup_name, T0=T0, alpha=alpha)[0])


def test_handover_at_the_first_chance():
    """handover_at 256: the hot launch ends after its 48 rounds, at a step that is no multiple of the pre-pass block, and
    the deep launch continues from there with a table of its own"""
    n_steps, seed = 6001, 77
    tab, ctx, used, _ = single("table", n_steps, seed, 256)
    hot_used, deep_committed = used[0]
    assert hot_used == 1 and 0 < deep_committed < n_steps
    assert (n_steps - deep_committed) % 256 != 0
    assert ctx.get_option("prepass_queues_used") == 1
    assert_same(tab, single("drawn", n_steps, seed, 256)[0])
    assert_same(tab, single("deep", n_steps, seed)[0])


def test_default_handover():
    """the 256-px / 80-object / 30 000-step chain of test_hot_start_hands_the_chain_over_without_changing_it"""
    n_steps, seed = 30000, 11
    kw = dict(tile=256, n_obj=80, alpha=0.999)
    tab, ctx, used, _ = single("table", n_steps, seed, **kw)
    assert used[0][0] == 1 and 0 < used[0][1] < n_steps
    assert ctx.get_option("prepass_queues_used") == 1
    assert_same(tab, single("drawn", n_steps, seed, **kw)[0])
    assert_same(tab, single("deep", n_steps, seed, **kw)[0])


def test_three_calls():
    """the second and third call build their tables from a step other than 0 (hot again: handover_at 2048)"""
    n_steps, seed = 5000, 31
    tab, _, used, _ = single("table", n_steps, seed, 2048, calls=3)
    assert used == [(1, 0)] * 3
    assert_same(tab, single("drawn", n_steps, seed, 2048, calls=3)[0])
    assert_same(tab, single("deep", n_steps, seed, calls=3)[0])


def test_from_the_empty_configuration():
    """steps with a target while n == 0: their queue entry is read, the tail leaves them without a target"""
    def empty(ctx):
        ctx.set_points(0, np.zeros((0, 2), np.int32), np.zeros((0, 3), np.float64))
    n_steps, seed = 5000, 3
    tab, _, used, _ = single("table", n_steps, seed, 2048, prepare=empty)
    assert used == [(1, 0)] and len(tab[0][0]) > 0
    assert_same(tab, single("drawn", n_steps, seed, 2048, prepare=empty)[0])
    assert_same(tab, single("deep", n_steps, seed, prepare=empty)[0])


@pytest.mark.parametrize("at", [2048, 256])
def test_capacity_stop_and_relaunch_in_mid_table(at):
    """the point capacity just holds the initial configuration: the first net birth stops the chain, auto_grow doubles the
    capacity and the launch is issued again; it reads the call's table from the step the chain stopped at.  handover_at
    2048: the stops fall into the hot start; 256: the deep launch takes over after 48 rounds and is stopped and re-launched"""
    n_steps, seed, T0, alpha = 5000, 9, 5.0, 0.9995
    _, _, probe = setup_case(128, 40, "legacy", spec=8, deep=128)
    n0 = len(probe.get_points()[0])
    probe.close()
    tab, ctx, used, _ = single("table", n_steps, seed, at, T0=T0, alpha=alpha, cap=n0)
    assert used[0][0] == 1 and (used[0][1] == 0) == (at == 2048)
    assert ctx.get_option("grow_events") >= 1 and ctx.get_option("point_capacity") > n0
    big, ctx_b, _, _ = single("table", n_steps, seed, at, T0=T0, alpha=alpha)
    assert ctx_b.get_option("grow_events") == 0
    assert_same(tab, big)
    drawn, ctx_d, _, _ = single("drawn", n_steps, seed, at, T0=T0, alpha=alpha, cap=n0)
    assert ctx_d.get_option("grow_events") == ctx.get_option("grow_events")
    assert_same(tab, drawn)
    assert_same(tab, single("deep", n_steps, seed, T0=T0, alpha=alpha)[0])


def test_packed_tile():
    """the packed tile of tests/test_gpu_deep_live_state.py (30 strongly overlapping rectangles at T0 = 5), where accepted steps
    change many neighbours at once.  (An apply round -- a step that changes more neighbours than the stash of 32 holds is
    evaluated again, alone, from the same entry -- cannot be asserted: the kernel counts none.)"""
    def packed(ctx):
        rng = np.random.default_rng(3)
        xy = rng.integers(24, 72, (30, 2)).astype(np.int32)
        marks = np.stack([rng.uniform(20.0, 30.0, 30), rng.uniform(0.3, 0.6, 30), rng.uniform(0.0, np.pi, 30)], axis=1)
        ctx.set_points(0, xy, marks)
    n_steps, seed = 4100, 5
    kw = dict(tile=96, n_obj=30, T0=5.0, alpha=0.9995, prepare=packed, cap=256)
    tab, _, used, _ = single("table", n_steps, seed, 2048, **kw)
    assert used == [(1, 0)]
    assert_same(tab, single("drawn", n_steps, seed, 2048, **kw)[0])
    assert_same(tab, single("deep", n_steps, seed, **kw)[0])


def many(form, n_chains, big=False):
    """chains with Philox keys of their own (the way restarts set them) on 8 tiles' maps, two calls: they cool down at
    different steps, so the deep launch that follows starts every chain at a step of its own"""
    ctx = multi_ctx("queues", n_chains, big)
    set_form(ctx, form)
    used = []
    for n_steps in (4500, 4200):
        ctx.run(n_steps, 0)
        used.append(ctx.get_option("hot_table_used"))
    res = final(ctx, n_chains)
    hbm = ctx.get_option("hbm_chains")
    ctx.close()
    assert all(r[2] == 8700 for r in res)
    return res, used, hbm


@functools.lru_cache(maxsize=None)
def many_deep(n_chains, big=False):
    return many("deep", n_chains, big)


@pytest.mark.parametrize("n_chains", [1, 16, 64])
def test_launches_of_several_keyed_chains(n_chains):
    tab, used, _ = many("table", n_chains)
    assert used == [1, 1]
    assert_same(tab, many("drawn", n_chains)[0])
    assert_same(tab, many_deep(n_chains)[0])


def test_too_many_chains_for_a_hot_start():
    """65 chains are more than handover_tiles: no hot start, no table of its own"""
    tab, used, _ = many("table", 65)
    assert used == [0, 0]
    assert_same(tab, many_deep(65)[0])


def test_routed_launch():
    """one chain in device memory (2 100 points) next to four LDS chains that start hot.  (The first call finds the context's
    capacities too large for an LDS launch and decides against a hot start before it decouples them; the second starts hot.)"""
    tab, used, hbm = many("table", 5, True)
    assert used == [0, 1] and hbm == 1
    assert_same(tab, many("drawn", 5, True)[0])
    assert_same(tab, many_deep(5, True)[0])


def test_over_budget():
    """prepass_mb 1: the queues of 200 000 steps do not fit, the hot start draws for itself"""
    n_steps, seed = 200000, 3

    def one_mb(ctx):
        ctx.set_option("prepass_mb", 1)
    tab, ctx, used, _ = single("table", n_steps, seed, prepare=one_mb)
    assert used[0][0] == 0 and ctx.get_option("prepass_queues_used") == 0
    assert_same(tab, single("deep", n_steps, seed)[0])
    assert_same(tab, single("drawn", n_steps, seed, prepare=one_mb)[0])
    with pytest.raises(Exception):
        ctx.set_option("hot_table", 2)
