"""The proposal kernels at kernel parameters and mark mappings other than the defaults (tests/kernel_param_cases.py), against
the CPU oracle, which is generic in all of them: translation windows from 1 x 1 to 31 x 31 pixels (the generic loop of
window_draw_lane, up to 31 lanes of window_draw, k_boxsum at max_delta != 8), bin edges that are no linspace (the binary
search of value_to_class_tab, and every copy of the edge table), ranges that do not start at 0, other cyclic flags and
sigmas, tiles thinner than the window, longer than 512 pixels and higher than 1 024, and a context re-configured while
its chain runs.  tests/test_kernel_param_cases_host.py shows on the CPU that each case reaches what it is there for."""
import dataclasses

import numpy as np
import pytest

import kernel_param_cases as kc
import oracle
from helpers import lockstep_vs_oracle, worst_differences
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings
from test_gpu_layout_shapes import SHAPES
from test_gpu_prepass_queue import MODES, set_mode

pytestmark = pytest.mark.gpu
ONE_WAVE = (1, 0, 0, 1)                 # (spec_waves, spec_lanes, deep, chain_state), as in SHAPES
CAP = 512                               # points per chain: no case passes 200 (the oracle's walk), auto_grow stays on


def make_ctx(b, shape=ONE_WAVE, maps=None, kd=None, points=True):
    spec, lanes, deep, state = shape
    ctx = hip_api.MppContext(0, point_capacity=CAP, spec_waves=spec, spec_lanes=lanes, deep=deep, chain_state=state)
    ctx.set_maps(b.det, b.marks)
    ctx.set_model(b.model, maps or b.maps)
    ctx.set_kernels(kd or b.kd)
    if points:
        ctx.set_points(0, b.xy, b.mk)
    ctx.set_schedule(b.case.T0, b.case.alpha, 0.0)
    return ctx


def assert_final_equals_oracle(ctx, o):
    gxy, gm = ctx.get_points()
    oxy, om = o.get_points()
    np.testing.assert_array_equal(gxy, oxy)
    np.testing.assert_allclose(gm, om, rtol=1e-9, atol=1e-9)
    assert ctx.total_energy() == pytest.approx(o.total_energy(), rel=1e-10, abs=1e-9)


# ---- a. lockstep against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.CASES, ids=str)
def test_chain_in_lockstep_with_the_oracle(case):
    """every step of the case: proposals (integers exactly, reals to 1e-9), fwd / bwd to 1e-9 relative -- the box-sum
    normaliser of the translation window, which the oracle sums pixel by pixel and the device takes from row prefixes up to
    1 040 entries long, reaches the test through them --, dE to DE_TOL, decisions and populations; then the configuration"""
    b = kc.build(case)
    o, ctx = kc.make_oracle(b), make_ctx(b)
    ties = lockstep_vs_oracle(ctx, o, case.steps, case.seed, case.chain, case.alpha)
    assert ties == 0                                      # (the schedules never freeze)
    assert ctx.step_index() == case.steps
    assert_final_equals_oracle(ctx, o)
    # for the report (pytest -s): the worst differences behind those bars, from a second, traced run of the same chain
    worst = worst_differences(make_ctx(b), kc.make_oracle(b), case.steps, case.seed, case.chain)
    print(f"\n{case.name}: worst differences device / oracle: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


# ---- b. one chain in every launch shape --------------------------------------------------------------------------------
def final_bytes(b, shape, steps=None, prepare=None):
    ctx = make_ctx(b, shape)
    if prepare:
        prepare(ctx)
    ctx.run(steps or b.case.steps, b.case.seed, chain0=b.case.chain)
    gxy, gm = ctx.get_points()
    return (gxy.tobytes(), gm.tobytes()), ctx


def refused(case, shape):
    """the split / merge kernels are built for 1 and 8 waves with no lane mode"""
    spec, lanes, deep, state = shape
    return case.split_merge and not (lanes == 0 and spec in (1, 8))


@pytest.mark.parametrize("case", kc.CASES, ids=str)
def test_every_launch_shape_runs_the_same_chain(case):
    b = kc.build(case)
    want, ctx = final_bytes(b, ONE_WAVE)
    w = kc.walk(case)                                      # the oracle's own chain (no lockstep): the same configuration
    gxy, gm = ctx.get_points()
    np.testing.assert_array_equal(gxy, w.final[0])
    np.testing.assert_allclose(gm, w.final[1], rtol=1e-9, atol=1e-9)
    lost = 0
    for shape in SHAPES:
        if refused(case, shape):
            with pytest.raises(hip_api.MppError):
                final_bytes(b, shape)
            lost += 1
            continue
        got, ctx = final_bytes(b, shape)
        assert got == want, (case.name, shape)
        assert ctx.get_option("hbm_chains") == (1 if shape[3] == 2 else 0)
    assert lost <= 1                                       # (lane mode, for the split / merge case)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_prepass_modes_run_the_same_chain(mode):
    """deep rounds fed by the pre-pass (none, births table, per-type queues): its copy of the warped edge table (s_edges) and
    its window draws at max_delta 9, under a mixture with three kernels of probability 0"""
    b = kc.build(kc.BY_NAME["mix48x80-warped-md9"])
    want, _ = final_bytes(b, ONE_WAVE)

    def prepare(ctx):
        ctx.set_option("handover", 0)
        set_mode(ctx, mode)
    got, ctx = final_bytes(b, (8, 0, 128, 1), prepare=prepare)
    assert got == want
    assert ctx.deep_stats()["committed"] == b.case.steps
    assert ctx.get_option("prepass_used") == MODES[mode][0]
    assert ctx.get_option("prepass_queues_used") == MODES[mode][1]


def test_hot_start_runs_the_same_chain():
    """the hot start (one wave per step, its draws from the pre-pass table) that hands over to deep rounds, on the long tile
    under the warped mapping with a 31 x 31 window; 5 000 steps: a call of fewer than 4 096 does not start hot.  This
    schedule stays above T = 0.41, so handover_at 256 (the first chance, as in test_handover_at_the_first_chance) makes the
    hand-over certain: both the table kernel and the deep rounds after it run part of the chain, which the test asserts"""
    b = kc.build(kc.BY_NAME["long24x1040-warped-md15"])
    steps = 5000
    want, _ = final_bytes(b, ONE_WAVE, steps=steps)

    def prepare(ctx):
        ctx.set_option("handover", 1)
        ctx.set_option("handover_at", 256)
    got, ctx = final_bytes(b, (8, 0, 128, 1), steps=steps, prepare=prepare)
    assert got == want
    assert ctx.step_index() == steps
    assert ctx.get_option("hot_table_used") == 1           # the hot start ran, and from the table
    assert 0 < ctx.deep_stats()["committed"] < steps       # ... and handed over to deep rounds
    assert ctx.get_option("prepass_queues_used") == 1


# ---- c. naive initialisation and from-scratch energies under other mappings -----------------------------------------------
@pytest.mark.parametrize("name", ["split40x56-offset-md3", "mix48x80-warped-md9"])
def test_naive_init_and_from_scratch_energies(name):
    b = kc.build(kc.BY_NAME[name])
    H, W = b.case.shape
    o = oracle.Oracle(b.case.shape, b.det, b.marks, b.model, b.kd)
    ctx = make_ctx(b, points=False)
    thr = b.setup.detection_threshold
    ctx.naive_init(thr, 6.0)
    oxy, om = o.naive_detection(thr, 6.0)
    gxy, gm = ctx.get_points()
    assert len(oxy) >= 5
    np.testing.assert_array_equal(gxy, oxy)
    np.testing.assert_array_equal(gm, om)                   # edge values of the custom table, bit for bit
    edges = np.stack([m.feature_mapping for m in b.maps])
    assert all(np.isin(gm[:, k], edges[k]).all() for k in range(3))
    # a configuration with marks anywhere in the ranges, on edges of the table and on the range ends
    rng = np.random.default_rng(5)
    n = 60
    lo, hi = b.kd.vmin, b.kd.vmax
    xy = np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], axis=1).astype(np.int32)
    mk = lo + (hi - lo) * rng.random((n, 3))
    for k in range(3):
        mk[:12, k] = edges[k][rng.integers(0, 32, 12)]
    mk[12, :], mk[13, :2] = lo, hi[:2]
    ctx.set_points(0, xy, mk); o.set_points(xy, mk)
    removals = [[int(i)] for i in rng.integers(0, n, 8)] + [sorted(set(int(i) for i in rng.integers(0, n, 3))) for _ in range(8)] + [[]] * 4
    add_xy, add_mk = [], []
    for r in removals:
        m = int(rng.integers(0, 3)) if r else 2
        base = xy[int(rng.integers(0, n))]
        add_xy.append(np.clip(base + rng.integers(-6, 7, size=(m, 2)), 0, [H - 1, W - 1]).astype(np.int32))
        add_mk.append((lo + (hi - lo) * rng.random((m, 3))).reshape(m, 3))
    assert len(removals) == 20
    pap, want = o.papangelou(), [o.delta(removal_slots=r, add_xy=a, add_marks=m) for r, a, m in zip(removals, add_xy, add_mk)]
    e0 = o.total_energy()
    for grid in (0, 1):
        ctx.set_option("scratch_grid_min_points", grid)
        assert ctx.total_energy() == pytest.approx(e0, rel=1e-9, abs=1e-7)
        np.testing.assert_allclose(ctx.papangelou(0), pap, rtol=1e-9, atol=1e-8)
        got = ctx.delta_batch(0, removals, add_xy, add_mk)
        for k in range(20):
            assert got[k] == pytest.approx(want[k], rel=1e-9, abs=1e-8), (grid, k)


# ---- d. a live context re-configured -----------------------------------------------------------------------------------
def reconfigure_sides():
    """A: the default mappings and kernel parameters (max_delta 8); B: the warped mappings, max_delta 12, other sigmas.  Same
    maps, model and start (the 48 x 80 tile), so that only what set_model / set_kernels carry changes."""
    base = kc.BY_NAME["wide-default-md12"]
    a = kc.build(base, max_delta=8, sigma_trans=2.0, sigma_transform=0.1)
    mb = kc.make_mappings("warped")
    kb = dataclasses.replace(kernels.make_kernels(mb, base.intensity), max_delta=12, sigma_trans=3.5, sigma_transform=0.25)
    return a, {"A": (a.maps, a.kd), "B": (mb, kb)}


@pytest.mark.parametrize("remap", [0, 1])
@pytest.mark.parametrize("spec", [1, 8])
@pytest.mark.parametrize("order", ["AB", "BA"])
def test_reconfigured_context_follows_the_new_parameters(order, spec, remap):
    """500 steps under one side, then set_model / set_kernels / set_schedule on the SAME context and 1 500 steps under the other:
    the box sums (box_dirty), uniform_bins, inv_step, the edge tables and the remap tables must all be the new side's.  Both
    orders, so that a stale table cannot pass by being the larger one.  (Points of side A may lie outside side B's ranges:
    a value below the first edge is class 0 on both sides.)"""
    b, sides = reconfigure_sides()
    seed, chain, alpha = 321, 2, 0.9995
    (m1, k1), (m2, k2) = sides[order[0]], sides[order[1]]
    ctx = make_ctx(b, (spec, 0, 0, 1), maps=m1, kd=k1)
    ctx.set_option("remap_table", remap)
    ctx.set_schedule(5.0, alpha, 0.0)
    o = oracle.Oracle(b.case.shape, b.det, b.marks, b.model, k1)
    o.set_points(b.xy, b.mk); o.set_temperature(5.0, alpha, 0.0)
    assert lockstep_vs_oracle(ctx, o, 500, seed, chain, alpha) == 0
    ctx.set_model(b.model, m2)
    ctx.set_kernels(k2)
    ctx.set_schedule(3.0, alpha, 0.0)                       # (a new schedule starts the step count, the Philox counter, at 0)
    o2 = oracle.Oracle(b.case.shape, b.det, b.marks, b.model, k2)
    o2.restore((ctx.get_points(), ctx.step_index(), 3.0), alpha)
    assert o2.step_index() == ctx.step_index() == 0
    assert lockstep_vs_oracle(ctx, o2, 1500, seed + 1, chain, alpha) == 0
    assert ctx.get_option("remap_table") == remap and ctx.step_index() == 1500
    assert_final_equals_oracle(ctx, o2)


# ---- e. refusals ---------------------------------------------------------------------------------------------------------
def test_refused_parameters_leave_the_context_usable():
    base = kc.BY_NAME["wide-default-md12"]
    b = kc.build(base, max_delta=8, sigma_trans=2.0, sigma_transform=0.1)
    fresh, _ = final_bytes(b, ONE_WAVE, steps=1500)
    ctx = make_ctx(b)
    for md in (16, -1):
        with pytest.raises(hip_api.MppError, match="max_delta"):
            ctx.set_kernels(dataclasses.replace(b.kd, max_delta=md))
    flat = mappings.default_mappings()
    flat[1].feature_mapping = flat[1].feature_mapping.copy()
    flat[1].feature_mapping[7] = flat[1].feature_mapping[6]
    with pytest.raises(hip_api.MppError, match="edges"):
        ctx.set_model(b.model, flat)
    ctx.run(1500, base.seed, chain0=base.chain)
    gxy, gm = ctx.get_points()
    assert (gxy.tobytes(), gm.tobytes()) == fresh
