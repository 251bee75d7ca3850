"""The commit decision of a deep round (csrc/mpp_deep.hip, phase C; the rule and the pair test: csrc/mpp_commit.hpp) is a
function of the round's reports that needs no order: the changing steps are dealt to the waves, each wave keeps the first
report its steps conflict with, the minimum over the waves ends the round.  None of it may change the chain -- every case
equals the one-wave kernel (``spec`` 1, ``deep`` 0) byte for byte -- nor which steps a round commits: the counts of rounds
and of evaluated steps are those of the serial decision (PARENT_COUNTS, measured on the build of the commit before the
split; profiles/commit_split.md lists them)."""
import functools

import numpy as np
import pytest

import oracle
from helpers import model_for
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings, synth
from test_gpu_capacity import make as capacity_ctx
from test_gpu_deep_live_state import PACKED_SEED, PACKED_STEPS, assert_same_chain, finish, packed_ctx, packed_reference

pytestmark = pytest.mark.gpu

# (fixed depth, traced) -> (rounds, evaluated) of the packed tile's 4 000 steps with the serial commit loop
PARENT_COUNTS = {(8, True): (1984, 15863), (8, False): (1984, 15863), (64, True): (1982, 125942), (64, False): (1982, 125942),
                 (128, True): (1982, 249859), (128, False): (1982, 249859), (256, True): (1982, 485378), (256, False): (1982, 485378)}


def fixed_ctx(fixed):
    ctx = packed_ctx(8, 256 if fixed > 128 else 128)
    ctx.set_option("deep_fixed", fixed)
    return ctx


@pytest.mark.parametrize("traced", [True, False])
@pytest.mark.parametrize("fixed", [8, 64, 128, 256])
def test_packed_tile_fixed_depths(fixed, traced):
    """a window of 256 steps at T0 = 5 holds far more than 8 changing steps: the waves take several each"""
    ctx = fixed_ctx(fixed)
    got = finish(ctx, PACKED_STEPS, PACKED_SEED, traced)
    assert ctx.get_option("prepass_queues_used") == 1
    st = ctx.deep_stats()
    assert st["committed"] == PACKED_STEPS
    assert_same_chain(packed_reference(), got, traced)
    assert (st["rounds"], st["evaluated"]) == PARENT_COUNTS[(fixed, traced)], st


@pytest.mark.parametrize("spec,deep", [(1, 64), (2, 128), (4, 256)])
def test_adaptive_depth_sorted_rounds(spec, deep):
    """the instantiations that sort their steps (no queues), one, two and four waves, the depth following the commits"""
    ctx = packed_ctx(spec, deep)
    got = finish(ctx, PACKED_STEPS, PACKED_SEED, True)
    st = ctx.deep_stats()
    assert st["committed"] == PACKED_STEPS and st["rounds"] > 0, st
    assert_same_chain(packed_reference(), got, True)


# ---- the two capacity stops: the chain ends in the state before the step that does not fit
def limited_ctx(spec, deep, auto_grow, **caps):
    """the packed tile in a context with its own capacities"""
    t = synth.make_tile(96, 30, tile_id=0, noise=0.1)
    setup, _, model = model_for("legacy")
    maps = mappings.default_mappings()
    o = oracle.Oracle(t.shape, t.det, t.marks, model, kernels.make_kernels(maps, 1.0))
    n0 = len(o.naive_detection(setup.detection_threshold, 6.0)[0])
    ctx = hip_api.MppContext(0, spec_waves=spec, deep=deep, **caps)
    ctx.set_maps(t.det, t.marks)
    ctx.set_model(model, maps)
    ctx.set_kernels(kernels.make_kernels(maps, max(1, n0)))
    rng = np.random.default_rng(3)
    xy = rng.integers(24, 72, (30, 2)).astype(np.int32)
    marks = np.stack([rng.uniform(20.0, 30.0, 30), rng.uniform(0.3, 0.6, 30), rng.uniform(0.0, np.pi, 30)], axis=1)
    ctx.set_points(0, xy, marks)
    ctx.set_option("handover", 0)
    ctx.set_option("auto_grow", auto_grow)
    ctx.set_schedule(5.0, 0.9995, 0.0)
    return ctx


def stopped_run(ctx, code):
    with pytest.raises(hip_api.MppError) as e:
        ctx.run(PACKED_STEPS, PACKED_SEED)
    assert e.value.code == code, e.value
    xy, m = ctx.get_points()
    return ctx.step_index(), xy.tobytes(), m.tobytes()


@functools.lru_cache(maxsize=None)
def cell_stop_reference():
    return stopped_run(limited_ctx(1, 0, 0, point_capacity=256, cell_capacity=3), -11)


@pytest.mark.parametrize("deep", [128, 256])
def test_cell_limit_stops_at_the_same_step(deep):
    ref = cell_stop_reference()
    got = stopped_run(limited_ctx(8, deep, 0, point_capacity=256, cell_capacity=3), -11)
    assert got == ref              # (30 rectangles within 48 x 48 px: the tile's first cell list is already too long, step 0)


def test_cell_limit_with_auto_grow_runs_to_the_same_end():
    ctx = limited_ctx(8, 128, 1, point_capacity=256, cell_capacity=3)
    got = finish(ctx, PACKED_STEPS, PACKED_SEED, False)
    assert ctx.get_option("grow_events") >= 1
    assert_same_chain(packed_reference(), got, False)


# ... and in mid-chain: the hot tile of tests/test_gpu_capacity.py, whose uniform births pile up until a cell is full
def crowded_stop(spec, deep):
    tile = synth.make_tile(96, 14, tile_id=71, noise=0.1)
    setup, _, model = model_for("legacy")
    maps = mappings.default_mappings()
    o = oracle.Oracle(tile.shape, tile.det, tile.marks, model, kernels.make_kernels(maps, 1.0))
    xy, mk = o.naive_detection(setup.detection_threshold, 6.0)
    ctx = capacity_ctx(tile, model, kernels.make_kernels(maps, 150.0), xy, mk, 5.0, 0.9995, spec, point_capacity=1024, cell_capacity=3)
    ctx.set_option("deep", deep)
    ctx.set_option("handover", 0)
    ctx.set_option("auto_grow", 0)
    with pytest.raises(hip_api.MppError) as e:
        ctx.run(6000, 31, chain0=3)
    assert e.value.code == -11, e.value
    pxy, pm = ctx.get_points()
    return ctx.step_index(), pxy.tobytes(), pm.tobytes()


def test_cell_limit_in_mid_chain():
    ref = crowded_stop(1, 0)
    assert 0 < ref[0] < 6000
    assert crowded_stop(8, 128) == ref


POINT_CAP = 32                 # the tile starts with 30 rectangles


@functools.lru_cache(maxsize=None)
def point_stop_reference():
    return stopped_run(limited_ctx(1, 0, 0, point_capacity=POINT_CAP), -12)


@pytest.mark.parametrize("deep", [128, 256])
def test_point_limit_stops_at_the_same_step(deep):
    ref = point_stop_reference()
    got = stopped_run(limited_ctx(8, deep, 0, point_capacity=POINT_CAP), -12)
    assert 0 < ref[0] < PACKED_STEPS               # (step 103)
    assert got == ref
