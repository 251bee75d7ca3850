"""The queue rounds of the deep kernel keep their live state out of private memory (csrc/mpp_deep.hip): the fields of a
step that the neighbour pass does not read wait in LDS while it runs -- u_acc, qf, qb in the step's own report slots,
lin_a and gate_a in the space of the sorted Philox words until deep_mutate writes the slot -- the step's temperature is
read from the ring again, and the commit decision keeps two chunks of reports per lane where a round has at most 128
steps.  None of it may change the chain: everything here equals the one-wave kernel (``spec`` 1, ``deep`` 0) byte for byte."""
import functools

import numpy as np
import pytest

import oracle
from helpers import model_for
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings, synth
from test_gpu_chain import setup_case
from test_gpu_deep import deep_case

pytestmark = pytest.mark.gpu


def finish(ctx, n_steps, seed, trace):
    res = ctx.run(n_steps, seed, trace_tile=0) if trace else None
    if not trace:
        ctx.run(n_steps, seed)
    xy, m = ctx.get_points()
    return res, xy, m, ctx.step_index()


def assert_same_chain(ref, got, traced):
    (r_out, r_props), r_xy, r_m, r_step = ref
    g_res, g_xy, g_m, g_step = got
    if traced:
        for f in r_out.dtype.names:
            np.testing.assert_array_equal(r_out[f], g_res[0][f], err_msg=f)
        assert r_props.tobytes() == g_res[1].tobytes()
    assert r_xy.tobytes() == g_xy.tobytes() and r_m.tobytes() == g_m.tobytes()
    assert r_step == g_step


# ---- second pass with parked state: a tile packed with strongly overlapping rectangles at a hot temperature
PACKED_STEPS, PACKED_SEED = 4000, 5


def packed_ctx(spec, deep):
    _, _, ctx = setup_case(96, 30, "legacy", spec=spec, cap=256, deep=deep)
    rng = np.random.default_rng(3)
    xy = rng.integers(24, 72, (30, 2)).astype(np.int32)                    # 30 rectangles ~33 x 16 px within 48 x 48 px
    marks = np.stack([rng.uniform(20.0, 30.0, 30), rng.uniform(0.3, 0.6, 30), rng.uniform(0.0, np.pi, 30)], axis=1)
    ctx.set_points(0, xy, marks)
    ctx.set_option("handover", 0)
    ctx.set_schedule(5.0, 0.9995, 0.0)
    return ctx


@functools.lru_cache(maxsize=None)
def packed_reference():
    return finish(packed_ctx(1, 0), PACKED_STEPS, PACKED_SEED, True)


@pytest.mark.parametrize("traced", [True, False])
def test_second_pass_reads_the_parked_fields(traced):
    """steps that change more than two neighbours commit: they run the second pass (stage 0), whose deep_mutate reads
    lin_a / gate_a back from LDS, next to steps that commit without it"""
    ctx = packed_ctx(8, 128)
    got = finish(ctx, PACKED_STEPS, PACKED_SEED, traced)
    assert ctx.get_option("prepass_queues_used") == 1
    st = ctx.deep_stats()
    assert st["committed"] == PACKED_STEPS and st["rounds_with_change"] > 0, st
    assert_same_chain(packed_reference(), got, traced)


# ---- one lane per wave, a full window, and the four-chunk instantiation
FIXED_STEPS, FIXED_SEED = 4000, 13


@functools.lru_cache(maxsize=None)
def fixed_reference():
    _, _, c1 = setup_case(128, 40, "legacy", spec=1)
    c1.set_schedule(1.0, 0.9985, 0.0)
    return finish(c1, FIXED_STEPS, FIXED_SEED, True)


@pytest.mark.parametrize("deep,fixed", [(128, 8), (128, 128), (256, 256)])
def test_fixed_windows_untraced(deep, fixed):
    """the production (untraced) instantiation: 8 steps a round (one lane per wave), 128 (every report of the two chunks
    in use), and 256 (the instantiation that keeps four chunks)"""
    _, _, ctx = deep_case(128, 40, "legacy", 8, deep, fixed)
    ctx.set_option("handover", 0)
    ctx.set_schedule(1.0, 0.9985, 0.0)
    got = finish(ctx, FIXED_STEPS, FIXED_SEED, False)
    assert ctx.get_option("prepass_queues_used") == 1
    st = ctx.deep_stats()
    assert st["committed"] == FIXED_STEPS
    if fixed == 8:
        assert st["evaluated"] <= 8 * st["rounds"]
    assert_same_chain(fixed_reference(), got, False)


# ---- routed launch: one chain in device memory next to LDS chains
def routed_ctx(spec, deep, n_chains=5):
    """as tests/test_gpu_prepass_queue.py: tile 0 starts with 2 100 points, more than an LDS launch holds"""
    setup, _, model = model_for("legacy")
    maps = mappings.default_mappings()
    rng = np.random.default_rng(5)
    tiles, pts = [], []
    for i in range(n_chains):
        t = synth.make_tile(256, 20, tile_id=900 + i, noise=0.1)
        o = oracle.Oracle(t.shape, t.det, t.marks, model, kernels.make_kernels(maps, 1.0))
        xy, mk = o.naive_detection(setup.detection_threshold, 6.0)
        if i == 0:
            k = rng.integers(0, len(xy), 2100)
            xy = rng.integers(0, t.shape[0], (2100, 2)).astype(np.int32)
            mk = mk[k]
        tiles.append(t); pts.append((xy, mk))
    ctx = hip_api.MppContext(0, point_capacity=8192, cell_capacity=64, spec_waves=spec, deep=deep)
    ctx.set_option("handover", 0)
    ctx.set_maps(np.stack([t.det for t in tiles]), [np.stack([t.marks[k] for t in tiles]) for k in range(3)])
    ctx.set_model(model, maps)
    ctx.set_kernels(kernels.make_kernels(maps, 1.0), intensity=np.array([float(max(1, len(p[0]))) for p in pts]))
    for i, (xy, mk) in enumerate(pts):
        ctx.set_points(i, xy, mk)
    ctx.set_chain_keys(np.arange(n_chains, dtype=np.uint64) + 40, np.arange(n_chains, dtype=np.uint32) * 3 + 1)
    ctx.set_schedule(1.0, 0.999, 0.0)
    return ctx


def test_routed_launch_equals_one_wave_chains():
    n_chains, n_steps = 5, 3000
    runs = []
    for spec, deep in ((1, 0), (8, 128)):
        ctx = routed_ctx(spec, deep, n_chains)
        ctx.run(n_steps, 0)
        assert ctx.get_option("hbm_chains") == 1
        if deep:
            assert ctx.get_option("prepass_queues_used") == 1 and ctx.deep_stats()["rounds"] > 0
        runs.append([ctx.get_points(i) + (ctx.step_index(i),) for i in range(n_chains)])
        ctx.close()
    for i, (a, b) in enumerate(zip(*runs)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], f"chain {i}"
