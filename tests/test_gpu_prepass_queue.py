"""The pre-pass queues of the deep rounds (csrc/mpp_prepass.hip, option ``prepass_queues``): with eight waves and the cost
deal, every wave takes its steps from per-type queues the pre-pass sorted, and its steps' proposals start from the heads
the pre-pass drew.  None of it may change the chain: traces and final configurations equal the ones of the births-only
table (``prepass_queues`` 0) and of no table (``prepass`` 0), bit for bit."""
import numpy as np
import pytest

import oracle
from helpers import model_for
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings, synth
from test_gpu_chain import setup_case

pytestmark = pytest.mark.gpu

MODES = {"none": (0, 0), "births": (1, 0), "queues": (1, 1)}


def set_mode(ctx, mode):
    prepass, queues = MODES[mode]
    ctx.set_option("prepass", prepass)
    ctx.set_option("prepass_queues", queues)


def run_case(mode, n_steps, seed, deep=128, fixed=0, handover=0, trace=True, gain=None, calls=1, setup_name="legacy",
             tile=128, n_obj=40, p_kernel=None, budget_mb=None):
    _, _, ctx = setup_case(tile, n_obj, setup_name, spec=8, deep=deep)
    if p_kernel is not None:                                 # a mixture of the caller's (kernels 0..7, no split / merge)
        xy, _ = ctx.get_points()
        kd = kernels.make_kernels(mappings.default_mappings(), max(1, len(xy)))
        kd.p_kernel = np.asarray(p_kernel, dtype=float)
        ctx.set_kernels(kd)
    if budget_mb is not None:
        ctx.set_option("prepass_mb", budget_mb)
    ctx.set_option("handover", handover)
    ctx.set_option("deep_fixed", fixed)
    set_mode(ctx, mode)
    if gain is not None:
        ctx.set_option("deep_gain", gain)
    ctx.set_schedule(1.0, 0.9985, 0.0)
    outs, used = [], []
    for _ in range(calls):
        if trace:
            outs.append(ctx.run(n_steps, seed, trace_tile=0))
        else:
            ctx.run(n_steps, seed)
        used.append(ctx.get_option("prepass_queues_used"))
    xy, m = ctx.get_points()
    return outs, xy, m, ctx, used


def assert_same(a, b):
    (oa, xa, ma, _, _), (ob, xb, mb, _, _) = a, b
    assert len(oa) == len(ob)
    for (out_a, props_a), (out_b, props_b) in zip(oa, ob):
        for f in out_a.dtype.names:
            np.testing.assert_array_equal(out_a[f], out_b[f], err_msg=f)
        assert props_a.tobytes() == props_b.tobytes()
    assert xa.tobytes() == xb.tobytes() and ma.tobytes() == mb.tobytes()


@pytest.mark.parametrize("deep,fixed", [(128, 0), (256, 0), (64, 8), (128, 32), (128, 128), (256, 256)])
def test_queues_give_the_same_chain(deep, fixed):
    """adaptive and fixed depths; at 256 a kernel type has more than 64 steps in a window and the window ends early"""
    n_steps, seed = 6000, 23
    base = run_case("none", n_steps, seed, deep=deep, fixed=fixed)
    births = run_case("births", n_steps, seed, deep=deep, fixed=fixed)
    que = run_case("queues", n_steps, seed, deep=deep, fixed=fixed)
    assert que[4] == [1] and births[4] == [0]
    assert_same(base, que)
    assert_same(births, que)
    assert que[3].deep_stats()["committed"] == n_steps
    un = run_case("queues", n_steps, seed, deep=deep, fixed=fixed, trace=False)   # the production instantiation
    assert un[1].tobytes() == base[1].tobytes() and un[2].tobytes() == base[2].tobytes()


@pytest.mark.parametrize("setup_name", ["no-calibration"])
def test_queues_other_model(setup_name):
    n_steps, seed = 6000, 29
    assert_same(run_case("births", n_steps, seed, setup_name=setup_name), run_case("queues", n_steps, seed, setup_name=setup_name))


@pytest.mark.parametrize("handover", [0, 1])
def test_hot_start_and_three_calls(handover):
    """the hot start hands the chain to the deep rounds inside the first call; the chain continues over three calls, each
    deep launch building its queues from the step it starts at"""
    n_steps, seed = 5000, 31
    base = run_case("none", n_steps, seed, handover=handover, calls=3)
    que = run_case("queues", n_steps, seed, handover=handover, calls=3)
    assert que[4][1:] == [1, 1] and (handover or que[4][0] == 1)
    assert_same(base, que)


def test_block_deal_does_not_use_queues():
    """deep_gain + 256 deals the sorted steps in blocks: the queues are not built, the chain is the same"""
    n_steps, seed = 4000, 37
    base = run_case("none", n_steps, seed, gain=12 + 256)
    que = run_case("queues", n_steps, seed, gain=12 + 256)
    assert que[4] == [0] and que[3].get_option("prepass_used") == 1
    assert_same(base, que)


def test_over_budget_falls_back():
    """prepass_mb 1: the queues of 200 000 steps do not fit (nor the birth records): the chain draws its steps itself"""
    n_steps, seed = 200000, 3
    ref = run_case("none", n_steps, seed, trace=False)
    _, _, ctx = setup_case(128, 40, "legacy", spec=8, deep=128)
    ctx.set_option("handover", 0)
    ctx.set_option("prepass_mb", 1)
    assert ctx.get_option("prepass_queues") == 1
    ctx.set_schedule(1.0, 0.9985, 0.0)
    ctx.run(n_steps, seed)
    assert ctx.get_option("prepass_queues_used") == 0
    xy, m = ctx.get_points()
    assert xy.tobytes() == ref[1].tobytes() and m.tobytes() == ref[2].tobytes()
    with pytest.raises(Exception):
        ctx.set_option("prepass_queues", 2)


def test_births_table_when_the_queues_do_not_fit():
    """prepass_mb 1, 22 000 steps: the queues alone fit (~0.88 MB), the queues and the ~3 700 birth records together do
    not, the births table and its records do (~0.44 MB): the launch runs the births table"""
    n_steps, seed = 22000, 5
    ref = run_case("none", n_steps, seed, trace=False)
    que = run_case("queues", n_steps, seed, trace=False, budget_mb=1)
    assert que[4] == [0] and que[3].get_option("prepass_used") == 1
    assert que[1].tobytes() == ref[1].tobytes() and que[2].tobytes() == ref[2].tobytes()


# kernels: uniform birth, uniform death, data-driven birth, data-driven death, Gaussian / data-driven translation,
# Gaussian / data-driven transform
@pytest.mark.parametrize("cut,p_kernel", [
    # wave 1: the uniform birth and death together ~77 of a 256-step window, each ~38 (> 64 together: 32 of each at most)
    ("uniform pair", [0.15, 0.15, 0.08, 0.08, 0.08, 0.30, 0.08, 0.08, 0.0, 0.0]),
    # waves 4 and 5: the data-driven translation ~154 of a 256-step window (> 128: the window ends after its 128th)
    ("translation halves", [0.05, 0.05, 0.06, 0.06, 0.06, 0.60, 0.06, 0.06, 0.0, 0.0]),
])
def test_windows_that_end_early(cut, p_kernel):
    """fixed depth 256 with a mixture that overfills one wave's share of the window: the queue rounds end early (fewer
    steps evaluated per round than the births-only rounds, which deal such a window in blocks), the chain is the same"""
    n_steps, seed = 6000, 41
    births = run_case("births", n_steps, seed, deep=256, fixed=256, p_kernel=p_kernel)
    que = run_case("queues", n_steps, seed, deep=256, fixed=256, p_kernel=p_kernel)
    assert que[4] == [1]
    assert_same(births, que)
    sb, sq = births[3].deep_stats(), que[3].deep_stats()
    assert sb["committed"] == sq["committed"] == n_steps
    per_b, per_q = sb["evaluated"] / sb["rounds"], sq["evaluated"] / sq["rounds"]
    assert per_b > 240 and per_q < 0.95 * per_b, (cut, per_b, per_q)
    base = run_case("none", n_steps, seed, deep=256, fixed=256, p_kernel=p_kernel, trace=False)
    un = run_case("queues", n_steps, seed, deep=256, fixed=256, p_kernel=p_kernel, trace=False)
    assert un[1].tobytes() == base[1].tobytes() and un[2].tobytes() == base[2].tobytes()


def multi_ctx(mode, n_chains, big=False):
    """n_chains chains in one launch, on 8 tiles' maps with chain keys of their own; big: tile 0 starts with 2 100 points,
    more than an LDS launch holds -- it runs in device memory next to the LDS chains"""
    setup, _, model = model_for("legacy")
    maps = mappings.default_mappings()
    rng = np.random.default_rng(5)
    base_tiles = [synth.make_tile(128 if not big else 256, 20, tile_id=900 + i, noise=0.1) for i in range(min(8, n_chains))]
    tiles, pts = [], []
    for i in range(n_chains):
        t = base_tiles[i % len(base_tiles)]
        o = oracle.Oracle(t.shape, t.det, t.marks, model, kernels.make_kernels(maps, 1.0))
        xy, mk = o.naive_detection(setup.detection_threshold, 6.0)
        if big and i == 0:
            k = rng.integers(0, len(xy), 2100)
            xy = rng.integers(0, t.shape[0], (2100, 2)).astype(np.int32)
            mk = mk[k]
        tiles.append(t); pts.append((xy, mk))
    if big:
        ctx = hip_api.MppContext(0, point_capacity=8192, cell_capacity=64, spec_waves=8)
    else:
        ctx = hip_api.MppContext(0, point_capacity=256, spec_waves=8)
    set_mode(ctx, mode)
    ctx.set_option("handover", 0)
    ctx.set_maps(np.stack([t.det for t in tiles]), [np.stack([t.marks[k] for t in tiles]) for k in range(3)])
    ctx.set_model(model, maps)
    ctx.set_kernels(kernels.make_kernels(maps, 1.0), intensity=np.array([float(max(1, len(p[0]))) for p in pts]))
    for i, (xy, mk) in enumerate(pts):
        ctx.set_points(i, xy, mk)
    ctx.set_chain_keys(np.arange(n_chains, dtype=np.uint64) + 40, np.arange(n_chains, dtype=np.uint32) * 3 + 1)
    ctx.set_schedule(1.0, 0.999, 0.0)
    return ctx


@pytest.mark.parametrize("n_chains,big", [(1, False), (16, False), (64, False), (5, True)])
def test_launches_of_many_chains(n_chains, big):
    runs = []
    for mode in ("births", "queues"):
        ctx = multi_ctx(mode, n_chains, big)
        for n_steps in (4000, 2000):                        # the second call starts at step0 != 0
            ctx.run(n_steps, 0)
            assert ctx.get_option("prepass_queues_used") == (1 if mode == "queues" else 0)
            if big:
                assert ctx.get_option("hbm_chains") == 1
        assert ctx.deep_stats()["rounds"] > 0
        runs.append([ctx.get_points(i) for i in range(n_chains)])
        ctx.close()
    for i, (a, b) in enumerate(zip(*runs)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), f"chain {i}"
