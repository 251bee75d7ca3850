"""Chains that outgrow a CU's LDS continue with their state in device memory (option chain_state, mpp_chain_hbm_kernel):
the chain is the one an unlimited capacity would have produced, only the chains that need it leave the LDS, and
chain_state 1 keeps the LDS-only behaviour (-12 / -11 / -7)."""
import numpy as np
import pytest

import oracle
from helpers import Tape, lockstep_vs_oracle, model_for, soak_case
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings, synth

pytestmark = pytest.mark.gpu
DENSE_CASE = 1401        # 256 px, no-calibration, split / merge, crowded, T0 = 5: more than 1 024 points (-12 LDS-only)


def oracle_final(c):
    t = c["tile"]
    o = oracle.Oracle(t.shape, t.det, t.marks, c["model"], c["kd"])
    o.set_points(c["xy"], c["marks"]); o.set_temperature(c["T0"], c["alpha"], 0.0)
    o.run(c["steps"], c["seed"], chain=c["chain"])
    return o.get_points()


def soak_ctx(c, spec=8, chain_state=None):
    t = c["tile"]
    ctx = hip_api.MppContext(0, point_capacity=1024, spec_waves=spec, chain_state=chain_state)
    ctx.set_maps(t.det, t.marks); ctx.set_model(c["model"], mappings.default_mappings()); ctx.set_kernels(c["kd"])
    ctx.set_points(0, c["xy"], c["marks"]); ctx.set_schedule(c["T0"], c["alpha"], 0.0)
    return ctx


@pytest.fixture(scope="module")
def dense():
    c = soak_case(DENSE_CASE)
    return c, oracle_final(c)


@pytest.mark.parametrize("spec", [8, 1])
def test_soak_case_1401_runs_to_the_oracle_result(dense, spec):
    c, (oxy, om) = dense
    ctx = soak_ctx(c, spec)
    ctx.run(c["steps"], c["seed"], chain0=c["chain"])
    gxy, gm = ctx.get_points()
    np.testing.assert_array_equal(gxy, oxy, err_msg=f"{c['text']} spec {spec}")
    np.testing.assert_allclose(gm, om, rtol=1e-9, atol=1e-9)
    assert len(gxy) > 1024
    assert ctx.get_option("hbm_chains") == 1
    assert ctx.get_option("hbm_bytes") > 0
    assert ctx.get_option("point_capacity") > 1024


def test_dense_chain_grows_twice_in_device_memory():
    """Uniform births at intensity 20 000 and T = 1e6: the population passes the 1 024 slots an LDS launch holds on a
    256-px tile, then 2 048 in device memory (grown to 4 096).  Every step equals the oracle (lockstep, traced tile)."""
    t = synth.make_tile(256, 40, tile_id=77, noise=0.1)
    setup, comb, model = model_for("legacy")
    kd = kernels.make_kernels(mappings.default_mappings(), 20000.0)
    o = oracle.Oracle(t.shape, t.det, t.marks, model, kd)
    xy, mk = o.naive_detection(setup.detection_threshold, 6.0)
    o.set_points(xy, mk); o.set_temperature(1e6, 1.0, 0.0)
    ctx = hip_api.MppContext(0, point_capacity=512, spec_waves=8)
    ctx.set_maps(t.det, t.marks); ctx.set_model(model, mappings.default_mappings()); ctx.set_kernels(kd)
    ctx.set_points(0, xy, mk); ctx.set_schedule(1e6, 1.0, 0.0)
    lockstep_vs_oracle(ctx, o, 16000, seed=1234, chain=3, alpha=1.0, chunk=4000)
    gxy, gm = ctx.get_points()
    oxy, om = o.get_points()
    np.testing.assert_array_equal(gxy, oxy)
    np.testing.assert_allclose(gm, om, rtol=1e-9, atol=1e-9)
    assert len(gxy) > 2048
    assert ctx.get_option("point_capacity") >= 4096          # 512 -> 1024 in LDS, 2048 -> 4096 in device memory
    assert ctx.get_option("grow_events") >= 3
    assert ctx.get_option("hbm_chains") == 1


def small_ctx(setup_name, spec, chain_state, split_merge=False):
    t = synth.make_tile(128, 40, tile_id=3, noise=0.2)
    setup, comb, model = model_for(setup_name)
    o = oracle.Oracle(t.shape, t.det, t.marks, model, kernels.make_kernels(mappings.default_mappings(), 1.0))
    xy, mk = o.naive_detection(setup.detection_threshold, 6.0)
    kd = kernels.make_kernels(mappings.default_mappings(), max(1, len(xy)), use_split_merge=split_merge)
    ctx = hip_api.MppContext(0, point_capacity=256, spec_waves=spec, deep=0, chain_state=chain_state)
    ctx.set_maps(t.det, t.marks); ctx.set_model(model, mappings.default_mappings()); ctx.set_kernels(kd)
    ctx.set_points(0, xy, mk); ctx.set_schedule(1.0, 0.998, 0.0)
    return ctx


def assert_same_run(a, b):
    (ao, ap, axy, am), (bo, bp, bxy, bm) = a, b
    assert ao.tobytes() == bo.tobytes() and ap.tobytes() == bp.tobytes()
    assert axy.tobytes() == bxy.tobytes() and am.tobytes() == bm.tobytes()


@pytest.mark.parametrize("setup_name,split_merge,spec", [
    ("legacy", False, 1), ("legacy", False, 8), ("no-calibration", False, 1), ("no-calibration", False, 8),
    ("legacy", True, 1), ("legacy", True, 8),
    ("legacy", False, 4)])                                   # spec_waves 4 runs the 8-wave HBM kernel: the same chain
def test_forced_device_memory_equals_lds(setup_name, split_merge, spec):
    runs = []
    for state in (0, 2):
        ctx = small_ctx(setup_name, spec, state, split_merge)
        out, props = ctx.run(3000, 29, chain0=5, trace_tile=0)
        runs.append((out, props) + tuple(ctx.get_points()))
        assert ctx.get_option("hbm_chains") == (1 if state == 2 else 0)
    assert_same_run(*runs)


@pytest.mark.parametrize("spec", [1, 8])
@pytest.mark.parametrize("name", ["tape_hrc_64.npz", "tape_contrast_96.npz", "tape_hrc_96_sm.npz"])
def test_forced_device_memory_replays_a_tape_like_lds(name, spec):
    """mpp_replay goes through the same routing: the reference's tapes (legacy, the contrast image energy, split /
    merge) give the same records and final configuration in device memory as in LDS."""
    t = Tape(name)
    runs = []
    for state in (0, 2):
        ctx = hip_api.MppContext(0, point_capacity=256, spec_waves=spec, chain_state=state)
        ctx.set_maps(t.det, t.marks)
        if t.image is not None:
            ctx.set_image(t.image)
        ctx.set_model(t.model, mappings.default_mappings()); ctx.set_kernels(t.kernels)
        ctx.set_points(0, t.init_xy, t.init_marks)
        p = t.params
        ctx.set_schedule(p["init_temperature"], p["alpha_t"], p["target_temperature"])
        out = ctx.replay(0, t.proposals)
        runs.append((out, t.proposals) + tuple(ctx.get_points()))
        assert ctx.get_option("hbm_chains") == (1 if state == 2 else 0)
    np.testing.assert_array_equal(runs[1][0]["accepted"], t.col("accepted").astype(int))
    assert_same_run(*runs)


def batch(c, extra, with_dense, chain_state=None):
    """the dense tile of case 1401 (tile 0, when with_dense) plus `extra` ordinary 256-px tiles, one model / kernel
    mixture / schedule, each chain with its own Philox key"""
    tiles, pts, keys, lam = [], [], [], []
    if with_dense:
        tiles.append(c["tile"]); pts.append((c["xy"], c["marks"])); keys.append((c["seed"], c["chain"]))
        lam.append(c["kd"].intensity)
    setup, _, _ = model_for("no-calibration")
    for i in range(extra):
        t = synth.make_tile(256, 30, tile_id=900 + i, noise=0.1)
        o = oracle.Oracle(t.shape, t.det, t.marks, c["model"], c["kd"])
        tiles.append(t); pts.append(o.naive_detection(setup.detection_threshold, 6.0)); keys.append((1000 + i, 50 + 3 * i))
        lam.append(float(max(1, len(pts[-1][0]))))           # each tile's own birth intensity, as the sampler sets it
    ctx = hip_api.MppContext(0, point_capacity=1024, spec_waves=8, chain_state=chain_state)
    ctx.set_maps(np.stack([t.det for t in tiles]), [np.stack([t.marks[k] for t in tiles]) for k in range(3)])
    ctx.set_model(c["model"], mappings.default_mappings()); ctx.set_kernels(c["kd"], intensity=np.array(lam))
    for i, (xy, mk) in enumerate(pts):
        ctx.set_points(i, xy, mk)
    ctx.set_chain_keys(np.array([k[0] for k in keys], np.uint64), np.array([k[1] for k in keys], np.uint32))
    ctx.set_schedule(c["T0"], c["alpha"], 0.0)
    return ctx


def test_one_overfull_tile_among_many(dense):
    c, (oxy, om) = dense
    extra, more = 7, 3000
    ctx = batch(c, extra, True)
    ctx.run(c["steps"], 0)
    assert ctx.get_option("hbm_chains") == 1
    gxy, gm = ctx.get_points(0)
    np.testing.assert_array_equal(gxy, oxy)
    np.testing.assert_allclose(gm, om, rtol=1e-9, atol=1e-9)
    ref = batch(c, extra, False, chain_state=1)             # LDS only: it raises if any of these chains outgrew the LDS
    ref.run(c["steps"], 0)
    assert ref.get_option("hbm_chains") == 0
    for i in range(extra):
        a, b = ctx.get_points(1 + i), ref.get_points(i)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), f"tile {1 + i}"
    # the next call on the same context: the dense tile goes on in device memory, the others in LDS
    ctx.run(more, 0)
    assert ctx.get_option("hbm_chains") == 1
    whole = batch(c, extra, False, chain_state=1)
    whole.run(c["steps"] + more, 0)                          # uninterrupted, LDS only
    for i in range(extra):
        a, b = ctx.get_points(1 + i), whole.get_points(i)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), f"tile {1 + i} (second call)"
    assert ctx.step_index(0) == c["steps"] + more


def test_lds_only_keeps_todays_behaviour(dense):
    c, _ = dense
    ctx = soak_ctx(c, 8, chain_state=1)
    with pytest.raises(hip_api.MppError) as e:
        ctx.run(c["steps"], c["seed"], chain0=c["chain"])
    assert e.value.code == -12
    assert "chain_state is 1" in str(e.value)
    xy, _ = ctx.get_points()
    assert len(xy) == ctx.get_option("point_capacity")      # stopped before the birth that did not fit, state written back
    assert 0 < ctx.step_index(0) < c["steps"]
    assert ctx.get_option("hbm_chains") == 0
    with pytest.raises(hip_api.MppError):
        ctx.set_option("chain_state", 3)
    assert ctx.get_option("chain_state") == 1
