"""The deep-round kernel does not evaluate a step that re-writes its target with the values it already holds
(csrc/mpp_deep.hip, ``deep_same_values``; option ``deep_skip_same``, default 1): no geometry, no unit terms, no place in the
neighbour pass, no accept test.  Such a step changes nothing whichever way its test goes, and in an untraced chain nothing
reads its outcome; its report is the one the evaluated step gets, up to the accept bit.

None of it may change the chain or a round: every case runs the same call with the option on and off and compares the final
configurations byte for byte with each other and with the one-wave kernel (``spec`` 1, ``deep`` 0), and the rounds, evaluated
and committed steps and rounds with a change of ``deep_stats()`` with each other.  A traced chain never skips: its records are
those of the option off, entry for entry.

The cases (tests/same_value_cases.py) are the smallest chains that hold such steps in numbers --
tests/test_same_value_cases_host.py counts at least 100 data-driven transforms and 5 translations of that kind in each, on
the oracle -- in every form of a deep round: the queue rounds at adaptive and fixed depths, the rounds that sort their steps
(with the birth table and without a pre-pass) on 1, 2, 4 and 8 waves, the instantiation with a classic image energy."""
import functools

import numpy as np
import pytest

import same_value_cases as sv
from mpp_cnn_rs_object_detection_amd import hip_api

pytestmark = pytest.mark.gpu

# form: (waves, deep, deep_fixed, prepass, prepass_queues)
FORMS = {"queues": (8, 128, 0, 1, 1), "queues-8": (8, 128, 8, 1, 1), "queues-64": (8, 128, 64, 1, 1), "queues-256": (8, 256, 256, 1, 1),
         "table": (8, 128, 0, 1, 0), "sorted": (8, 128, 0, 0, 1), "w1": (1, 64, 0, 1, 1), "w2": (2, 128, 0, 1, 1), "w4": (4, 256, 0, 1, 1)}
STAT_KEYS = ("rounds", "evaluated", "committed", "rounds_with_change")


def make_ctx(b, waves, deep, n_tiles=1, **caps):
    caps.setdefault("point_capacity", 256)
    ctx = hip_api.MppContext(0, spec_waves=waves, deep=deep, **caps)
    if n_tiles == 1:
        ctx.set_maps(b.det, b.marks)
    else:
        ctx.set_maps(np.stack([b.det] * n_tiles), [np.stack([m] * n_tiles) for m in b.marks])
    if b.image is not None:
        ctx.set_image(b.image)
    ctx.set_model(b.model, b.maps)
    ctx.set_kernels(b.kd, intensity=np.full(n_tiles, float(b.kd.intensity)))
    for t in range(n_tiles):
        ctx.set_points(t, b.xy, b.mk)
    ctx.set_schedule(b.T0, b.alpha, 0.0)
    ctx.set_option("handover", 0)
    return ctx


def deep_ctx(b, form, skip, **kw):
    waves, deep, fixed, prepass, queues = FORMS[form]
    ctx = make_ctx(b, waves, deep, **kw)
    ctx.set_option("deep_fixed", fixed)
    ctx.set_option("prepass", prepass)
    ctx.set_option("prepass_queues", queues)
    assert ctx.get_option("deep_skip_same") == 1                     # (the default)
    ctx.set_option("deep_skip_same", skip)
    assert ctx.get_option("deep_skip_same") == skip
    return ctx


def state(ctx, tile=0):
    xy, m = ctx.get_points(tile)
    return xy.tobytes(), m.tobytes(), ctx.step_index(tile)


@functools.lru_cache(maxsize=None)
def one_wave(name):
    """the case's chain in the one-wave kernel: (final state, traced records)"""
    b = sv.build(name)
    ctx = make_ctx(b, 1, 0)
    out, props = ctx.run(b.steps, b.seed, chain0=b.chain, trace_tile=0)
    res = state(ctx), out, props
    ctx.close()
    return res


def deep_run(name, form, skip):
    b = sv.build(name)
    ctx = deep_ctx(b, form, skip)
    ctx.run(b.steps, b.seed, chain0=b.chain)
    st = ctx.deep_stats()
    used = ctx.get_option("prepass_queues_used"), ctx.get_option("prepass_used")
    res = state(ctx)
    ctx.close()
    assert st["committed"] == b.steps and st["rounds"] > 0, st
    return res, st, used


def both_ways(name, form):
    (on, st_on, used), (off, st_off, _) = deep_run(name, form, 1), deep_run(name, form, 0)
    print(name, form, "on", st_on, "off", st_off)
    assert on == off, "the option changes the chain"
    assert on == one_wave(name)[0], "deep rounds differ from the one-wave kernel"
    assert {k: st_on[k] for k in STAT_KEYS} == {k: st_off[k] for k in STAT_KEYS}
    return st_on, used


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["tile112", "packed"])
def test_small_tiles_in_every_form_of_a_round(name, form):
    st, (queues_used, table_used) = both_ways(name, form)
    waves, _, fixed, prepass, queues = FORMS[form]
    assert queues_used == (1 if waves == 8 and prepass and queues else 0)
    assert table_used == prepass
    if fixed == 8:
        assert st["evaluated"] <= 8 * st["rounds"]
    if name == "packed":
        assert st["rounds_with_change"] > 0                           # (steps that change more than two neighbours: the second pass)


@pytest.mark.parametrize("form", ["queues", "sorted", "w2"])
def test_initial_marks_off_the_class_values(form):
    """the first data-driven transform of a mark into the class it sits in proposes the class EDGE, another value: it is
    evaluated, and where it is accepted it changes the configuration.  A kernel that compared classes would skip it."""
    both_ways("off-class", form)


@pytest.mark.parametrize("form", ["sorted", "w1"])
def test_contrast_energy_setup(form):
    """the instantiation with a classic image energy (the contrast pre-term of a wave's rectangles is cooperative: a skipped
    step takes no part in it); nine in ten of this chain's steps are rejected for a NaN, as in the one-wave kernel"""
    assert int(np.isnan(one_wave("contrast")[1]["dE"]).sum()) > 1000
    both_ways("contrast", form)


@pytest.mark.parametrize("form", ["queues", "w4"])
def test_from_the_empty_configuration(form):
    both_ways("empty", form)


def test_cell_capacity_stop_in_mid_chain_and_a_continued_call():
    b = sv.build("capacity")
    runs = {}
    for skip in (1, 0):
        ctx = deep_ctx(b, "queues", skip, cell_capacity=3)
        ctx.set_option("auto_grow", 0)
        with pytest.raises(hip_api.MppError) as e:
            ctx.run(b.steps, b.seed, chain0=b.chain)
        assert e.value.code == -11 and "cell" in str(e.value)
        stopped, st0, at_stop = ctx.step_index(), ctx.deep_stats(), state(ctx)
        assert 0 < stopped < b.steps
        pxy, pm = ctx.get_points()
        ctx.set_option("cell_capacity", 32)
        ctx.set_points(0, pxy, pm)                                    # (clears the sticky error; step and temperature stay)
        ctx.run(b.steps - stopped, b.seed, chain0=b.chain)
        runs[skip] = at_stop, {k: st0[k] for k in STAT_KEYS}, state(ctx), {k: ctx.deep_stats()[k] for k in STAT_KEYS}
        ctx.close()
    assert runs[1] == runs[0]
    assert runs[1][2] == one_wave("capacity")[0]


def test_hot_start_hands_over_to_the_deep_rounds():
    b = sv.build("hot-start")
    runs = {}
    for skip in (1, 0):
        ctx = deep_ctx(b, "queues", skip)
        ctx.set_option("handover", 1)
        ctx.set_option("handover_at", 256)                            # (the hot launch ends after its first 48 rounds)
        ctx.run(b.steps, b.seed, chain0=b.chain)
        st = ctx.deep_stats()
        assert ctx.get_option("hot_table_used") == 1 and 0 < st["committed"] < b.steps, st
        runs[skip] = state(ctx), {k: st[k] for k in STAT_KEYS}
        ctx.close()
    assert runs[1] == runs[0]
    assert runs[1][0] == one_wave("hot-start")[0]


@pytest.mark.parametrize("name,form", [("tile112", "queues"), ("packed", "w2"), ("contrast", "sorted")])
def test_a_traced_chain_never_skips(name, form):
    b = sv.build(name)
    rec = {}
    for skip in (1, 0):
        ctx = deep_ctx(b, form, skip)
        out, props = ctx.run(b.steps, b.seed, chain0=b.chain, trace_tile=0)
        rec[skip] = out.tobytes(), props.tobytes(), state(ctx), {k: ctx.deep_stats()[k] for k in STAT_KEYS}
        ctx.close()
    assert rec[1] == rec[0]
    _, out1, props1 = one_wave(name)
    assert rec[1][1] == props1.tobytes()
    out = np.frombuffer(rec[1][0], dtype=out1.dtype)
    np.testing.assert_array_equal(out["accepted"], out1["accepted"])
    np.testing.assert_array_equal(out["n_after"], out1["n_after"])


def test_the_untraced_chain_of_a_traced_launch_skips():
    """two chains on the same maps, the first one traced: the launch runs the traced instantiation, in which the second chain
    is untraced and skips"""
    b = sv.build("tile112")
    res = {}
    for key, (form, skip) in {"one-wave": (None, 1), "on": ("queues", 1), "off": ("queues", 0)}.items():
        ctx = make_ctx(b, 1, 0, n_tiles=2) if form is None else deep_ctx(b, form, skip, n_tiles=2)
        out, props = ctx.run(b.steps, b.seed, chain0=b.chain, trace_tile=0)
        res[key] = props.tobytes(), out["accepted"].tobytes(), state(ctx, 0), state(ctx, 1)
        ctx.close()
    assert res["on"] == res["off"] == res["one-wave"]
    assert res["on"][2] != res["on"][3]                               # (chain ids 0 and 1: two different chains)
