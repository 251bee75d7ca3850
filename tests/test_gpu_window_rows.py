"""The data-driven translation reads its window's row sums from the transposed table ``rowwin`` (csrc/mpp_window.hpp, built by
``k_rowwin``; option ``window_rows``, default 1) instead of forming each of them from two entries of the per-row prefix table.
An entry is the same subtraction of the same two doubles, so nothing may change: every case runs the same call under
``window_rows`` 1 and 0 (the chains get a null pointer and draw as before) in the one-wave kernel, the hot start from its
table, deep rounds of 8 and of 128 steps and at the adaptive depth from the queues, and the chain of eight waves whose state
lives in device memory, and compares final points and step index (an untraced call: the production kernels) and a traced
call's step records byte for byte.  One case runs in lockstep with the C oracle (decisions exactly, dE to
1e-9), and a context of three tiles checks the table's tile offset against the oracle's chain of the last tile.

The cases (tests/window_rows_cases.py) are chains of 3 000 steps (4 400 in the hot start: a shorter call does not start
hot), about 70 % of them data-driven translations.  The oracle counts on the CPU how many of them each chain accepts: at
least 100, so that no case passes without drawing."""
import numpy as np
import pytest

import window_rows_cases as wc
from helpers import lockstep_vs_oracle
from kernel_param_cases import make_oracle
from mpp_cnn_rs_object_detection_amd import hip_api
from test_gpu_kernel_params import CAP, make_ctx

pytestmark = pytest.mark.gpu

# (spec_waves, spec_lanes, deep, chain_state), options, steps (None: the case's)
FORMS = {
    "one-wave": ((1, 0, 0, 1), {}, None),
    "hot": ((8, 0, 128, 1), dict(handover=1, handover_at=2048, hot_table=1), wc.HOT_STEPS),     # 2048 is never reached: all of it hot
    "deep-8": ((8, 0, 128, 1), dict(handover=0, deep_fixed=8), None),
    "deep-128": ((8, 0, 128, 1), dict(handover=0, deep_fixed=128), None),
    "queues": ((8, 0, 128, 1), dict(handover=0), None),
    "hbm": ((8, 0, 0, 2), {}, None),
}


def run_form(b, form, rows, traced):
    shape, opts, steps = FORMS[form]
    steps = steps or b.case.steps
    ctx = make_ctx(b, shape)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_option("window_rows", rows)
    assert ctx.get_option("window_rows") == rows
    trace = b""
    if traced:
        out, props = ctx.run(steps, b.case.seed, chain0=b.case.chain, trace_tile=0)
        trace = out.tobytes() + props.tobytes()
    else:
        ctx.run(steps, b.case.seed, chain0=b.case.chain)
    xy, mk = ctx.get_points()
    used = dict(hot=ctx.get_option("hot_table_used"), queues=ctx.get_option("prepass_queues_used"), hbm=ctx.get_option("hbm_chains"),
                deep=ctx.deep_stats()["committed"])
    res = (xy.tobytes(), mk.tobytes(), ctx.step_index(), trace)
    ctx.close()
    return res, used, steps


@pytest.mark.parametrize("case", wc.CASES, ids=str)
def test_the_oracle_chain_accepts_translations(case):
    """what the comparisons below rest on: the chain of every case (and its longer hot form) really draws"""
    b = wc.build(case)
    for steps in (case.steps, wc.HOT_STEPS):
        out, props, _ = wc.oracle_chain(b, steps, case.chain)
        assert wc.accepted_translations(out, props) >= 100, (case.name, steps)


@pytest.mark.parametrize("traced", [False, True], ids=["points", "traces"])
@pytest.mark.parametrize("case", wc.CASES, ids=str)
def test_table_and_no_table_run_the_same_chain(case, traced):
    b = wc.build(case)
    _, _, want = wc.oracle_chain(b, case.steps, case.chain)
    for form in FORMS:
        on, used, steps = run_form(b, form, 1, traced)
        off, used_off, _ = run_form(b, form, 0, traced)
        assert on == off, (case.name, form, traced)
        assert on[2] == steps and used == used_off
        if not traced:                   # (the kernel the form is there for ran)
            if form == "hot":
                assert used["hot"] == 1 and used["deep"] == 0
            if form.startswith("deep") or form == "queues":
                assert used["deep"] == steps and used["queues"] == 1
            if form == "hbm":
                assert used["hbm"] == 1
        if steps == case.steps:          # ... and the chain is the oracle's
            xy = np.frombuffer(on[0], np.int32).reshape(-1, 2)
            mk = np.frombuffer(on[1], np.float64).reshape(-1, 3)
            np.testing.assert_array_equal(xy, want[0])
            np.testing.assert_allclose(mk, want[1], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("form", ["one-wave", "queues"])
def test_lockstep_with_the_oracle(form):
    """the clipped windows of the 20 x 12 tile, read from the table: proposals and decisions exactly, dE to 1e-9 (helpers.DE_TOL)"""
    case = wc.BY_NAME["20x12-md8"]
    b = wc.build(case)
    shape, opts, _ = FORMS[form]
    ctx = make_ctx(b, shape)
    for k, v in opts.items():
        ctx.set_option(k, v)
    assert ctx.get_option("window_rows") == 1
    o = make_oracle(b)
    assert lockstep_vs_oracle(ctx, o, case.steps, case.seed, case.chain, case.alpha) == 0
    gxy, gm = ctx.get_points()
    oxy, om = o.get_points()
    np.testing.assert_array_equal(gxy, oxy)
    np.testing.assert_allclose(gm, om, rtol=1e-9, atol=1e-9)
    ctx.close()


def three_tiles(case, form, rows):
    shape, opts, _ = FORMS[form]
    spec, lanes, deep, state = shape
    bs = [wc.build(case, map_seed=i) for i in range(3)]
    ctx = hip_api.MppContext(0, point_capacity=CAP, spec_waves=spec, spec_lanes=lanes, deep=deep, chain_state=state)
    ctx.set_maps(np.stack([b.det for b in bs]), [np.stack([b.marks[k] for b in bs]) for k in range(3)])
    ctx.set_model(bs[0].model, bs[0].maps)
    ctx.set_kernels(bs[0].kd)
    for i, b in enumerate(bs):
        ctx.set_points(i, b.xy, b.mk)
    ctx.set_schedule(case.T0, case.alpha, 0.0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_option("window_rows", rows)
    ctx.run(case.steps, case.seed, chain0=0)
    res = [ctx.get_points(i) + (ctx.step_index(i),) for i in range(3)]
    ctx.close()
    return bs, res


@pytest.mark.parametrize("form", ["one-wave", "queues"])
@pytest.mark.parametrize("name", ["20x12-md8", "33x47-md12"])
def test_three_tiles_read_their_own_table(name, form):
    """tile t's table starts t * H * W entries into the context's: chains 1 and 2 draw from theirs (on the 20 x 12 tiles the
    17 entries of the one-lane form reach into the next tile's table, and into the pad behind the last)"""
    case = wc.BY_NAME[name]
    bs, on = three_tiles(case, form, 1)
    _, off = three_tiles(case, form, 0)
    for t in range(3):
        assert on[t][0].tobytes() == off[t][0].tobytes() and on[t][1].tobytes() == off[t][1].tobytes() and on[t][2] == off[t][2] == case.steps
    for t in (1, 2):
        out, props, want = wc.oracle_chain(bs[t], case.steps, chain=t)
        assert wc.accepted_translations(out, props) >= 100
        np.testing.assert_array_equal(on[t][0], want[0])
        np.testing.assert_allclose(on[t][1], want[1], rtol=1e-9, atol=1e-9)
