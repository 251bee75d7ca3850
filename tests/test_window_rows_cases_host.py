"""The cases of tests/window_rows_cases.py draw what they are there for -- counted on the CPU oracle's own chain, no GPU.

The floors are conditions on the cases, not measurements of the code under test: a case that misses one is changed (seed,
intensity, length), the floor stays."""
import numpy as np
import pytest

import window_rows_cases as wc
from mpp_cnn_rs_object_detection_amd import kernels as K


@pytest.mark.parametrize("case", wc.CASES, ids=str)
def test_a_case_accepts_a_hundred_translations(case):
    b = wc.build(case)
    assert b.kd.p_kernel[K.K_DTRANS] > 0.65 and b.kd.max_delta == case.max_delta
    H, W = case.shape
    md = case.max_delta
    for steps in (case.steps, wc.HOT_STEPS):
        out, props, final = wc.oracle_chain(b, steps, case.chain)
        n = wc.accepted_translations(out, props)
        print(f"\n{case.name}: {steps} steps, {n} accepted data-driven translations, {len(final[0])} points at the end")
        assert n >= 100
    # the windows the case is there for (around the pixels the accepted translations left)
    dt = (props["kernel"] == K.K_DTRANS) & (props["target"] >= 0)
    assert dt.sum() >= 0.6 * steps
    if case.name.endswith(wc.ZERO_ROWS):
        assert not b.det[::5].any() and b.det[1::5].any()
    if md == 12:
        assert 2 * md + 1 > 17 and min(H, W) > 17          # windows of more than 17 rows exist on this tile
    if case.shape == (20, 12):
        assert W < 2 * md + 1 and H < 2 * md + 1 + 4        # every window is clipped in its columns, all but 4 rows' in theirs


def test_three_tiles_differ():
    a, b = wc.build(wc.CASES[0], 0), wc.build(wc.CASES[0], 2)
    assert not np.array_equal(a.det, b.det)
