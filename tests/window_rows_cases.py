"""Chains that are mostly data-driven translation, for the window's row table (host side: no GPU import).

The cases of tests/test_gpu_window_rows.py, built the way tests/kernel_param_cases.py builds its mixtures (overrides of
``kernels.BASE_KERNEL_WEIGHTS``): three quarters of the steps are translations, sixteen in seventeen of those are
data-driven, so about 70 % of a chain's steps draw a pixel from the window around their target.  The tiles are the smallest
at which the draw can go wrong: 20 x 12 (with max_delta 8 every window is clipped, most on three or four sides, and the 17
entries the one-lane form reads run past the window's last row into the next column, the next tile's table or the pad behind
the last table), 33 x 47 at max_delta 1 and at 12 (windows of more than 17 rows: the loop form), 64 x 64 at the default 8
(whole 17 x 17 windows in the middle), and 33 x 47 with every fifth row of the detection map zero (row sums of 0: equal
partial sums in the walk).  ``accepted_translations`` counts on the CPU oracle what a chain really draws."""
from __future__ import annotations

import dataclasses

import numpy as np

import kernel_param_cases as kc
from mpp_cnn_rs_object_detection_amd import kernels as K

MOSTLY_TRANSLATION = dict(translation_weight=6, gaussian_translation_weight=0.25, data_translation_weight=4)
ZERO_ROWS = "zero-rows"                 # (the case whose detection map has all-zero rows)


def _case(name, shape, md, seed, intensity, **kw):
    return kc.Case(name, shape, "default", "legacy", dict(max_delta=md), intensity, seed=seed, steps=3000, weights=MOSTLY_TRANSLATION, **kw)


CASES = [
    _case("20x12-md8", (20, 12), 8, 401, 6.0),
    _case("33x47-md1", (33, 47), 1, 402, 12.0),
    _case("33x47-md12", (33, 47), 12, 403, 12.0),
    _case("64x64-md8", (64, 64), 8, 404, 20.0),
    _case("33x47-md8-" + ZERO_ROWS, (33, 47), 8, 405, 12.0),
]
BY_NAME = {c.name: c for c in CASES}
HOT_STEPS = 4400                        # a call of fewer than 4 096 steps does not start hot


def build(case: kc.Case, map_seed: int = 0) -> kc.Built:
    b = kc.build(dataclasses.replace(case, map_seed=map_seed))
    if case.name.endswith(ZERO_ROWS):
        b.det = b.det.copy()
        b.det[::5, :] = 0.0
    return b


def oracle_chain(b: kc.Built, steps: int, chain: int = 0):
    """the oracle's own chain of `steps` steps from the case's start: (out, props, final points)"""
    o = kc.make_oracle(b)
    out, props = o.run(steps, b.case.seed, chain=chain, trace=True)
    return out, props, o.get_points()


def accepted_translations(out, props) -> int:
    return int(((props["kernel"] == K.K_DTRANS) & (props["target"] >= 0) & (out["accepted"] > 0)).sum())
