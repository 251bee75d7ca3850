"""The cases of tests/kernel_param_cases.py exercise what they are there for -- counted on the CPU oracle's own walk, no GPU.

The floors are conditions on the cases, not measurements of the code under test: a case that misses one is changed (seed,
schedule, intensity), the floor stays.  Every count is printed (pytest -s shows them)."""
import json

import numpy as np
import pytest

import kernel_param_cases as kc
from mpp_cnn_rs_object_detection_amd import kernels as K


def test_the_cases_cover_the_parameters():
    by_map = {}
    for c in kc.CASES:
        by_map.setdefault(c.mapping, []).append(c)
    assert all(len(by_map[m]) >= 2 for m in ("default", "offset", "warped", "flags"))
    assert {c.max_delta for c in kc.CASES} >= {0, 3, 9, 12, 15}
    assert {c.kernel.get("sigma_trans", 2.0) for c in kc.CASES} >= {0.5, 3.5}
    assert {c.kernel.get("sigma_transform", 0.1) for c in kc.CASES} >= {0.02, 0.25}
    assert {c.setup for c in kc.CASES} == {"legacy", "no-calibration"}
    assert {c.shape for c in kc.CASES} >= {(48, 80), (5, 70), (70, 5), (1, 90), (40, 56), (1040, 24), (24, 1040)}
    sm = [c for c in kc.CASES if c.split_merge]
    assert len(sm) == 1 and sm[0].kernel["split_radius"] == 9.0 and sm[0].kernel["split_sigma"] == 0.2
    mix = [kc.build(c).kd.p_kernel for c in kc.CASES if c.weights and c.weights.get("uniform_bd_weight") == 0]
    assert len(mix) == 1 and mix[0][K.K_UBIRTH] == mix[0][K.K_UDEATH] == mix[0][K.K_GTRANS] == 0 and abs(mix[0].sum() - 1) < 1e-12
    for c in kc.CASES:
        assert 3000 <= c.steps <= 4000
        for m in kc.build(c).maps:                    # non-default cases really are non-default where they say so
            assert np.all(np.diff(m.feature_mapping) > 0)
    d = kc.build(kc.CASES[0]).kd
    assert (d.max_delta, d.sigma_trans, d.sigma_transform) == (12, 3.5, 0.25)
    m1, m3 = kc.make_mappings("offset"), kc.make_mappings("flags")
    assert [(m.v_min, m.v_max) for m in m1[:2]] == [(4, 28), (0.2, 1.0)] and m1[2].is_cyclic
    assert [m.is_cyclic for m in m3] == [False, True, False]


def test_the_warped_mapping_is_far_from_a_linspace():
    """the host's linspace test (|edge_i - (vmin + range * i / 32)| <= 1e-9 * (|range| + 1) for every i) must fail by a wide
    margin, so that the device takes the binary search and not the corrected guess"""
    for m in kc.make_mappings("warped"):
        i = np.arange(32)
        off = np.abs(m.feature_mapping - (m.v_min + m.range * i / 32))
        assert off.max() > 1e6 * 1e-9 * (abs(m.range) + 1.0)
        assert (off > 1e-9 * (abs(m.range) + 1.0)).sum() >= 30          # every edge but the first
        assert m.feature_mapping[0] == m.v_min
    for name in ("default", "offset", "flags"):
        for m in kc.make_mappings(name):
            off = np.abs(m.feature_mapping - (m.v_min + m.range * np.arange(32) / 32))
            assert off.max() <= 1e-9 * (abs(m.range) + 1.0)


@pytest.mark.parametrize("case", kc.CASES, ids=str)
def test_a_case_exercises_its_branches(case):
    w = kc.walk(case)
    c = kc.count(case, w)
    print(f"\n{case.name}: {json.dumps(c)}")
    H, W = case.shape
    kd = w.built.kd
    assert c["nan_dE"] == 0
    assert c["pop_median"] >= 5
    assert c["longest_empty_run"] <= 50
    for i in range(10):
        if kd.p_kernel[i] <= 0:
            continue
        name = K.KERNEL_NAMES[i]
        if i == K.K_SPLIT:
            assert c["accepted_Split"] >= 100
        elif i == K.K_MERGE:
            assert c["accepted_Merge"] >= 1
        else:
            assert c[f"proposed_{name}"] >= 100 and c[f"accepted_{name}"] >= 30, name
    if case.max_delta >= 9:
        assert c["dtrans_window_over_17"] >= 200 and c["dtrans_corner"] >= 50
    if min(H, W) <= 5:
        assert c["dtrans_spans_short_side"] >= 200
    if case.max_delta == 0:
        assert c["dtrans_own_pixel"] == c["dtrans"]
        assert c["dtrans"] >= 100
    if max(H, W) > 512:
        assert c["dbirth_beyond_512"] >= 50
    if case.kernel.get("sigma_transform") == 0.25:
        for j, m in enumerate(w.built.maps):
            assert c[f"gtransf_wraps_{j}" if m.is_cyclic else f"gtransf_at_range_end_{j}"] >= 10, j
    if case.mapping == "warped":
        assert c["proposals_off_the_linspace_class"] >= 100
