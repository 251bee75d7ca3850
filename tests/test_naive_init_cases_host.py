"""The cases of tests/naive_init_cases.py on the CPU: each reaches the edge it is there for, and the C oracle's
`naive_detection` -- the start of every oracle-checked chain -- gives the expectation (host_greedy, pinned to the reference's
recorded output, and np.argmax) on every one of them, centres in pick order and marks bit for bit."""
import numpy as np
import pytest

import naive_init_cases as nc
import oracle
from helpers import model_for
from kernel_param_cases import make_mappings
from mpp_cnn_rs_object_detection_amd import kernels

CAPACITY, REFIT_THR = 64, 0.95          # the capacity test of tests/test_gpu_naive_init.py on the stack (checked below)


def kept(e, r, c):
    return bool(len(e.centers)) and bool((e.centers == [r, c]).all(axis=1).any())


@pytest.mark.parametrize("name", nc.CASE_NAMES)
def test_case_keeps_enough_centres(name):
    case = nc.by_name(name)
    e = nc.expected(case)
    assert case.det.dtype == np.float32 and all(m.dtype == np.float32 and m.shape == case.shape + (32,) for m in case.marks)
    assert len(e.centers) >= case.min_kept
    assert e.n_cand >= len(e.centers)
    assert len(set(map(tuple, e.centers))) == len(e.centers)
    edges = nc.edges_of(case)
    assert all(np.isin(e.marks[:, k], edges[k]).all() for k in range(3))


def test_case_list_is_the_built_list():
    assert [c.name for c in nc.cases()] == nc.CASE_NAMES
    assert [c.name for c in nc.stack_cases()] == nc.STACK_NAMES


def test_fixture_cases_hold_the_float32_boundaries_and_the_recorded_results():
    g = nc.golden()
    det = g["det"]
    for name, thr in (("fixture-0.2", 0.2), ("fixture-0.7", 0.7)):
        case = nc.by_name(name)
        e = nc.expected(case)
        key = case.golden_key
        np.testing.assert_array_equal(e.centers, g[f"{key}_centers"])          # the reference's own output
        np.testing.assert_array_equal(e.classes, g[f"{key}_classes"])
        assert e.n_cand == int(g[f"{key}_n_cand"])
        # the three boundary values of test_fixture_holds_the_float32_threshold_boundaries: isolated pixels, so a candidate
        # among them is a centre
        t = np.float32(thr)
        below, above = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(2))
        for v, want in ((below, False), (t, True), (above, True)):
            (r,), (c,) = np.nonzero(det == v)
            assert kept(e, r, c) == want, (name, float(v))
    # float32 rounds 0.2 up and 0.7 and the shipped threshold down: there a double compare drops the pixel equal to float32(thr)
    assert float(np.float32(0.2)) > 0.2 and float(np.float32(0.7)) < 0.7 and float(np.float32(nc.SHIPPED_THR)) < nc.SHIPPED_THR
    (r,), (c,) = np.nonzero(det == np.float32(0.7))
    assert (r, c) == (197, 285) and not (np.float64(det[r, c]) >= 0.7)
    # the recorded tie pixels that are centres: the first of the tied maxima is the recorded class
    e = nc.expected(nc.by_name("fixture-0.2"))
    ties = [(tuple(rc), k, j) for rc, k, j in zip(g["tie_rc"], g["tie_k"], g["tie_j"]) if kept(e, *rc)]
    assert len(ties) >= 1
    marks = nc.by_name("fixture-0.2").marks
    for (r, c), k, j in ties:
        assert marks[k][r, c, j] == marks[k][r, c].max() and int(np.argmax(marks[k][r, c])) == int(g["mark_cls"][k, r, c]) < j


def test_cases_reach_their_edges():
    e = nc.expected(nc.by_name("zeros"))
    assert len(e.centers) == 16 * 24 and tuple(e.centers[-1]) == (0, 0) and tuple(e.centers[0]) == (15, 23)
    e = nc.expected(nc.by_name("ramp-thr0"))
    assert tuple(e.centers[-1]) == (0, 0) and nc.by_name("ramp-thr0").det[0, 0] == 0.0
    assert (np.diff(nc.by_name("ramp-thr0").det.ravel()) > 0).all()
    case = nc.by_name("ramp-thr-px01")
    e = nc.expected(case)
    assert np.float32(case.thr) == case.det[0, 1] and tuple(e.centers[-1]) == (0, 1) and not kept(e, 0, 0)
    e = nc.expected(nc.by_name("nms-lattice-d5"))
    assert e.n_cand == 3 and e.centers.tolist() == [[13, 16]]                   # of three tied peaks the largest index
    counts = [len(nc.expected(nc.by_name(f"nms-d{d}")).centers) for d in (0.0, 1.0, 4.5, 5.0, 6.0)]
    assert counts[0] == nc.expected(nc.by_name("nms-d0.0")).n_cand > counts[1] > counts[2] >= counts[4] == 30
    case = nc.by_name("plateau")
    e = nc.expected(case)
    assert case.det[0, 0] == 1.0 and case.det[-1, -1] == 1.0 and tuple(e.centers[0]) == (47, 79)
    assert (case.det[e.centers[:, 0], e.centers[:, 1]] == 1.0).all() and e.n_cand > 20 * len(e.centers)
    case = nc.by_name("negatives")
    e = nc.expected(case)
    v = case.det[e.centers[:, 0], e.centers[:, 1]]
    assert np.signbit(case.det[5, 5]) and case.det[5, 5] == 0 and not np.signbit(case.det[5, 7])
    assert (v < 0).sum() >= 10 and (v > 0).sum() >= 20 and (np.diff(v) <= 0).all()
    assert kept(e, 5, 7) and not kept(e, 5, 5)        # -0.0 ties with +0.0: the larger index wins, 2 px away
    # marks: tie pixels (a second maximum at class 31) are among the centres of every built case
    for name in ("plateau", "zeros", "negatives", "stack-noise"):
        case = nc.by_name(name)
        e = nc.expected(case)
        rows = [case.marks[k][e.centers[:, 0], e.centers[:, 1]] for k in range(3)]
        tied = sum(int(((r == r.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum()) for r in rows)
        assert tied >= 3, name


def test_stack_populations_and_the_capacity_scenario():
    pops = [len(nc.expected(c).centers) for c in nc.stack_cases()]
    assert pops[1] == 0 and len(set(pops)) == 5
    assert nc.by_name("stack-empty").det.max() == np.nextafter(np.float32(nc.STACK_THR), np.float32(0))
    np.testing.assert_array_equal(nc.expected(nc.by_name("stack-plateau")).centers, nc.expected(nc.by_name("plateau")).centers)
    # one tile (not the first) overflows CAPACITY, every tile fits it at REFIT_THR and keeps something to run a chain from
    assert [p > CAPACITY for p in pops] == [False, False, False, True, False]
    refit = [len(nc.expected(c, REFIT_THR).centers) for c in nc.stack_cases()]
    assert max(refit) <= CAPACITY and sum(refit) >= 20 and refit != pops


@pytest.mark.parametrize("name", nc.CASE_NAMES)
def test_oracle_naive_detection_equals_the_expectation(name):
    case = nc.by_name(name)
    e = nc.expected(case)
    _, _, model = model_for("legacy")
    o = oracle.Oracle(case.shape, case.det, case.marks, model, kernels.make_kernels(make_mappings(case.mapping), 1.0))
    xy, marks = o.naive_detection(case.thr, case.nms)
    assert len(xy) == len(e.centers), f"{name}: the oracle keeps {len(xy)} centres, the reference's rule {len(e.centers)}"
    np.testing.assert_array_equal(xy, e.centers)
    np.testing.assert_array_equal(marks, e.marks)
