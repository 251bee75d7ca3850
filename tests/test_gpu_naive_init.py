"""k_naive_init (csrc/mpp_maps.hip), the start of every chain, against the reference's rule at its edges: the cases of
tests/naive_init_cases.py, whose expectation is the host greedy pinned to the reference's recorded output and np.argmax over
the mark rows (tests/test_naive_init_cases_host.py shows on the CPU that each case reaches its edge).  Everything is an exact
comparison.  Run with -s for the candidate and kept counts of every case."""
import numpy as np
import pytest

import naive_init_cases as nc
from helpers import model_for
from kernel_param_cases import make_mappings
from mpp_cnn_rs_object_detection_amd import cnn_detection as cd
from mpp_cnn_rs_object_detection_amd import hip_api, kernels
from test_naive_init_cases_host import CAPACITY, REFIT_THR

pytestmark = pytest.mark.gpu


def make_ctx(dets, marks, mapping, capacity):
    """a context over one tile ([H, W]) or a stack ([T, H, W]) under the legacy model (naive_init reads its mapping table only)"""
    _, _, model = model_for("legacy")
    ctx = hip_api.MppContext(0, point_capacity=capacity)
    ctx.set_maps(dets, marks)
    ctx.set_model(model, make_mappings(mapping))
    return ctx


def case_ctx(case, capacity=None):
    e = nc.expected(case)
    return make_ctx(case.det, case.marks, case.mapping, capacity or max(64, len(e.centers) + 8))


def stack_ctx(capacity):
    tiles = nc.stack_cases()
    det = np.stack([c.det for c in tiles])
    marks = [np.stack([c.marks[k] for c in tiles]) for k in range(3)]
    return make_ctx(det, marks, tiles[0].mapping, capacity), tiles


def assert_points(got, e, n=None):
    xy, marks = got
    n = len(e.centers) if n is None else n
    assert len(xy) == n, f"{len(xy)} centres, expected {n}"
    np.testing.assert_array_equal(xy, e.centers[:n])                   # the same centres in the same pick order
    assert marks.dtype == np.float64 and marks.tobytes() == e.marks[:n].tobytes()      # table values, bit for bit


@pytest.mark.parametrize("name", nc.CASE_NAMES)
def test_naive_init_equals_the_reference_rule(name):
    case = nc.by_name(name)
    e = nc.expected(case)
    ctx = case_ctx(case)
    ctx.naive_init(case.thr, case.nms)
    got = ctx.get_points()
    print(f"\n{name}: {case.shape[0]} x {case.shape[1]}, thr {case.thr!r}, distance {case.nms}: {e.n_cand} candidates, "
          f"{len(e.centers)} kept by the rule, {len(got[0])} by the device")
    assert_points(got, e)
    assert ctx.counts().tolist() == [len(e.centers)]


@pytest.mark.parametrize("name", ["fixture-0.2", "fixture-0.7", "fixture-shipped"])
def test_fixture_meets_the_baseline_detector_and_the_recorded_result(name):
    """both implementations of naive_detection -- k_naive_init and mpp_detect_centers / mpp_mark_classes -- on the reference's
    recorded map: equal to each other and to the recording, the float32(thr) boundary pixels on the right side"""
    case = nc.by_name(name)
    g = nc.golden()
    ctx = case_ctx(case)
    ctx.naive_init(case.thr, case.nms)
    xy, marks = ctx.get_points()
    centers, _, n_cand = cd.detect_centers(case.det, case.thr, strict=False, nms_distance=case.nms)
    print(f"\n{name}: {n_cand} candidates, {len(centers)} kept by the baseline detector, {len(xy)} by the naive init")
    np.testing.assert_array_equal(xy, centers)
    values = cd.mark_values(case.marks, centers, make_mappings(case.mapping))
    assert marks.tobytes() == values.tobytes()
    if case.golden_key:
        np.testing.assert_array_equal(xy, g[f"{case.golden_key}_centers"])
        edges = nc.edges_of(case)
        cls = g[f"{case.golden_key}_classes"].astype(np.int64)
        assert marks.tobytes() == np.stack([edges[k][cls[:, k]] for k in range(3)], axis=1).tobytes()
        t = np.float32(case.thr)
        kept = {tuple(c) for c in xy}
        for v, want in ((np.nextafter(t, np.float32(0)), False), (t, True), (np.nextafter(t, np.float32(2)), True)):
            (r,), (c,) = np.nonzero(case.det == v)
            assert ((r, c) in kept) == want, f"pixel ({r}, {c}) = {float(v)!r} at thr {case.thr}"


def test_stack_equals_its_tiles_alone():
    ctx, tiles = stack_ctx(128)
    ctx.naive_init(nc.STACK_THR, nc.STACK_NMS)
    pops = [len(nc.expected(c).centers) for c in tiles]
    print(f"\nstack: populations {ctx.counts().tolist()}, expected {pops}")
    assert ctx.counts().tolist() == pops
    batch = ctx.get_points_all()
    for t, case in enumerate(tiles):
        assert_points(ctx.get_points(t), nc.expected(case))
        single = case_ctx(case, 128)
        single.naive_init(nc.STACK_THR, nc.STACK_NMS)
        sxy, sm = single.get_points()
        np.testing.assert_array_equal(batch[t][0], sxy)
        assert batch[t][1].tobytes() == sm.tobytes()


def _chain(ctx, tiles, steps=300):
    ctx.set_kernels(kernels.make_kernels(make_mappings(tiles[0].mapping), 10.0))
    ctx.set_schedule(1.0, 0.998, 0.0)
    ctx.run(steps, seed=7)
    return [(xy.tobytes(), m.tobytes()) for xy, m in ctx.get_points_all()], [ctx.step_index(t) for t in range(len(tiles))]


def test_capacity_overflow_is_reported_and_not_sticky():
    """a tile that keeps more than point_capacity centres: -12 naming the tile, the first point_capacity picks stored; the
    next naive_init on the same context, at a threshold whose survivors fit, succeeds, and a chain from it is the chain of a
    fresh context (the kernel's guarded path only: nothing is written past the capacity)"""
    ctx, tiles = stack_ctx(CAPACITY)
    pops = [len(nc.expected(c).centers) for c in tiles]
    over = [t for t, p in enumerate(pops) if p > CAPACITY]
    assert over == [3]
    with pytest.raises(hip_api.MppError) as err:
        ctx.naive_init(nc.STACK_THR, nc.STACK_NMS)
    assert err.value.code == -12 and "tile 3" in str(err.value), str(err.value)
    assert ctx.counts().tolist() == [min(p, CAPACITY) for p in pops]
    for t, case in enumerate(tiles):
        assert_points(ctx.get_points(t), nc.expected(case), min(pops[t], CAPACITY))
    # the same context again, at a threshold that fits
    refit = [nc.expected(c, REFIT_THR) for c in tiles]
    print(f"\ncapacity {CAPACITY}: populations {pops} at thr {nc.STACK_THR}, {[len(e.centers) for e in refit]} at thr {REFIT_THR}")
    ctx.naive_init(REFIT_THR, nc.STACK_NMS)
    assert ctx.counts().tolist() == [len(e.centers) for e in refit]
    for t, e in enumerate(refit):
        assert_points(ctx.get_points(t), e)
    # ... and a chain from it equals the chain of a context that never overflowed
    fresh, _ = stack_ctx(CAPACITY)
    fresh.naive_init(REFIT_THR, nc.STACK_NMS)
    got, want = _chain(ctx, tiles), _chain(fresh, tiles)
    assert want[1] == [300] * len(tiles)
    assert got == want
