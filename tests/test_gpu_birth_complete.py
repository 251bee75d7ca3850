"""Greedy completion (``mpp_select_minima``, ``mpp_birth_complete``, ``csrc/mpp_birth_complete.hip``).

The standard is the host walk of ``birth_complete_ref``: ``birth_energy_map(marks=True)`` -> numpy selection ->
``set_points(old + new)``, repeated -- calls that existed before the device loop.  The device loop has to give the same points,
marks, counts and the same bits of ``gain``; it is compared with itself only where the claim is that two launch shapes agree.

The energy bound of ``assert_energy_drop`` (derived, not measured).  Write u = 2^-53 and g(m) = (m - 1) u / (1 - (m - 1) u): a
recursive float64 sum of m terms, in any order, differs from the exact sum of the same terms by at most g(m) * sum |t_i|.
The point energies e(v | X) are the same bits wherever they are formed (the map's pre-pass runs the code of
``mpp_total_energy``, and the pair reductions are max / min, so adding a candidate to cached reductions IS the from-scratch
reduction); two births of one round lie further apart than 2 * max_inter, so no point's energy sees both.  Hence, with exact
sums, E(after) - E(before) is the sum over the appended points c of D_c, the exact sum of the terms the map added for c.  What
is computed differs by
  * the two from-scratch totals: at most n_after terms of magnitude at most B1 each: 2 g(n_after) n_after B1;
  * per appended point the map's own sum of m_c = n_c + 1 terms (n_c the chain's count when c was evaluated), bounded by the
    map-vs-delta_batch bound ``order_bound(n_c)`` of ``test_gpu_birth_map`` (2 g(m_c) m_c 2 B1, twice what one order needs);
  * the sequential sum of the k values into ``gain``: g(k + 1) * sum |dE_c|;
  * the subtraction and the comparison: 2 u |gain|.
B1 is 1 under the logistic combinator and ``point_energy_bound`` under the linear one.

Small on purpose: tiles of 40 x 48 to 96 x 96 pixels, one 130-wide map, at most 2 000 chain steps."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from birth_complete_ref import host_walk, numpy_summary, select_minima_ref
from helpers import GOLDEN, REPO, contrast_model
from mpp_cnn_rs_object_detection_amd import energies as E
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings, synth
from mpp_cnn_rs_object_detection_amd.custom_types import ImageWMaps
from mpp_cnn_rs_object_detection_amd.point_set import EPointsSet
from mpp_cnn_rs_object_detection_amd.shapes import Rectangle
from test_gpu_birth_map import (H, MAX_INTER, POINT_MARKS, POINTS, U, W, make_ctx, model_desc, order_bound, point_energy_bound,
                                tile_maps)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
MODELS = ["mpp_hrcM", "mpp_log"]
NO_POINTS = (np.zeros((0, 2), np.int32), np.zeros((0, 3)))


# ---- selection alone ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bare_ctx():
    ctx = hip_api.MppContext(0)
    yield ctx
    ctx.close()


def device_select(ctx, d, below, distance, ld=None):
    import torch
    h, w = d.shape
    if ld is None:
        t = torch.from_numpy(np.ascontiguousarray(d)).to("cuda:0")
    else:
        wide = torch.full((h, ld), -1e9, dtype=torch.float64, device="cuda:0")       # (what lies beyond W would be a candidate)
        wide[:, :w] = torch.from_numpy(np.ascontiguousarray(d)).to("cuda:0")
        t = wide[:, :w]
    xy, v, n = ctx.select_minima(t, below, distance)
    return xy.cpu().numpy(), v.cpu().numpy(), n


def assert_selection(ctx, d, below, distance, what, ld=None):
    want = select_minima_ref(d, below, distance)
    got = device_select(ctx, d, below, distance, ld)
    print(f"{what}: {d.shape[0]} x {d.shape[1]}, {want[2]} candidates, {len(want[0])} kept")
    assert got[2] == want[2], what
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    np.testing.assert_array_equal(got[1], want[1], err_msg=what)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    return want


def test_selection_on_hand_made_maps(bare_ctx):
    ctx = bare_ctx
    # the distance edge at the completion's own distance, 2 * max_inter = 64, on a 130-wide map
    d = np.zeros((150, 130))
    d[5, 3], d[5, 67] = -1.0, -2.0                                   # exactly 64 apart: only the better one
    d[140, 60], d[141, 124] = -3.0, -4.0                             # (1, 64): d^2 = 64^2 + 1: both
    xy, _, n = assert_selection(ctx, d, 0.0, 64.0, "distance edge")
    assert n == 4 and xy.tolist() == [[5, 67], [140, 60], [141, 124]]
    d = np.zeros((30, 30))
    d[2, 3], d[5, 7], d[20, 3], d[21, 8] = -1.0, -2.0, -1.0, -2.0    # (3, 4) = 5 apart; (1, 5): 26 = 5^2 + 1
    assert assert_selection(ctx, d, 0.0, 5.0, "distance edge, small")[0].tolist() == [[5, 7], [20, 3], [21, 8]]
    # equal values tie toward the smaller index; a NaN is never a candidate, -inf is one
    d = np.zeros((13, 37))                                           # (neither side a multiple of a block's span)
    d[4, 4], d[4, 6], d[1, 1] = -1.0, -1.0, -1.0
    d[8, 30], d[8, 31], d[9, 30] = NAN, -INF, -INF
    d[12, 36], d[0, 36] = -0.5, NAN
    xy, v, n = assert_selection(ctx, d, 0.0, 2.0, "ties, NaN, -inf")
    assert xy.tolist() == [[1, 1], [4, 4], [8, 31], [12, 36]] and n == 6 and v[2] == -INF
    assert_selection(ctx, d, -0.75, 2.0, "a level below 0")
    assert_selection(ctx, d, 0.0, 2.0, "ld > W", ld=41)
    assert_selection(ctx, d, 0.0, 0.0, "distance 0: every candidate stands alone")
    # order-free, not a walk: b loses to a and c to b although a does not reach c
    d = np.zeros((3, 9))
    d[1, 0], d[1, 2], d[1, 4] = -3.0, -2.0, -1.0
    assert assert_selection(ctx, d, 0.0, 2.0, "a chain of three")[0].tolist() == [[1, 0]]
    xy, v, n = assert_selection(ctx, np.ones((7, 5)), 0.0, 3.0, "no candidate")
    assert n == 0 and xy.shape == (0, 2) and v.shape == (0,)
    assert assert_selection(ctx, np.full((1, 1), -1.0), 0.0, 3.0, "one pixel")[0].tolist() == [[0, 0]]


def test_selection_with_every_pixel_a_candidate(bare_ctx):
    """9 216 equal candidates: the list is longer than any workgroup's LDS could hold, and exactly one pixel is kept"""
    d = np.full((96, 96), -1.0)
    xy, v, n = assert_selection(bare_ctx, d, 0.0, 136.0, "all equal")               # (the diagonal is 134.4)
    assert n == 96 * 96 and xy.tolist() == [[0, 0]] and v.tolist() == [-1.0]
    xy, _, n = device_select(bare_ctx, d, 0.0, 0.0)                                  # ... and every one of them with distance 0
    assert n == len(xy) == 96 * 96 and xy[:, 0].tolist() == np.repeat(np.arange(96), 96).tolist()
    assert xy[:, 1].tolist() == np.tile(np.arange(96), 96).tolist()


def test_selection_on_a_random_map(bare_ctx):
    rng = np.random.default_rng(12)
    d = np.round(rng.normal(0.0, 1.0, (96, 96)), 2)                  # (rounded: equal values occur)
    below = float(np.quantile(d, 0.22))
    want = assert_selection(bare_ctx, d, below, 3.0, "random")
    assert 1800 <= want[2] <= 2300 and len(want[0]) > 100
    assert_selection(bare_ctx, d, below, 64.0, "random, wide")


def test_selection_output_too_small_and_bad_arguments(bare_ctx):
    import torch
    ctx = bare_ctx
    d = np.zeros((20, 30))
    for k in range(5):
        d[4 * k, 5 * k] = -1.0 - k
    want = select_minima_ref(d, 0.0, 3.0)
    assert len(want[0]) == 5
    t = torch.from_numpy(d).to("cuda:0")
    nc, nk = C.c_int64(-7), C.c_int64(-7)

    def call(h, w, ld, below, distance, cap):
        xy = torch.full((max(cap, 1), 2), -5, dtype=torch.int32, device="cuda:0")
        v = torch.full((max(cap, 1),), -5.0, dtype=torch.float64, device="cuda:0")
        rc = ctx._L.mpp_select_minima(ctx._h, h, w, ld, hip_api._ptr(t), below, distance, cap, hip_api._ptr(xy), hip_api._ptr(v),
                                      C.byref(nc), C.byref(nk))
        ctx.synchronize()
        return rc, xy.cpu().numpy(), v.cpu().numpy()
    rc, xy, v = call(20, 30, 30, 0.0, 3.0, 4)                        # one too small
    assert rc == -13 and nk.value == 5 and nc.value == 5 and np.all(xy == -5) and np.all(v == -5.0)
    rc, xy, v = call(20, 30, 30, 0.0, 3.0, 5)
    assert rc == 0 and xy.tolist() == want[0].tolist() and v.tolist() == want[1].tolist()
    for args in [(20, 30, 30, 0.0, -1.0, 8), (20, 30, 30, 0.0, NAN, 8), (20, 30, 30, 0.0, INF, 8), (20, 30, 30, NAN, 3.0, 8),
                 (20, 30, 30, -INF, 3.0, 8), (20, 30, 29, 0.0, 3.0, 8), (65536, 32768, 32768, 0.0, 3.0, 8), (0, 30, 30, 0.0, 3.0, 8)]:
        rc, xy, v = call(*args)
        assert rc == -1 and np.all(xy == -5), args


# ---- the starting states ------------------------------------------------------------------------------------------------------

def tile_96():
    gt_xy, gt_marks = synth.make_gt(96, 20, tile_id=31)
    return tile_maps((96, 96), seed=9, gt_xy=gt_xy, gt_marks=gt_marks)


def contexts(kind, name, **options):
    """(desc, det, device ctx, walk ctx) with the same starting state in both contexts"""
    setup, _, desc = model_desc(name)
    if kind == "a":                                   # nothing on a 96 x 96 tile with 20 objects: a greedy detector
        det, marks = tile_96()
        pair = [make_ctx(desc, det, marks, **options) for _ in range(2)]
    elif kind == "b":                                 # the 12 points of the birth-map test on 40 x 48
        det, marks = tile_maps()
        pair = [make_ctx(desc, det, marks, **options) for _ in range(2)]
        for c in pair:
            c.set_points(0, POINTS, POINT_MARKS)
    else:                                             # the written-back state of a run of 2 000 steps
        t = synth.make_tile(64, 12, tile_id=52, noise=0.2)
        det, marks = t.det, t.marks
        ctx = make_ctx(desc, det, marks, point_capacity=256, spec_waves=8)
        ctx.naive_init(setup.detection_threshold, 6.0)
        n0 = ctx.count(0)
        ctx.set_kernels(kernels.make_kernels(mappings.default_mappings(), 1.0), intensity=[float(max(1, n0))])
        ctx.set_schedule(0.1, 0.999, 0.0)
        ctx.run(2000, seed=17)
        xy, mk = ctx.get_points(0)
        walk = make_ctx(desc, det, marks, point_capacity=256)
        walk.set_points(0, xy, mk)
        pair = [ctx, walk]
    return desc, det, pair[0], pair[1]


def report_tuple(r):
    return (float(r["min_dE"]), int(r["x"]), int(r["y"]), int(r["n_negative"]), int(r["n_nan"]))


def assert_equals_walk(ctx, chain, rep, walk, what):
    xy, mk = ctx.get_points(chain)
    print(f"{what}: status {walk['status']}, {walk['rounds']} round(s), +{walk['n_added']} -> {walk['n_after']} points, "
          f"gain {walk['gain']!r}, summary {walk['summary']}")
    np.testing.assert_array_equal(xy, walk["xy"], err_msg=what)                      # equal, not close
    np.testing.assert_array_equal(mk, walk["marks"], err_msg=what)
    assert (int(rep["status"]), int(rep["rounds"]), int(rep["n_added"]), int(rep["n_after"])) == \
        (walk["status"], walk["rounds"], walk["n_added"], walk["n_after"]), what
    assert float(rep["gain"]) == walk["gain"], (what, float(rep["gain"]), walk["gain"])     # the same bits
    assert report_tuple(rep) == walk["summary"], what


def assert_rounds_are_sparse(walk):
    """within a round the appended points lie pairwise further apart than 2 * max_inter"""
    for kxy, _ in walk["per_round"]:
        p = kxy.astype(np.int64)
        d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        d2[np.arange(len(p)), np.arange(len(p))] = 1 << 40
        assert len(p) >= 1 and d2.min() > (2 * MAX_INTER) ** 2


def assert_energy_drop(desc, det, e_before, e_after, n_before, walk, what):
    """E(after) - E(before) against the gain, within the bound derived in the module's docstring"""
    g = lambda m: (m - 1) * U / (1.0 - (m - 1) * U) if m > 1 else 0.0
    B1 = 1.0 if desc.combinator == E.C_LOGISTIC else point_energy_bound(desc, det, walk["marks"] if len(walk["marks"]) else None)
    n_after, bound, n, k, mag = walk["n_after"], 0.0, n_before, 0, 0.0
    bound += 2.0 * g(n_after) * n_after * B1
    for kxy, kv in walk["per_round"]:
        bound += len(kxy) * order_bound(n, desc, det, walk["marks"])
        n, k, mag = n + len(kxy), k + len(kxy), mag + float(np.abs(kv).sum())
    bound += g(k + 1) * mag + 2.0 * U * abs(walk["gain"])
    err = abs((e_after - e_before) - walk["gain"])
    print(f"{what}: E {e_before!r} -> {e_after!r}, gain {walk['gain']!r}, |difference| {err!r}, bound {bound!r}")
    assert np.isfinite(e_before) and np.isfinite(e_after) and err <= bound, (what, err, bound)


# ---- completion equals the host walk --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_completion_equals_the_host_walk(kind, name):
    desc, det, ctx, ref = contexts(kind, name)
    n_before = ctx.count(0)
    e_before = float(ctx.total_energy_all()[0])
    first = ref.birth_energy_map()[0][0].cpu().numpy()
    # (births of one round lie more than 64 px apart: the 96 x 96 tile takes few per round and more rounds than the default 16)
    rounds = 64 if kind == "a" else 16
    walk = host_walk(ref, 0, MAX_INTER, max_rounds=rounds)
    rep = ctx.birth_complete(max_rounds=rounds)
    assert len(rep) == 1 and rep.dtype == hip_api.COMPLETE_REPORT_DTYPE
    what = f"state ({kind}), {name}"
    assert_equals_walk(ctx, 0, rep[0], walk, what)
    # what the input has to exercise, asserted on the walk's values
    assert walk["status"] == 0
    if kind == "a":
        assert walk["n_added"] >= 5 and walk["rounds"] >= 2
    else:
        assert np.any(first < 0) and walk["n_added"] >= 1
    if kind == "b":                                   # the tile's diagonal is below 2 * max_inter: one birth per round
        assert (H - 1) ** 2 + (W - 1) ** 2 < (2 * MAX_INTER) ** 2 and all(len(k) == 1 for k, _ in walk["per_round"])
    # invariants that do not lean on the walk
    fresh, _, s = ctx.birth_energy_map()
    assert int(s[0]["n_negative"]) == 0 and int(rep[0]["n_negative"]) == 0 and not bool((fresh < 0).any())
    assert_rounds_are_sparse(walk)
    assert_energy_drop(desc, det, e_before, float(ctx.total_energy_all()[0]), n_before, walk, what)
    ctx.close()
    ref.close()


@pytest.mark.parametrize("name", MODELS)
def test_min_gain_leaves_nothing_below_it(name):
    desc, det, ctx, ref = contexts("b", name)
    first = ref.birth_energy_map()[0][0].cpu().numpy()
    g = float(-0.5 * np.nanmin(first))                               # half the deepest pixel: it still qualifies
    assert g > 0
    walk = host_walk(ref, 0, MAX_INTER, min_gain=g)
    rep = ctx.birth_complete(min_gain=g)
    assert_equals_walk(ctx, 0, rep[0], walk, f"min_gain {g!r}, {name}")
    assert walk["status"] == 0 and walk["n_added"] >= 1
    fresh = ctx.birth_energy_map()[0][0].cpu().numpy()
    assert not np.any(fresh < -g)
    assert int(rep[0]["n_negative"]) == int(np.sum(fresh < 0))       # (the summary still counts below 0, not below -g)
    ctx.close()
    ref.close()


def test_max_rounds_1_reports_the_returned_state():
    desc, det, ctx, ref = contexts("a", "mpp_log")
    walk = host_walk(ref, 0, MAX_INTER, max_rounds=1)
    rep = ctx.birth_complete(max_rounds=1)
    assert walk["status"] == 1 and walk["rounds"] == 1
    assert_equals_walk(ctx, 0, rep[0], walk, "max_rounds 1")
    fresh, _, s = ctx.birth_energy_map()
    assert report_tuple(rep[0]) == report_tuple(s[0]) == numpy_summary(fresh[0].cpu().numpy())
    assert int(s[0]["n_negative"]) > 0                               # (one round does not finish this tile)
    ctx.close()
    ref.close()


# ---- the append leaves a complete state -----------------------------------------------------------------------------------------

def test_a_run_after_the_completion_equals_a_run_after_set_points():
    setup, _, desc = model_desc("mpp_log")
    det, marks = tile_96()
    kd = kernels.make_kernels(mappings.default_mappings(), 1.0)

    def fresh():
        ctx = make_ctx(desc, det, marks, point_capacity=256, spec_waves=8)
        ctx.set_kernels(kd, intensity=[8.0])
        ctx.set_schedule(0.1, 0.999, 0.0)
        return ctx
    a = fresh()
    rep = a.birth_complete()
    xy, mk = a.get_points(0)
    assert int(rep[0]["n_added"]) == len(xy) >= 5
    e = a.total_energy_all()
    b = fresh()
    b.set_points(0, xy, mk)
    assert b.total_energy_all().tolist() == e.tolist()
    a.run(500, seed=23)
    b.run(500, seed=23)
    xa, ma = a.get_points(0)
    xb, mb = b.get_points(0)
    assert xa.tolist() != xy.tolist() or ma.tolist() != mk.tolist()                  # (the run did something)
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(ma, mb)
    assert a.step_index(0) == b.step_index(0) == 500
    a.close()
    b.close()


# ---- crossing the grid threshold ------------------------------------------------------------------------------------------------

def test_the_grid_threshold_is_crossed_between_rounds():
    _, _, desc = model_desc("mpp_log")
    det, marks = tile_96()
    rng = np.random.default_rng(4)
    pix = rng.permutation(16 * 16)[:250]                             # 250 points crowded into the 16 x 16 corner
    xy0 = np.stack([pix // 16, pix % 16], axis=1).astype(np.int32)
    mk0 = np.stack([rng.uniform(4.0, 9.0, 250), rng.uniform(0.3, 0.9, 250), rng.uniform(0.0, np.pi, 250)], axis=1)
    ctxs = [make_ctx(desc, det, marks) for _ in range(3)]
    for c in ctxs:
        assert c.get_option("scratch_grid_min_points") == 256
        c.set_points(0, xy0, mk0)
    grid, scan, ref = ctxs
    scan.set_option("scratch_grid_min_points", 0)
    walk = host_walk(ref, 0, MAX_INTER)
    assert walk["n_added"] > 6 and walk["rounds"] >= 2                # 250 + more than 6: the last rounds run on >= 256 points
    n, crossing = 250, []
    for kxy, _ in walk["per_round"]:
        crossing.append(n >= 256)                                    # this round's pre-pass took its neighbours from the grid
        n += len(kxy)
    assert crossing[0] is False and n >= 256
    rep = grid.birth_complete()
    assert grid.get_option("birth_map_grid") == 1
    assert_equals_walk(grid, 0, rep[0], walk, "across 256 points, grid")
    rep0 = scan.birth_complete()
    assert scan.get_option("birth_map_grid") == 0
    assert_equals_walk(scan, 0, rep0[0], walk, "across 256 points, scan")
    assert rep0[0] == rep[0]
    for c in ctxs:
        c.close()


# ---- capacity ---------------------------------------------------------------------------------------------------------------------

def capacity_contexts(cap):
    """two chains on the 40 x 48 tile: chain 0 holds the 12 points, chain 1 nothing"""
    _, _, desc = model_desc("mpp_hrcM")
    det, marks = tile_maps()
    ctx = make_ctx(desc, det, marks, point_capacity=cap, replicas=2)
    ctx.set_points(0, POINTS, POINT_MARKS)
    return desc, det, marks, ctx


def test_capacity():
    desc, det, marks, big = capacity_contexts(64)
    free = host_walk(big, 0, MAX_INTER)                              # what chain 0 would do with room
    other = host_walk(big, 1, MAX_INTER)                             # ... and the empty chain 1
    big.close()
    k1 = len(free["per_round"][0][0])
    assert free["rounds"] >= 2 and k1 == 1 and 1 <= other["n_after"] <= len(POINTS)
    # exactly n + k of the first round: the round fits, the second one does not
    _, _, _, ctx = capacity_contexts(len(POINTS) + k1)
    rep = ctx.birth_complete()
    xy, mk = ctx.get_points(0)
    assert (int(rep[0]["status"]), int(rep[0]["rounds"]), int(rep[0]["n_added"]), int(rep[0]["n_after"])) == (2, 1, 1, 13)
    np.testing.assert_array_equal(xy, free["xy"][:13])
    np.testing.assert_array_equal(mk, free["marks"][:13])
    assert float(rep[0]["gain"]) == float(free["per_round"][0][1][0])
    assert report_tuple(rep[0]) == report_tuple(ctx.birth_energy_map()[2][0])
    ctx.close()
    # one less: nothing of the round is appended to chain 0, chain 1 completes
    _, _, _, ctx = capacity_contexts(len(POINTS))
    ref = capacity_contexts(len(POINTS))[3]
    walk0, walk1 = host_walk(ref, 0, MAX_INTER), host_walk(ref, 1, MAX_INTER)
    assert walk0["status"] == 2 and walk0["n_added"] == 0 and walk1["status"] == 0
    rep = ctx.birth_complete()
    assert_equals_walk(ctx, 0, rep[0], walk0, "capacity, the full chain")
    assert_equals_walk(ctx, 1, rep[1], walk1, "capacity, the other chain")
    np.testing.assert_array_equal(ctx.get_points(0)[0], POINTS)
    np.testing.assert_array_equal(walk1["xy"], other["xy"])
    ctx.close()
    ref.close()
    # the point set on the same input: it moves to a larger context and finishes as the unbounded walk does
    setup, comb, _ = model_desc("mpp_hrcM")
    data = ImageWMaps(name="0", shape=(H, W), image=None, detection_map=det, param_dist_maps=marks,
                      mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS, gt_config=[])
    unit, pair = setup.make_energies(data)
    pts = [Rectangle(int(x), int(y), size=float(m[0]), ratio=float(m[1]), angle=float(m[2])) for (x, y), m in zip(POINTS, POINT_MARKS)]
    ps = EPointsSet(pts, (H, W), unit, pair, image_data=data, point_capacity=len(POINTS))
    out = ps.birth_complete(energy_combinator=comb)
    assert ps._ctx.get_option("point_capacity") > len(POINTS)
    rows = [(p.x, p.y, p.size, p.ratio, p.angle) for p in ps]
    assert rows == [tuple(r) for r in np.concatenate([free["xy"], free["marks"]], axis=1).tolist()]
    assert all(a is b for a, b in zip(list(ps)[:len(pts)], pts))                     # the old objects stay, in place
    assert (out["status"], out["rounds"], out["n_added"], out["n_after"]) == (0, free["rounds"], free["n_added"], free["n_after"])
    assert out["gain"] == free["gain"]
    assert (out["min_dE"], out["argmin"][0], out["argmin"][1], out["n_negative"], out["n_nan"]) == free["summary"]
    assert len(ps) == free["n_after"]


# ---- launch-shape independence --------------------------------------------------------------------------------------------------

def test_a_chain_does_not_depend_on_tiles_and_replicas():
    _, _, desc = model_desc("mpp_hrcM")
    maps3 = [tile_maps(seed=20 + k) for k in range(3)]
    det = np.stack([m[0] for m in maps3])
    marks = [np.stack([m[1][k] for m in maps3]) for k in range(3)]
    configs = [NO_POINTS, (POINTS[8:9], POINT_MARKS[8:9]), (POINTS, POINT_MARKS)]
    ctx = make_ctx(desc, det, marks, replicas=2)
    assert ctx.get_option("n_chains") == 6
    for c in range(6):
        ctx.set_points(c, *configs[c % 3])
    rep = ctx.birth_complete()
    state = ctx.get_points_all()
    assert len(rep) == 6 and len(set(int(r["rounds"]) for r in rep)) > 1               # (the chains finish in different rounds)
    for c in range(6):
        one = make_ctx(desc, maps3[c % 3][0], maps3[c % 3][1])
        one.set_points(0, *configs[c % 3])
        r1 = one.birth_complete()
        xy, mk = one.get_points(0)
        assert r1[0] == rep[c], (c, r1[0], rep[c])                                    # every field, bit for bit
        np.testing.assert_array_equal(state[c][0], xy)
        np.testing.assert_array_equal(state[c][1], mk)
        one.close()
    ctx.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals():
    z = np.load(os.path.join(GOLDEN, "tape_contrast_96.npz"), allow_pickle=False)
    _, _, cdesc, image = contrast_model(z)
    shape = tuple(int(v) for v in z["shape"])
    ctx = hip_api.MppContext(0)
    with pytest.raises(hip_api.MppError):                            # before set_maps
        ctx.birth_complete()
    ctx.set_maps(np.zeros(shape, np.float32), [np.zeros(shape + (32,), np.float32)] * 3)
    with pytest.raises(hip_api.MppError):                            # before set_model
        ctx.birth_complete()
    ctx.set_image(image)
    ctx.set_model(cdesc, mappings.default_mappings())
    with pytest.raises(hip_api.MppError, match="classic"):
        ctx.birth_complete()
    ctx.close()
    _, _, desc = model_desc("mpp_log")
    det, marks = tile_maps()
    ctx = make_ctx(desc, det, marks)
    ctx.set_points(0, POINTS, POINT_MARKS)
    for bad in (0, -1, 1025):
        with pytest.raises(hip_api.MppError, match="max_rounds"):
            ctx.birth_complete(max_rounds=bad)
    for bad in (-0.5, NAN, INF):
        with pytest.raises(hip_api.MppError, match="min_gain"):
            ctx.birth_complete(min_gain=bad)
    np.testing.assert_array_equal(ctx.get_points(0)[0], POINTS)      # a refused call changes nothing
    import torch
    for bad in (torch.zeros((4, 4), dtype=torch.float32, device="cuda:0"), torch.zeros((4, 4), dtype=torch.float64),
                torch.zeros((4, 8), dtype=torch.float64, device="cuda:0")[:, ::2], torch.zeros((2, 4, 4), dtype=torch.float64, device="cuda:0")):
        with pytest.raises(ValueError):
            ctx.select_minima(bad, 0.0, 1.0)
    ctx.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def test_infer_image_with_and_without_the_completion():
    from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel
    cfg = json.load(open(os.path.join(REPO, "model_configs", "mpp", "mpp_hrcM.json")))
    cfg["inference"]["rjmcmc_params"]["burn_in"] = 4000
    cwd = os.getcwd()
    os.chdir(REPO)
    try:
        model = MPPModel(cfg, phase="val", load=True)
    finally:
        os.chdir(cwd)
    gt_xy, gt_marks = synth.make_gt(300, 60, tile_id=61)
    det, marks = synth.render_maps((300, 400), gt_xy, gt_marks)
    data = ImageWMaps(name="0001", shape=(300, 400), image=None, detection_map=det, param_dist_maps=marks,
                      mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS, gt_config=[])
    rows = lambda pts: [(p.x, p.y, p.size, p.ratio, p.angle) for p in pts]
    assert "birth_complete" not in cfg["inference"]
    off, s_off = model.infer_image(data, seed=5)
    assert getattr(model, "last_complete", None) is None
    again, s_again = model.infer_image(data, seed=5)                                 # off: the rows and scores of before
    assert rows(again) == rows(off) and np.asarray(s_again).tolist() == np.asarray(s_off).tolist()
    model.config["inference"]["birth_complete"] = {"max_rounds": 256}                # (the default 16 rounds do not finish this image)
    on, s_on = model.infer_image(data, seed=5)
    summary = model.last_complete
    assert set(summary) == {"n_added", "rounds", "gain", "status", "min_dE", "argmin", "n_negative", "n_nan"}
    n = len(rows(off))
    assert n > 3 and rows(on)[:n] == rows(off) and len(s_on) == len(rows(on)) == n + summary["n_added"]
    # the walk from the detections of the run without it, on the image as one tile
    # (with the model's own terms and stored combinator: the manual weights of ``model_desc`` differ from them in the last bits)
    desc = E.build_model_desc(*model.energy_setup.make_energies(data), model.energy_model)
    ref = make_ctx(desc, det, marks, point_capacity=max(1024, 2 * n + 64))
    ref.set_points(0, np.array([r[:2] for r in rows(off)], np.int32).reshape(-1, 2), np.array([r[2:] for r in rows(off)]).reshape(-1, 3))
    walk = host_walk(ref, 0, MAX_INTER, max_rounds=256)
    print(f"infer_image: {n} detections, walk +{walk['n_added']} in {walk['rounds']} round(s), gain {walk['gain']!r}")
    assert walk["n_added"] >= 1                                                      # (the chain of 4 000 steps leaves objects out)
    assert rows(on)[n:] == [tuple(r) for r in np.concatenate([walk["xy"], walk["marks"]], axis=1)[n:].tolist()]
    assert (summary["n_added"], summary["rounds"], summary["status"], summary["gain"]) == \
        (walk["n_added"], walk["rounds"], walk["status"], walk["gain"])
    assert (summary["min_dE"], summary["argmin"][0], summary["argmin"][1], summary["n_negative"], summary["n_nan"]) == walk["summary"]
    # every point is scored in the completed configuration: the scores are those of a set built from the rows
    np.testing.assert_array_equal(np.asarray(s_on), np.exp(-ref.papangelou(0)))
    _, s2 = model.birth_map(data, on)                                                # a map computed afterwards
    assert s2["n_negative"] == summary["n_negative"] == 0 and s2["min_dE"] == summary["min_dE"]
    # with the birth map on too, its map is that of the completed configuration
    model.config["inference"]["birth_map"] = True
    both, _ = model.infer_image(data, seed=5)
    assert rows(both) == rows(on) and model.last_birth[1] == s2
    model.config["inference"]["birth_map"] = False
    model.config["inference"]["birth_complete"] = False
    ref.close()


def test_main_infer_with_the_completion_flag(tmp_path):
    """``main.py -p infer --birth-complete`` on the synthetic dataset of ``test_gpu_detect.py``: the key in the pickle, the log
    line; without the flag the key is absent"""
    import pickle
    import shutil
    import subprocess
    import sys
    from test_gpu_detect import write_image
    root = tmp_path
    for d in ("model_configs", "models_storage"):
        shutil.copytree(os.path.join(REPO, d), root / d)
    with open(root / "paths_config.json", "w") as f:
        json.dump({"dataset_path": ["data/"], "model_path": ["models_storage/"]}, f)
    write_image(root, "val", 7, 21)
    cfg = json.load(open(root / "model_configs" / "mpp" / "mpp_hrcM.json"))
    cfg["inference"]["rjmcmc_params"]["burn_in"] = 2000
    with open(root / "cfg.json", "w") as f:
        json.dump(cfg, f)
    out = root / "data" / "inference" / "SYNTH" / "val" / "mpp_hrcM"
    records = {}
    for flag in ([], ["--birth-complete"]):
        r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "-p", "infer", "-m", "mpp", "-c", str(root / "cfg.json"),
                            "-d", "SYNTH", "-o"] + flag, cwd=root, env=dict(os.environ, PYTHONPATH=REPO),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(out / "0007_results.pkl", "rb") as f:
            records[bool(flag)] = (pickle.load(f), r.stderr + r.stdout)
    rec, log = records[False]
    assert "birth_complete" not in rec and "birth completion" not in log
    rec_on, log = records[True]
    s = rec_on["birth_complete"]
    assert set(s) == {"n_added", "rounds", "gain", "status", "min_dE", "argmin", "n_negative", "n_nan"}
    assert len(rec_on["detection_points"]) == len(rec["detection_points"]) + s["n_added"] == len(rec_on["detection_score"])
    assert rec_on["detection_points"][:len(rec["detection_points"])] == rec["detection_points"]
    # (the flag runs the default 16 rounds: converged with nothing left below 0, or stopped at the limit)
    assert (s["status"] == 0 and s["n_negative"] == 0) or (s["status"] == 1 and s["rounds"] == 16)
    assert (s["n_added"] > 0) == (s["gain"] < 0) and s["n_added"] >= s["rounds"]
    line = (f"birth completion: +{s['n_added']} object(s) in {s['rounds']} round(s), energy -{abs(s['gain']):.2f}, "
            f"{s['n_negative']} pixel(s) still below 0")
    assert line in log
