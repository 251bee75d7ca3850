"""Local descent (``mpp_papangelou_all``, ``mpp_select_points``, ``mpp_descend``, ``csrc/mpp_descent.hip``).

The standard is the host walk of ``descent_ref``: ``papangelou`` -> the double loop's selection -> ``set_points(survivors)``
and ``birth_energy_map(marks=True)`` -> ``select_minima_ref`` -> ``set_points(old + new)``, repeated -- calls that existed
before the device loop.  The device loop has to give the same points, marks, ``src``, counts and the same bits of both gains;
it is compared with itself only where the claim is that two launch shapes agree.

The energy bound of ``assert_energy_identity`` (derived, not measured).  Write u = 2^-53 and g(m) = (m - 1) u / (1 - (m - 1) u):
a recursive float64 sum of m terms, in any order, differs from the exact sum of the same terms by at most g(m) * sum |t_i|.
The point energies e(v | X) are the same bits wherever they are formed (every path runs the code of ``mpp_total_energy``, and
the pair reductions are max / min, so a reduction with one point left out or one added IS the from-scratch reduction of that
configuration).  Two points removed in one round, and two appended in one round, lie further apart than 2 * max_inter, so no
point's energy sees both.  Hence, with exact sums, E(after) - E(before) is the sum over the appended points c of D_c minus
the sum over the removed points v of P_v, where D_c is the exact sum of the terms the map added for c and P_v the exact sum
of the terms the Papangelou kernel added for v.  What is computed differs by
  * the two from-scratch totals, n_before and n_after terms of magnitude at most B1 each:
    g(n_before) n_before B1 + g(n_after) n_after B1;
  * per appended point the map's own sum of m_c = n_c + 1 terms (n_c the chain's count when c was evaluated), bounded by the
    map-vs-delta_batch bound ``order_bound(n_c)`` of ``test_gpu_birth_map`` (2 g(m_c) m_c 2 B1, twice what one order needs);
  * per removed point the Papangelou kernel's sum -- the point's own energy and one difference e(w | X - v) - e(w | X) per
    neighbour w, at most n_v terms (n_v the chain's count when v was evaluated) of magnitude at most 2 B1, added per lane and
    then in a tree: g(n_v) n_v 2 B1;
  * the sequential sums of the k_b appended values and the k_d removed values into the two gains:
    g(k_b + 1) sum |dE_c| + g(k_d + 1) sum |p_v|;
  * the two subtractions and the comparison: 2 u (|E(after) - E(before)| + |gain_births - gain_deaths|).
B1 is 1 under the logistic combinator and ``point_energy_bound`` under the linear one.

Small on purpose: tiles of 40 x 48 to 96 x 96 pixels, at most 2 000 chain steps."""
import ctypes as C
import json
import logging
import os
import pickle

import numpy as np
import pytest

from birth_complete_ref import numpy_summary
from descent_ref import NO_MAP, host_walk, papangelou_summary, select_points_ref, state_d
from helpers import GOLDEN, REPO, contrast_model
from mpp_cnn_rs_object_detection_amd import energies as E
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings, synth
from mpp_cnn_rs_object_detection_amd.custom_types import ImageWMaps
from mpp_cnn_rs_object_detection_amd.point_set import EPointsSet
from mpp_cnn_rs_object_detection_amd.shapes import Rectangle
from test_gpu_birth_complete import NO_POINTS, contexts, report_tuple
from test_gpu_birth_map import (H, MAX_INTER, POINT_MARKS, POINTS, U, W, make_ctx, model_desc, order_bound, point_energy_bound,
                                tile_maps)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
MODELS = ["mpp_hrcM", "mpp_log"]
JUNK_MARKS = (6.0, 0.5, 0.4)


# ---- selection alone ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bare_ctx():
    ctx = hip_api.MppContext(0)
    yield ctx
    ctx.close()


def assert_selection(ctx, xy, v, above, distance, what):
    xy, v = np.asarray(xy, np.int32).reshape(-1, 2), np.asarray(v, np.float64).reshape(-1)
    want, n_cand = select_points_ref(xy, v, above, distance)
    keep, nc, nk = ctx.select_points(xy, v, above, distance)
    keep = keep.cpu().numpy()
    print(f"{what}: {len(v)} points, {n_cand} candidates, {int(want.sum())} kept")
    assert keep.dtype == np.uint8 and keep.shape == want.shape, what
    np.testing.assert_array_equal(keep, want, err_msg=what)
    assert (nc, nk) == (n_cand, int(want.sum())), what
    return keep.tolist()


def test_selection_on_hand_made_lists(bare_ctx):
    ctx = bare_ctx
    assert assert_selection(ctx, np.zeros((0, 2)), [], 0.0, 64.0, "n = 0") == []
    assert assert_selection(ctx, [[3, 4]], [1.0], 0.0, 64.0, "n = 1") == [1]
    assert assert_selection(ctx, [[3, 4]], [0.0], 0.0, 64.0, "n = 1, no candidate") == [0]
    # the distance edge at the descent's own distance, 2 * max_inter = 64
    assert assert_selection(ctx, [[5, 3], [5, 67]], [1.0, 2.0], 0.0, 64.0, "exactly 64 apart") == [0, 1]
    assert assert_selection(ctx, [[140, 60], [141, 124]], [3.0, 4.0], 0.0, 64.0, "d^2 = 64^2 + 1") == [1, 1]
    assert assert_selection(ctx, [[2, 3], [5, 7], [20, 3], [21, 8]], [1.0, 2.0, 1.0, 2.0], 0.0, 5.0, "3-4-5") == [0, 1, 1, 1]
    # equal values on one pixel: the smaller slot; a NaN never, +inf is kept
    assert assert_selection(ctx, [[4, 4], [4, 4], [4, 6]], [1.0, 1.0, 1.0], 0.0, 1.0, "ties on one pixel") == [1, 0, 1]
    assert assert_selection(ctx, [[1, 1], [1, 2], [9, 9], [9, 9], [9, 10]], [NAN, 1.0, INF, 5.0, INF], 0.0, 1.0,
                            "NaN, +inf") == [0, 1, 1, 0, 0]
    # order-free, not a walk: b loses to a and c to b although a does not reach c
    assert assert_selection(ctx, [[1, 0], [1, 2], [1, 4]], [3.0, 2.0, 1.0], 0.0, 2.0, "a chain of three") == [1, 0, 0]
    assert assert_selection(ctx, [[1, 0], [1, 2], [1, 4]], [3.0, 2.0, 1.0], 3.0, 2.0, "above every value") == [0, 0, 0]
    assert assert_selection(ctx, [[1, 0], [1, 2], [1, 4]], [3.0, 2.0, 1.0], 0.0, 0.0, "distance 0") == [1, 1, 1]
    assert assert_selection(ctx, [[1, 0], [1, 2], [1, 4]], [-3.0, -2.0, -1.0], -2.5, 2.0, "a level below 0") == [0, 0, 1]
    # coordinates whose squared distance does not fit 32 bits
    assert assert_selection(ctx, [[0, 0], [60000, 60000]], [1.0, 2.0], 0.0, 64.0, "far apart") == [1, 1]


@pytest.mark.parametrize("n", [65, 257])
def test_selection_across_a_wave_and_a_workgroup(bare_ctx, n):
    rng = np.random.default_rng(n)
    xy = rng.integers(0, 96, (n, 2))
    v = np.round(rng.normal(0.0, 1.0, n), 1)                         # (rounded: equal values occur)
    v[[3, n - 1]] = NAN
    v[n - 2] = INF
    for distance in (3.0, 24.0, 64.0):
        keep = assert_selection(bare_ctx, xy, v, 0.0, distance, f"{n} random points, distance {distance}")
        assert 1 <= sum(keep) < int(np.sum(v > 0)) or distance == 3.0
    # the last point, alone in the second wave / workgroup, beats one of the first
    xy2, v2 = np.zeros((n, 2), np.int32), np.zeros(n)
    xy2[:, 1] = np.arange(n) * 100
    xy2[n - 1] = (0, 3)
    v2[0], v2[n - 1] = 1.0, 2.0
    keep = assert_selection(bare_ctx, xy2, v2, 0.0, 64.0, f"{n} points, the last beats the first")
    assert keep[0] == 0 and keep[n - 1] == 1 and sum(keep) == 1


def test_selection_with_every_point_equal_on_a_lattice(bare_ctx):
    """9 216 equal values: more than any workgroup's LDS chunk holds, and exactly slot 0 is kept"""
    xy = np.stack(np.meshgrid(np.arange(96), np.arange(96), indexing="ij"), axis=-1).reshape(-1, 2)
    v = np.full(96 * 96, 1.0)
    keep, nc, nk = bare_ctx.select_points(xy, v, 0.0, 136.0)         # (the diagonal is 134.4)
    assert (nc, nk) == (96 * 96, 1) and keep.cpu().numpy().tolist() == [1] + [0] * (96 * 96 - 1)
    keep, nc, nk = bare_ctx.select_points(xy, v, 0.0, 0.0)           # distinct pixels at distance 0: all of them
    assert (nc, nk) == (96 * 96, 96 * 96) and bool(keep.all())
    assert_selection(bare_ctx, xy[:1500], v[:1500], 0.0, 5.0, "lattice, 1 500 points")


def test_selection_refusals(bare_ctx):
    import torch
    ctx = bare_ctx
    xy = torch.zeros((4, 2), dtype=torch.int32, device="cuda:0")
    v = torch.ones((4,), dtype=torch.float64, device="cuda:0")
    keep = torch.full((4,), 7, dtype=torch.uint8, device="cuda:0")
    nc, nk = C.c_int64(-7), C.c_int64(-7)
    for n, above, distance in [(4, 0.0, -1.0), (4, 0.0, NAN), (4, 0.0, INF), (4, NAN, 3.0), (4, INF, 3.0), (4, -INF, 3.0),
                               (-1, 0.0, 3.0)]:
        rc = ctx._L.mpp_select_points(ctx._h, n, hip_api._ptr(xy), hip_api._ptr(v), above, distance, hip_api._ptr(keep),
                                      C.byref(nc), C.byref(nk))
        ctx.synchronize()
        message = ctx._L.mpp_last_error(ctx._h).decode()
        assert rc == -1 and keep.cpu().tolist() == [7] * 4 and "select_points" in message, (n, above, distance)
    with pytest.raises(ValueError):
        ctx.select_points(np.zeros((3, 2)), np.zeros(4), 0.0, 1.0)


# ---- the starting states ------------------------------------------------------------------------------------------------------

def state(kind, name, **options):
    """(desc, det, marks, device ctx, walk ctx) with the same starting state in both contexts"""
    if kind == "d":
        _, _, desc = model_desc(name)
        det, marks, xy, mk = state_d(synth.render_maps, synth.make_gt)
        pair = [make_ctx(desc, det, marks, **options) for _ in range(2)]
        for c in pair:
            c.set_points(0, xy, mk)
        return desc, det, pair[0], pair[1]
    return contexts(kind, name, **options)


def assert_equals_walk(ctx, chain, rep, src, walk, what):
    xy, mk = ctx.get_points(chain)
    print(f"{what}: status {walk['status']}, {walk['rounds']} round(s), +{walk['n_added']} -{walk['n_removed']} -> "
          f"{walk['n_after']} points, gains {walk['gain_births']!r} / {walk['gain_deaths']!r}, p {walk['papangelou']}, "
          f"map {walk['summary']}")
    np.testing.assert_array_equal(xy, walk["xy"], err_msg=what)                      # equal, not close
    np.testing.assert_array_equal(mk, walk["marks"], err_msg=what)
    n = walk["n_after"]
    np.testing.assert_array_equal(src[:n], walk["src"], err_msg=what)
    assert np.all(src[n:] == -1) and src.dtype == np.int32, what
    assert (int(rep["status"]), int(rep["rounds"]), int(rep["n_added"]), int(rep["n_removed"]), int(rep["n_after"])) == \
        (walk["status"], walk["rounds"], walk["n_added"], walk["n_removed"], walk["n_after"]), what
    assert float(rep["gain_births"]) == walk["gain_births"], (what, float(rep["gain_births"]), walk["gain_births"])   # the same bits
    assert float(rep["gain_deaths"]) == walk["gain_deaths"], (what, float(rep["gain_deaths"]), walk["gain_deaths"])
    assert (float(rep["max_p"]), int(rep["slot_max"]), int(rep["n_positive"])) == walk["papangelou"], what
    assert report_tuple(rep) == walk["summary"], what


def pairwise_further_than(xy, distance):
    p = np.asarray(xy, np.int64).reshape(-1, 2)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    d2[np.arange(len(p)), np.arange(len(p))] = 1 << 40
    return len(p) < 2 or d2.min() > distance * distance


def assert_energy_identity(desc, det, e_before, e_after, n_before, walk, all_marks, what):
    """E(after) - E(before) against gain_births - gain_deaths, within the bound derived in the module's docstring"""
    g = lambda m: (m - 1) * U / (1.0 - (m - 1) * U) if m > 1 else 0.0
    B1 = 1.0 if desc.combinator == E.C_LOGISTIC else point_energy_bound(desc, det, all_marks if len(all_marks) else None)
    n, kb, kd, mag_b, mag_d = n_before, 0, 0, 0.0, 0.0
    bound = g(n_before) * n_before * B1 + g(walk["n_after"]) * walk["n_after"] * B1
    for (rxy, rv), (axy, av) in zip(walk["removed"], walk["added"]):
        bound += len(rxy) * g(n) * n * 2.0 * B1
        n, kd, mag_d = n - len(rxy), kd + len(rxy), mag_d + float(np.abs(rv).sum())
        bound += len(axy) * order_bound(n, desc, det, all_marks if len(all_marks) else None)
        n, kb, mag_b = n + len(axy), kb + len(axy), mag_b + float(np.abs(av).sum())
    assert n == walk["n_after"]
    gain = walk["gain_births"] - walk["gain_deaths"]
    bound += g(kb + 1) * mag_b + g(kd + 1) * mag_d + 2.0 * U * (abs(e_after - e_before) + abs(gain))
    err = abs((e_after - e_before) - gain)
    print(f"{what}: E {e_before!r} -> {e_after!r}, births {walk['gain_births']!r} - deaths {walk['gain_deaths']!r}, "
          f"|difference| {err!r}, bound {bound!r}")
    assert np.isfinite(e_before) and np.isfinite(e_after) and err <= bound, (what, err, bound)


# ---- papangelou_all -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MODELS)
def test_papangelou_all_equals_papangelou_per_chain(name):
    _, _, desc = model_desc(name)
    det, marks, xy, mk = state_d(synth.render_maps, synth.make_gt)
    for grid_min in (None, 1):                                       # the default scans at these counts; 1: every chain by its grid
        ctx = make_ctx(desc, det, marks, replicas=3, point_capacity=64)
        if grid_min is not None:
            ctx.set_option("scratch_grid_min_points", grid_min)
        ctx.set_points(1, POINTS, POINT_MARKS)
        ctx.set_points(2, xy, mk)
        assert ctx.counts().tolist() == [0, 12, 50]
        p = ctx.papangelou_all()
        assert p.shape == (3, 64) and p.dtype == np.float64
        for c, n in enumerate((0, 12, 50)):
            one = ctx.papangelou(c)
            assert len(one) == n and p[c, :n].tobytes() == one.tobytes(), (name, grid_min, c)      # bit for bit
            assert np.all(p[c, n:] == 0.0) and not np.any(np.signbit(p[c, n:]))
        assert np.any(p[1] > 0) and np.any(p[2] > 0) and np.any(p[2] < 0)
        ctx.close()


# ---- the descent equals the host walk ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("what", [1, 2, 3])
@pytest.mark.parametrize("kind", ["b", "c", "d"])
def test_descent_equals_the_host_walk(kind, what, name):
    desc, det, ctx, ref = state(kind, name)
    n_before = ctx.count(0)
    marks_before = ctx.get_points(0)[1]
    e_before = float(ctx.total_energy_all()[0])
    walk = host_walk(ref, 0, MAX_INTER, what=what, max_rounds=64)
    rep, src = ctx.descend(what=what, max_rounds=64, src=True)
    assert len(rep) == 1 and rep.dtype == hip_api.DESCENT_REPORT_DTYPE and src.shape == (1, ctx.get_option("point_capacity"))
    label = f"state ({kind}), what {what}, {name}"
    assert_equals_walk(ctx, 0, rep[0], src[0], walk, label)
    # what the input has to exercise, asserted on the walk's values
    assert walk["status"] == 0
    if kind == "b" and what == 3:
        assert walk["n_removed"] >= 1 and walk["n_added"] >= 1
    if kind == "b" and what == 1:                     # the tile's diagonal is below 2 * max_inter: one death per round
        assert (walk["n_removed"], walk["rounds"], walk["n_after"]) == (9, 9, 3)
    if kind == "d" and what == 1:
        assert walk["n_removed"] >= 20 and any(len(r[0]) == 2 for r in walk["removed"])
    if not what & 2:
        assert walk["summary"] == NO_MAP and walk["n_added"] == 0
    if not what & 1:
        assert walk["n_removed"] == 0 and np.array_equal(walk["src"][:n_before], np.arange(n_before))
    # invariants that do not lean on the walk
    if what & 1:
        fresh = ctx.papangelou_all()[0]
        assert not np.any(fresh > 0) and int(rep[0]["n_positive"]) == 0 and not float(rep[0]["max_p"]) > 0
    if what & 2:
        dE, _, s = ctx.birth_energy_map()
        assert int(s[0]["n_negative"]) == 0 and int(rep[0]["n_negative"]) == 0 and not bool((dE < 0).any())
    for (rxy, _), (axy, _) in zip(walk["removed"], walk["added"]):
        assert pairwise_further_than(rxy, 2 * MAX_INTER) and pairwise_further_than(axy, 2 * MAX_INTER)
    assert_energy_identity(desc, det, e_before, float(ctx.total_energy_all()[0]), n_before, walk,
                           np.concatenate([marks_before, walk["marks"]]), label)
    ctx.close()
    ref.close()


@pytest.mark.parametrize("name", MODELS)
def test_the_points_removed_in_one_round_lie_further_apart_than_64(name):
    """the device alone, one round per call: ``src`` says which slots each round removed"""
    desc, det, ctx, ref = state("d", name)
    ref.close()
    e, total, rounds, pairs = float(ctx.total_energy_all()[0]), 0, 0, 0
    while True:
        xy = ctx.get_points(0)[0]
        rep, src = ctx.descend(what=1, max_rounds=1, src=True)
        k, n = int(rep[0]["n_removed"]), int(rep[0]["n_after"])
        gone = np.setdiff1d(np.arange(len(xy)), src[0][:n])
        assert len(gone) == k and n == len(xy) - k and np.all(np.diff(src[0][:n]) > 0)
        np.testing.assert_array_equal(ctx.get_points(0)[0], xy[src[0][:n]])
        if k == 0:
            assert int(rep[0]["status"]) == 0 and int(rep[0]["rounds"]) == 0
            break
        assert int(rep[0]["status"]) == 1 and int(rep[0]["rounds"]) == 1 and pairwise_further_than(xy[gone], 2 * MAX_INTER)
        e2 = float(ctx.total_energy_all()[0])
        assert e2 < e and float(rep[0]["gain_deaths"]) > 0           # every round lowers the energy
        e, total, rounds, pairs = e2, total + k, rounds + 1, pairs + (k == 2)
        assert rounds <= 64
    print(f"state (d), {name}: -{total} in {rounds} calls of one round, {pairs} with two removals")
    assert total >= 20 and pairs >= 1
    ctx.close()


# ---- births alone are the completion ----------------------------------------------------------------------------------------------

SHARED = ("status", "rounds", "n_added", "n_after", "min_dE", "x", "y", "n_negative", "n_nan")


def assert_same_as_completion(a, b, rounds, what):
    rep = a.descend(what=2, max_rounds=rounds)[0]
    done = b.birth_complete(max_rounds=rounds)[0]
    print(f"{what}: {done}")
    for k in SHARED:
        assert rep[k] == done[k] and rep[k].tobytes() == done[k].tobytes(), (what, k, rep[k], done[k])
    assert rep["gain_births"].tobytes() == done["gain"].tobytes() and int(rep["n_removed"]) == 0 and float(rep["gain_deaths"]) == 0.0
    for got, want in zip(a.get_points(0), b.get_points(0)):
        np.testing.assert_array_equal(got, want, err_msg=what)
    return done


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("kind", ["a", "b"])
def test_births_alone_equal_birth_complete(kind, name):
    desc, det, a, b = contexts(kind, name)
    done = assert_same_as_completion(a, b, 64 if kind == "a" else 16, f"state ({kind}), {name}")
    assert int(done["status"]) == 0 and int(done["n_added"]) >= 1
    a.close()
    b.close()
    desc, det, a, b = contexts(kind, name)                           # the round limit: one more map for the summary
    assert int(assert_same_as_completion(a, b, 1, f"state ({kind}), {name}, one round")["status"]) == 1
    a.close()
    b.close()


def test_births_alone_equal_birth_complete_at_the_capacity():
    _, _, desc = model_desc("mpp_hrcM")
    det, marks = tile_maps()
    pair = [make_ctx(desc, det, marks, point_capacity=len(POINTS)) for _ in range(2)]
    for c in pair:
        c.set_points(0, POINTS, POINT_MARKS)
    done = assert_same_as_completion(pair[0], pair[1], 16, "capacity")
    assert int(done["status"]) == 2 and int(done["n_added"]) == 0
    for c in pair:
        c.close()


# ---- state, limits and shapes -------------------------------------------------------------------------------------------------------

def test_a_run_after_the_descent_equals_a_run_after_set_points():
    setup, _, desc = model_desc("mpp_log")
    det, marks, xy0, mk0 = state_d(synth.render_maps, synth.make_gt)
    kd = kernels.make_kernels(mappings.default_mappings(), 1.0)

    def fresh():
        ctx = make_ctx(desc, det, marks, point_capacity=256, spec_waves=8)
        ctx.set_kernels(kd, intensity=[8.0])
        ctx.set_schedule(0.1, 0.999, 0.0)
        return ctx
    a = fresh()
    a.set_points(0, xy0, mk0)
    rep = a.descend(max_rounds=64)
    xy, mk = a.get_points(0)
    assert int(rep[0]["status"]) == 0 and int(rep[0]["n_removed"]) >= 20 and len(xy) == int(rep[0]["n_after"])
    e = a.total_energy_all()
    b = fresh()
    b.set_points(0, xy, mk)
    assert b.total_energy_all().tolist() == e.tolist()
    a.run(200, seed=23)
    b.run(200, seed=23)
    xa, ma = a.get_points(0)
    xb, mb = b.get_points(0)
    assert xa.tolist() != xy.tolist() or ma.tolist() != mk.tolist()                  # (the run did something)
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(ma, mb)
    assert a.step_index(0) == b.step_index(0) == 200
    a.close()
    b.close()


@pytest.mark.parametrize("what", [1, 3])
def test_max_rounds_1_reports_the_returned_state(what):
    desc, det, ctx, ref = state("b", "mpp_log")
    walk = host_walk(ref, 0, MAX_INTER, what=what, max_rounds=1)
    rep, src = ctx.descend(what=what, max_rounds=1, src=True)
    assert walk["status"] == 1 and walk["rounds"] == 1 and walk["n_removed"] == 1
    assert_equals_walk(ctx, 0, rep[0], src[0], walk, f"max_rounds 1, what {what}")
    p = ctx.papangelou_all()[0][:int(rep[0]["n_after"])]
    assert (float(rep[0]["max_p"]), int(rep[0]["slot_max"]), int(rep[0]["n_positive"])) == papangelou_summary(p)
    assert int(rep[0]["n_positive"]) > 0                             # (one round does not finish this tile)
    if what & 2:
        fresh, _, s = ctx.birth_energy_map()
        assert report_tuple(rep[0]) == report_tuple(s[0]) == numpy_summary(fresh[0].cpu().numpy())
    ctx.close()
    ref.close()


@pytest.mark.parametrize("name", MODELS)
def test_min_gain_leaves_nothing_above_it(name):
    desc, det, ctx, ref = state("b", name)
    g = 0.5 * float(np.max(ref.papangelou(0)))                       # half the largest p: that point still qualifies
    assert g > 0
    walk = host_walk(ref, 0, MAX_INTER, what=3, max_rounds=64, min_gain=g)
    rep, src = ctx.descend(what=3, max_rounds=64, min_gain=g, src=True)
    assert_equals_walk(ctx, 0, rep[0], src[0], walk, f"min_gain {g!r}, {name}")
    assert walk["status"] == 0 and walk["n_removed"] >= 1
    assert not np.any(ctx.papangelou_all()[0] > g) and not float(rep[0]["max_p"]) > g
    fresh = ctx.birth_energy_map()[0][0].cpu().numpy()
    assert not np.any(fresh < -g)
    assert int(rep[0]["n_negative"]) == int(np.sum(fresh < 0))       # (the summary still counts below 0, not below -g)
    ctx.close()
    ref.close()


def junk_state(cap, name="mpp_hrcM"):
    """a 96 x 96 tile with two objects in opposite corners, 101 px apart -- neither is detected, and each is the best candidate
    of its own disc of 64 px: two births in the first round -- and four copies of one bad rectangle in a third corner, 72 px
    from either: they are rivals of each other, one death per round"""
    _, _, desc = model_desc(name)
    det, marks = tile_maps((96, 96), seed=9, gt_xy=np.array([[12, 12], [84, 84]], np.int32),
                           gt_marks=np.array([[6.5, 0.5, 0.3], [7.0, 0.45, 1.2]]))
    xy = np.tile([84, 12], (4, 1)).astype(np.int32)
    mk = np.tile(JUNK_MARKS, (4, 1))
    ctx = make_ctx(desc, det, marks, point_capacity=cap)
    ctx.set_points(0, xy, mk)
    return desc, det, marks, xy, mk, ctx


def test_capacity_keeps_the_deaths_and_the_point_set_grows():
    desc, det, marks, xy, mk, big = junk_state(256)
    first = host_walk(big, 0, MAX_INTER, what=3, max_rounds=1)       # what the first round would do with room
    big.close()
    assert first["n_removed"] == 1 and first["n_added"] >= 2         # 4 - 1 + (>= 2) > 4: the first birth half overflows
    _, _, _, _, _, ctx = junk_state(4)
    _, _, _, _, _, ref = junk_state(4)
    walk = host_walk(ref, 0, MAX_INTER, what=3, max_rounds=64)
    rep, src = ctx.descend(what=3, max_rounds=64, src=True)
    assert_equals_walk(ctx, 0, rep[0], src[0], walk, "capacity 4")
    assert (walk["status"], walk["rounds"], walk["n_removed"], walk["n_added"], walk["n_after"]) == (2, 1, 1, 0, 3)
    assert src[0].tolist() == [1, 2, 3, -1] and float(rep[0]["gain_deaths"]) > 0 and float(rep[0]["gain_births"]) == 0.0
    ctx.close()
    ref.close()
    # the point set on the same input: it moves to larger contexts and finishes; the walk in the same parts is the standard
    setup, comb, _ = model_desc("mpp_hrcM")
    data = ImageWMaps(name="0", shape=(96, 96), image=None, detection_map=det, param_dist_maps=marks,
                      mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS, gt_config=[])
    unit, pair = setup.make_energies(data)
    pts = [Rectangle(int(x), int(y), size=float(m[0]), ratio=float(m[1]), angle=float(m[2])) for (x, y), m in zip(xy, mk)]
    ps = EPointsSet(pts, (96, 96), unit, pair, image_data=data, point_capacity=4)
    out = ps.descend(energy_combinator=comb, max_rounds=64)
    cap, cur, left, parts, alive = 4, (xy, mk), 64, [], list(range(4))
    while True:
        part = make_ctx(desc, det, marks, point_capacity=cap)
        part.set_points(0, *cur)
        w = host_walk(part, 0, MAX_INTER, what=3, max_rounds=left)
        part.close()
        parts.append(w)
        alive = [alive[s] if s >= 0 else -1 for s in w["src"]]
        cur, left, cap = (w["xy"], w["marks"]), left - w["rounds"], 2 * cap
        if w["status"] != 2:
            break
    assert len(parts) >= 2 and ps._ctx.get_option("point_capacity") == cap // 2 > 4
    rows = [(p.x, p.y, p.size, p.ratio, p.angle) for p in ps]
    assert rows == [tuple(r) for r in np.concatenate([cur[0], cur[1]], axis=1).tolist()] and len(ps) == out["n_after"]
    assert all((s >= 0 and p is pts[s]) or (s < 0 and not any(p is q for q in pts)) for s, p in zip(alive, ps))   # survivors stay
    gb, gd = parts[0]["gain_births"], parts[0]["gain_deaths"]
    for w in parts[1:]:
        gb, gd = gb + w["gain_births"], gd + w["gain_deaths"]
    assert (out["status"], out["rounds"], out["n_added"], out["n_removed"]) == \
        (parts[-1]["status"], sum(w["rounds"] for w in parts), sum(w["n_added"] for w in parts), sum(w["n_removed"] for w in parts))
    assert out["status"] == 0 and (out["gain_births"], out["gain_deaths"], out["gain"]) == (gb, gd, gb - gd)
    assert (out["max_p"], out["slot_max"], out["n_positive"]) == parts[-1]["papangelou"]
    assert (out["min_dE"], out["argmin"][0], out["argmin"][1], out["n_negative"], out["n_nan"]) == parts[-1]["summary"]


def test_chains_do_not_depend_on_each_other():
    _, _, desc = model_desc("mpp_hrcM")
    det, marks, xy, mk = state_d(synth.render_maps, synth.make_gt)
    configs = [NO_POINTS, (POINTS, POINT_MARKS), (xy, mk)]
    ctx = make_ctx(desc, det, marks, replicas=3, point_capacity=128)
    for c in range(3):
        ctx.set_points(c, *configs[c])
    rep, src = ctx.descend(what=3, max_rounds=64, src=True)
    final = ctx.get_points_all()
    assert len(rep) == 3 and len(set(int(r["rounds"]) for r in rep)) > 1             # (chains close in different rounds)
    assert all(int(r["status"]) == 0 for r in rep) and int(rep[2]["n_removed"]) >= 20 and int(rep[0]["n_added"]) >= 5
    for c in range(3):
        one = make_ctx(desc, det, marks, point_capacity=128)
        one.set_points(0, *configs[c])
        r1, s1 = one.descend(what=3, max_rounds=64, src=True)
        got = one.get_points(0)
        assert r1[0].tobytes() == rep[c].tobytes(), (c, r1[0], rep[c])               # every field, bit for bit
        np.testing.assert_array_equal(s1[0], src[c])
        np.testing.assert_array_equal(final[c][0], got[0])
        np.testing.assert_array_equal(final[c][1], got[1])
        one.close()
    ctx.close()


def test_chains_of_one_context_close_in_different_rounds():
    """the closed test of every kernel of a round reads the one book: an empty chain, the 12 points, and the state a completion
    of the 12 points returned (which the completion closes in its first round) equal three one-chain contexts, completed and
    descended.  The one-chain completions take 5, 2 and 0 rounds: pairwise different.  The one-chain descents take 5, 9 and 9:
    the last two states hold the same nine points to remove, one per round (the tile is smaller than the selection's
    distance), and that many rounds cover the two births the 12 points lack; there the empty chain closes before the others."""
    _, _, desc = model_desc("mpp_hrcM")
    det, marks = tile_maps()
    first = make_ctx(desc, det, marks, point_capacity=64)
    first.set_points(0, POINTS, POINT_MARKS)
    assert int(first.birth_complete(max_rounds=16)[0]["status"]) == 0
    configs = [NO_POINTS, (POINTS, POINT_MARKS), first.get_points(0)]
    first.close()
    calls = {"birth_complete": lambda c: (c.birth_complete(max_rounds=16), None),
             "descend": lambda c: c.descend(what=3, max_rounds=16, src=True)}
    for what, call in calls.items():
        ctx = make_ctx(desc, det, marks, replicas=3, point_capacity=64)
        for c in range(3):
            ctx.set_points(c, *configs[c])
        rep, src = call(ctx)
        final = ctx.get_points_all()
        ctx.close()
        rounds = []
        for c in range(3):
            one = make_ctx(desc, det, marks, point_capacity=64)
            one.set_points(0, *configs[c])
            r1, s1 = call(one)
            got = one.get_points(0)
            one.close()
            rounds.append(int(r1[0]["rounds"]))
            assert r1[0].tobytes() == rep[c].tobytes(), (what, c, r1[0], rep[c])     # every field, bit for bit
            assert src is None or np.array_equal(s1[0], src[c]), (what, c)
            np.testing.assert_array_equal(final[c][0], got[0], err_msg=f"{what}, chain {c}")
            np.testing.assert_array_equal(final[c][1], got[1], err_msg=f"{what}, chain {c}")
        print(f"{what}: rounds {rounds}, status {[int(r['status']) for r in rep]}")
        assert len(set(rounds)) >= (3 if what == "birth_complete" else 2), (what, rounds)


@pytest.mark.parametrize("name", MODELS)
def test_with_and_without_the_candidate_grid(name):
    out = []
    for grid_min in (1, 0):
        desc, det, ctx, ref = state("d", name)
        ref.close()
        ctx.set_option("scratch_grid_min_points", grid_min)
        rep, src = ctx.descend(what=3, max_rounds=64, src=True)
        assert ctx.get_option("birth_map_grid") == grid_min
        out.append((rep[0].tobytes(), src.tobytes(), ctx.get_points(0)[0].tobytes(), ctx.get_points(0)[1].tobytes()))
        assert int(rep[0]["status"]) == 0 and int(rep[0]["n_removed"]) >= 20
        ctx.close()
    assert out[0] == out[1]


def test_every_point_removed_and_an_empty_chain():
    desc, det, marks, xy, mk, ctx = junk_state(16)
    _, _, _, _, _, ref = junk_state(16)
    walk = host_walk(ref, 0, MAX_INTER, what=1, max_rounds=16)
    rep, src = ctx.descend(what=1, max_rounds=16, src=True)
    assert_equals_walk(ctx, 0, rep[0], src[0], walk, "every point removed")
    assert (walk["status"], walk["rounds"], walk["n_removed"], walk["n_after"]) == (0, 4, 4, 0)
    assert (float(rep[0]["max_p"]), int(rep[0]["slot_max"]), int(rep[0]["n_positive"])) == (-INF, -1, 0)
    assert ctx.count(0) == 0 and np.all(src == -1) and float(ctx.total_energy_all()[0]) == 0.0
    rep = ctx.descend(what=1)                                        # a chain that starts empty
    assert (int(rep[0]["status"]), int(rep[0]["rounds"]), int(rep[0]["n_removed"]), int(rep[0]["n_after"])) == (0, 0, 0, 0)
    assert float(rep[0]["gain_deaths"]) == 0.0 and report_tuple(rep[0]) == NO_MAP
    ctx.close()
    ref.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals():
    z = np.load(os.path.join(GOLDEN, "tape_contrast_96.npz"), allow_pickle=False)
    _, _, cdesc, image = contrast_model(z)
    shape = tuple(int(v) for v in z["shape"])
    ctx = hip_api.MppContext(0, point_capacity=32)
    for what in (1, 2, 3):
        with pytest.raises(hip_api.MppError, match="mpp_set_maps"):      # before set_maps
            ctx.descend(what=what)
    ctx.set_maps(np.zeros(shape, np.float32), [np.zeros(shape + (32,), np.float32)] * 3)
    for what in (1, 2, 3):
        with pytest.raises(hip_api.MppError, match="mpp_set_model"):     # before set_model
            ctx.descend(what=what)
    # a classic image energy: its unit terms are per point, so deaths alone run; the map refuses
    ctx.set_image(image)
    ctx.set_model(cdesc, mappings.default_mappings())
    rng = np.random.default_rng(3)
    xy = rng.integers(8, min(shape) - 8, (6, 2)).astype(np.int32)
    xy[1] = xy[0]
    mk = np.stack([rng.uniform(4.0, 9.0, 6), rng.uniform(0.3, 0.9, 6), rng.uniform(0.0, np.pi, 6)], axis=1)
    ctx.set_points(0, xy, mk)
    for what in (2, 3):
        with pytest.raises(hip_api.MppError, match="classic"):
            ctx.descend(what=what)
    np.testing.assert_array_equal(ctx.get_points(0)[0], xy)
    ref = hip_api.MppContext(0, point_capacity=32)
    ref.set_maps(np.zeros(shape, np.float32), [np.zeros(shape + (32,), np.float32)] * 3)
    ref.set_image(image)
    ref.set_model(cdesc, mappings.default_mappings())
    ref.set_points(0, xy, mk)
    walk = host_walk(ref, 0, MAX_INTER, what=1, max_rounds=16)
    rep, src = ctx.descend(what=1, src=True)
    assert_equals_walk(ctx, 0, rep[0], src[0], walk, "a classic image energy, deaths alone")
    ref.close()
    ctx.close()
    _, _, desc = model_desc("mpp_log")
    det, marks = tile_maps()
    ctx = make_ctx(desc, det, marks)
    ctx.set_points(0, POINTS, POINT_MARKS)
    for bad in (0, 4, -1):
        with pytest.raises(hip_api.MppError, match="what"):
            ctx.descend(what=bad)
    for bad in (0, -1, 1025):
        with pytest.raises(hip_api.MppError, match="max_rounds"):
            ctx.descend(max_rounds=bad)
    for bad in (-0.5, NAN, INF):
        with pytest.raises(hip_api.MppError, match="min_gain"):
            ctx.descend(min_gain=bad)
    np.testing.assert_array_equal(ctx.get_points(0)[0], POINTS)      # a refused call changes nothing
    # (a pair reduction that is neither max nor min is refused by mpp_set_model already -- ``unsupported (kind, reduce)
    # combination`` --, so the descent's own refusal of one, like the recombination's, cannot be reached through the ABI)
    import dataclasses
    bad = dataclasses.replace(desc, pair=[desc.pair[0][:2] + (2,) + desc.pair[0][3:]] + list(desc.pair[1:]))
    with pytest.raises(hip_api.MppError, match="reduce"):
        ctx.set_model(bad, mappings.default_mappings())
    ctx.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def test_infer_image_with_and_without_the_descent(tmp_path, caplog):
    from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel, format_descent_summary
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
                      mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS,
                      labels={"centers": np.zeros((0, 2)), "parameters": np.zeros((0, 3))}, gt_config=[])
    rows = lambda pts: [(p.x, p.y, p.size, p.ratio, p.angle) for p in pts]

    def run(value):
        """(rows, scores, summary, the pickle's bytes, the log) of one ``infer_image`` and the record written from it"""
        if value is None:
            model.config["inference"].pop("descent", None)
        else:
            model.config["inference"]["descent"] = value
        model.last_descent = None
        caplog.clear()
        with caplog.at_level(logging.INFO):
            merged, scores = model.infer_image(data, seed=5)
            out = str(tmp_path / "0001_results.pkl")
            model._result_record(1, out, data, merged, scores, descent=model.last_descent)
        log = [r.getMessage() for r in caplog.records]
        # (the line that times the launch differs from run to run)
        return rows(merged), np.asarray(scores), model.last_descent, open(out, "rb").read(), [m for m in log if not m.startswith("ran ")]

    assert "descent" not in cfg["inference"]
    off = run(None)
    off2 = run(False)
    assert off[2] is None and off2[2] is None and off[3] == off2[3] and off[4] == off2[4]        # off: byte for byte
    assert off[0] == off2[0] and "descent" not in pickle.loads(off[3]) and not any("descent" in m for m in off[4])
    on = run({"max_rounds": 256})
    summary = on[2]
    assert set(summary) == {"n_added", "n_removed", "rounds", "gain", "gain_births", "gain_deaths", "status", "max_p", "slot_max",
                            "n_positive", "min_dE", "argmin", "n_negative", "n_nan"}
    # the point set's own descent from the detections of the run without it, on the image as one tile
    unit, pair = model.energy_setup.make_energies(data)
    pts = [Rectangle(int(r[0]), int(r[1]), size=r[2], ratio=r[3], angle=r[4]) for r in off[0]]
    ps = EPointsSet(pts, (300, 400), unit, pair, image_data=data, point_capacity=max(1024, 2 * len(pts) + 64))
    want = ps.descend(energy_combinator=model.energy_model, max_rounds=256)
    print(f"infer_image: {len(pts)} detections, descent +{want['n_added']} -{want['n_removed']} in {want['rounds']} round(s)")
    assert want["n_added"] + want["n_removed"] >= 1                                  # (the chain of 4 000 steps leaves work)
    assert on[0] == rows(ps) and {k: want[k] for k in summary} == summary
    assert summary["status"] == 0 and summary["n_negative"] == 0 and summary["n_positive"] == 0
    np.testing.assert_array_equal(on[1], ps.papangelou_all(energy_combinator=model.energy_model))      # every point rescored
    assert len(on[1]) == len(on[0]) == len(off[0]) + summary["n_added"] - summary["n_removed"]
    record = pickle.loads(on[3])
    assert record["descent"] == summary and len(record["detection_points"]) == len(on[0])
    assert set(record) - {"descent"} == set(pickle.loads(off[3]))
    assert format_descent_summary(summary) in on[4]
    assert format_descent_summary(summary) == (f"descent: +{summary['n_added']} -{summary['n_removed']} object(s) in "
                                               f"{summary['rounds']} round(s), energy -{abs(summary['gain']):.2f}, 0 pixel(s) below 0, "
                                               f"0 point(s) above 0")
    # the descent contains the completion
    model.config["inference"]["birth_complete"] = True
    with pytest.raises(ValueError, match="descent contains the completion"):
        model.infer_image(data, seed=5)
    model.config["inference"]["birth_complete"] = False
    model.config["inference"]["descent"] = False
