"""Recombination of restarts on the GPU (``mpp_recombine``): the winner chain of a tile takes, for every
interaction cluster of the union of the tile's replicas, the points of the replica that spends the least energy there.

Every device output is compared with the NumPy restatement of the rules (tests/recombine_ref.py) EXACTLY -- integers, and
float64 by bit pattern with NaN equal to NaN -- on hand-set and on sampled states; ``check`` below also holds every state to
the properties the design rests on (per-point locality bit for bit, E_after, the two summation bounds).  Small on purpose:
one to four tiles of 64 to 256 px, ``point_capacity`` <= 256."""
import glob
import json
import logging
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from helpers import REPO, log_model
from recombine_ref import recombine_ref, same_bits, slot_sum
from test_gpu_pipeline import synthetic_dataset, write_image  # noqa: F401  (the fixture: a dataset directory with score maps)
from test_gpu_restarts import two_images, rows
from mpp_cnn_rs_object_detection_amd import energies as E
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings, synth
from mpp_cnn_rs_object_detection_amd.custom_types import ImageWMaps
from mpp_cnn_rs_object_detection_amd.sampler import (TileBatchSampler, resolve_schedule, sample_rjmcmc, sample_rjmcmc_batch,
                                                      select_replicas)
from mpp_cnn_rs_object_detection_amd.shapes import Rectangle

pytestmark = pytest.mark.gpu

MAX_INTER = 32.0            # the largest pair range of the mpp_log model (the overlap term's)
CAP = 256
U = 2.0 ** -53              # unit roundoff of float64


# ---- scenes and contexts ------------------------------------------------------------------------------------------------

def scene(size, gt_xy, gt_marks=None, noise=0.1, seed=0):
    """(det, marks) of a square tile with true objects at ``gt_xy``"""
    gt_xy = np.asarray(gt_xy, dtype=np.int32).reshape(-1, 2)
    if gt_marks is None:
        gt_marks = true_marks(len(gt_xy))
    return synth.render_maps((size, size), gt_xy, np.asarray(gt_marks, dtype=np.float64).reshape(-1, 3), noise=noise, noise_seed=seed)


def true_marks(n, seed=5):
    """marks of vehicle-like rectangles, as ``synth.make_gt`` draws them"""
    rng = np.random.default_rng(seed)
    size, ratio, angle = synth.wla_to_sra(rng.normal(4.5, 0.4, n), rng.normal(9.0, 0.8, n), rng.random(n) * np.pi)
    return np.stack([size, np.clip(ratio, 0.05, 1.0), angle], axis=1)


BAD = (9.5, 0.95, 0.3)       # a fat square where the maps promise a slim rectangle, or nothing


def context(maps, R, cap=CAP, **options):
    """a context of len(maps) tiles x R replicas under the mpp_log model; maps: [(det, marks)]"""
    setup, comb = log_model()
    unit, pair = setup.make_energies()
    ctx = hip_api.MppContext(0, point_capacity=cap, spec_waves=8, replicas=R)
    ctx.set_maps(np.stack([m[0] for m in maps]), [np.stack([m[1][k] for m in maps]) for k in range(3)])
    ctx.set_model(E.build_model_desc(unit, pair, comb), mappings.default_mappings())
    for name, value in options.items():
        ctx.set_option(name, value)
    assert ctx.get_option("n_chains") == len(maps) * R
    return ctx


def put(ctx, n, configs):
    """configs[i][r] = [(x, y, size, ratio, angle)] of replica r of tile i"""
    for i, tile in enumerate(configs):
        for r, pts in enumerate(tile):
            a = np.asarray(pts, dtype=np.float64).reshape(-1, 5)
            ctx.set_points(r * n + i, a[:, :2].astype(np.int32), a[:, 2:])


def snapshot(ctx):
    return [(xy.copy(), mk.copy()) for xy, mk in ctx.get_points_all()]


def check(ctx, n, R, cap=CAP, what=""):
    """``recombine`` on the context's state against the reference and the properties; returns (report, src, reference,
    chains before, chains after)."""
    T = n * R
    before = snapshot(ctx)
    energy = ctx.total_energy_all()
    e_rows = ctx.point_energies_all()
    assert e_rows.shape == (T, cap) and e_rows.dtype == np.float64
    for c in range(T):                                  # point energies: zero behind the count, the row's sum is the chain's energy
        assert np.all(e_rows[c, len(before[c][0]):] == 0.0) and not np.any(np.signbit(e_rows[c, len(before[c][0]):]))
        assert same_bits(slot_sum(e_rows[c]), energy[c]), (what, c)
        assert same_bits(energy[c], ctx.total_energy(c))
    vec_before = [ctx.total_energy(c, return_vectors=True)[1] for c in range(T)]

    rep, src = ctx.recombine(src=True)
    after = snapshot(ctx)
    ref = recombine_ref(before, e_rows, n, R, cap, MAX_INTER, energy)
    assert rep.dtype == hip_api.RECOMBINE_REPORT_DTYPE and rep.shape == (n,) and src.shape == (n, cap, 2) and src.dtype == np.int32
    for i in range(n):
        t, g = ref[i], rep[i]
        print(f"{what} tile {i}: " + ", ".join(f"{k} {g[k]!r}" for k in rep.dtype.names))
        for k in ("status", "winner", "n_clusters", "n_taken", "n_before", "n_after"):
            assert int(g[k]) == t[k], (what, i, k, int(g[k]), t[k])
        assert same_bits(g["E_winner"], t["E_winner"]) and same_bits(g["E_sum"], t["E_sum"]), (what, i, g, t["E_sum"])
        assert np.array_equal(src[i], t["src"]), (what, i)
        w = int(g["winner"])
        wc = w * n + i
        for r in range(R):                                               # every other chain is untouched
            c = r * n + i
            exp = (t["xy"], t["marks"]) if r == w else before[c]
            assert after[c][0].tobytes() == np.ascontiguousarray(exp[0], np.int32).tobytes(), (what, i, r)
            assert after[c][1].tobytes() == np.ascontiguousarray(exp[1], np.float64).tobytes(), (what, i, r)
        if g["status"] != 1:
            assert after[wc][0].tobytes() == before[wc][0].tobytes() and after[wc][1].tobytes() == before[wc][1].tobytes()
            assert same_bits(g["E_after"], g["E_winner"])
        # E_after is the energy of the written state; per-point locality: every point kept its energy vector, bit for bit
        e_after, vec_after = ctx.total_energy(wc, return_vectors=True)
        assert same_bits(g["E_after"], e_after), (what, i, g["E_after"], e_after)
        assert len(vec_after) == g["n_after"]
        for k in range(int(g["n_after"])):
            r, s = src[i, k]
            assert same_bits(vec_after[k], vec_before[r * n + i][s]), (what, i, k, (r, s))
        # the two bounds: N the tile's points over all replicas, A the sum of |e| over them; recursive summation of at most
        # N terms errs by at most (N - 1) u A (+ O(u^2)), E_sum and E_after are two such sums of the same kept terms,
        # E_winner a third whose exact value is, by the choice, no lower than E_sum's
        pts = np.concatenate([e_rows[r * n + i, :len(before[r * n + i][0])] for r in range(R)])
        N, A = len(pts), float(np.sum(np.abs(pts)))
        if np.isfinite(A):
            print(f"{what} tile {i}: N {N}, A {A!r}, |E_after - E_sum| {abs(g['E_after'] - g['E_sum'])!r} (bound {2 * N * U * A!r}), "
                  f"E_after - E_winner {g['E_after'] - g['E_winner']!r} (bound {4 * N * U * A!r})")
            if g["status"] != 2:                         # (status 2 writes nothing: E_after is the winner's, E_sum the unwritten composite's)
                assert abs(g["E_after"] - g["E_sum"]) <= 2 * N * U * A
            assert g["E_after"] <= g["E_winner"] + 4 * N * U * A
    return rep, src, ref, before, after


# ---- 1. two groups far apart --------------------------------------------------------------------------------------------

A_POS, B_POS = (30, 30), (95, 95)


def two_group_tile(shift=0):
    gt = np.array([A_POS, B_POS]) + shift
    return gt, true_marks(2, seed=5 + shift)


def two_group_configs(gt, tm):
    (ax, ay), (bx, by) = gt.tolist()
    good_a, good_b = (ax, ay, *tm[0]), (bx, by, *tm[1])
    return [[good_a, (bx + 2, by - 3, *BAD)], [(ax - 3, ay + 2, *BAD), good_b]]


def test_two_groups_take_the_true_object_of_each():
    gt, tm = two_group_tile()
    ctx = context([scene(128, gt, tm)], 2)
    put(ctx, 1, [two_group_configs(gt, tm)])
    e_before = ctx.total_energy_all()
    rep, src, ref, before, after = check(ctx, 1, 2, what="two groups")
    g = rep[0]
    assert g["status"] == 1 and g["n_taken"] == 1 and g["n_clusters"] == 2 and g["n_after"] == 2
    got = {(int(x), int(y)) for x, y in after[int(g["winner"])][0]}
    assert got == {A_POS, B_POS}                                  # both true objects
    assert g["E_after"] < e_before.min()                          # below both replicas' energies
    # equivalent state: a fresh context given the composite returns the same energy and Papangelou bits
    fresh = context([scene(128, gt, tm)], 2)
    fresh.set_points(0, *after[int(g["winner"])])
    assert same_bits(fresh.total_energy(0), g["E_after"])
    assert same_bits(fresh.papangelou(0), ctx.papangelou(int(g["winner"])))
    fresh.close()
    ctx.close()


# ---- 2. the link boundary -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset,is_linked", [((0, 32), True), ((24, 21), True), ((32, 1), False), ((31, 8), False), ((20, 25), False)])
def test_link_boundary(offset, is_linked):
    """Replica 0: the true object p and a bad rectangle q, ``offset`` apart; replica 1: two bad rectangles next to p, on the
    side away from q (more than 32 px from q for every offset that is not a link itself).  Replica 0
    wins.  Linked: one cluster, which stays (status 0).  Not linked: q is a cluster of its own with a positive energy
    against the other replica's 0.0 -- it goes (status 1, one point left)."""
    p = (60, 60)
    tm = true_marks(1, seed=9)
    ctx = context([scene(128, [p], tm)], 2)
    q = (p[0] + offset[0], p[1] + offset[1])
    put(ctx, 1, [[[(*p, *tm[0]), (*q, *BAD)], [(p[0] - 1, p[1], *BAD), (p[0], p[1] - 2, *BAD)]]])
    e = ctx.point_energies_all()
    assert e[0, 1] > 0.0 and e[0, 0] + e[0, 1] < e[1, 0] + e[1, 1]          # what the construction needs
    rep, src, ref, before, after = check(ctx, 1, 2, what=f"offset {offset}")
    g = rep[0]
    assert g["winner"] == 0
    if is_linked:
        assert g["n_clusters"] == 1 and g["status"] == 0 and g["n_after"] == 2
    else:
        assert g["n_clusters"] == 2 and g["status"] == 1 and g["n_taken"] == 1 and g["n_after"] == 1
        assert after[0][0].tolist() == [list(p)]
    ctx.close()


# ---- 3. a long path -----------------------------------------------------------------------------------------------------

def serpentine():
    """62 points, 61 links: 7 rows 40 px apart (not linked) of 8 points 32 px apart (linked), one connector between
    consecutive row ends, 20 px from each"""
    path = []
    for row in range(7):
        x = 8 + 40 * row
        ys = [8 + 32 * k for k in range(8)]
        ys = ys if row % 2 == 0 else ys[::-1]
        path += [(x, y) for y in ys]
        if row < 6:
            path.append((x + 20, ys[-1]))
    return path


@pytest.mark.parametrize("first", ["end", "middle"])
def test_a_serpentine_is_one_cluster(first):
    """the worst cases of label propagation: the smallest global index at an end of the path, and in its middle"""
    path = serpentine()
    assert len(path) == 62
    marks = true_marks(len(path), seed=3)
    pts = [(*xy, *m) for xy, m in zip(path, marks)]
    reps = [pts[0::2], pts[1::2]]                                 # consecutive points alternate between the replicas
    if first == "middle":
        reps[0] = reps[0][15:] + reps[0][:15]                     # slot 0 of replica 0: the 31st point of the path
    ctx = context([scene(256, np.zeros((0, 2)), np.zeros((0, 3)))], 2)
    put(ctx, 1, [reps])
    rep, src, ref, before, after = check(ctx, 1, 2, what=f"serpentine, smallest index at the {first}")
    assert rep[0]["n_clusters"] == 1 and rep[0]["status"] == 0
    assert all(np.all(c == 0) for c in ref[0]["cluster"])
    ctx.close()


# ---- 4. empty and identical replicas ------------------------------------------------------------------------------------

def test_empty_and_identical_replicas():
    gt, tm = two_group_tile()
    maps = scene(128, gt, tm)
    ctx = context([maps, maps, maps], 2)
    cfg = two_group_configs(gt, tm)
    put(ctx, 3, [[cfg[0], []], [[], []], [cfg[0], cfg[0]]])
    rep, src, ref, before, after = check(ctx, 3, 2, what="replicas")
    # tile 0: replica 1 is empty; its 0.0 wins the tile (a true object and a bad rectangle sum to more) and the bad
    # rectangle's cluster, the true object's cluster is taken from replica 0
    assert rep[0]["winner"] == 1 and rep[0]["n_before"] == 0 and rep[0]["status"] == 1 and rep[0]["n_taken"] == 1
    assert rep[0]["n_after"] == 1 and after[3][0].tolist() == [list(A_POS)]
    # tile 1: nothing at all
    assert rep[1]["status"] == 0 and rep[1]["n_clusters"] == 0 and rep[1]["n_after"] == 0 and rep[1]["E_sum"] == 0.0
    # tile 2: identical replicas tie everywhere: the winner chain keeps its bytes (checked in ``check`` for status 0)
    assert rep[2]["status"] == 0 and rep[2]["winner"] == 0 and rep[2]["n_clusters"] == 2 and rep[2]["n_taken"] == 0
    ctx.close()


# ---- 5. the composite does not fit --------------------------------------------------------------------------------------

def test_a_composite_that_does_not_fit_leaves_its_tile_alone():
    cap = 6
    grid = [(20 + 40 * a, 20 + 40 * b) for a in range(3) for b in range(3)][:8]        # 8 places, 40 px apart: no links
    tm = true_marks(8, seed=11)
    full = scene(128, grid, tm)
    gt, tm2 = two_group_tile()
    two = scene(128, gt, tm2)
    ctx = context([two, full, two], 2, cap=cap)
    good = [(*grid[k], *tm[k]) for k in range(8)]
    bad = [(grid[k][0] + 2, grid[k][1] - 2, *BAD) for k in range(8)]
    # replica 0: the true objects of places 0-3 and one bad rectangle; replica 1: those of places 4-7 and two bad ones.
    # Replica 0 wins; every place is better in one of the two: 8 points > 6
    put(ctx, 3, [two_group_configs(gt, tm2), [good[:4] + [bad[4]], good[4:] + [bad[0], bad[1]]], two_group_configs(gt, tm2)])
    rep, src, ref, before, after = check(ctx, 3, 2, cap=cap, what="does not fit")
    assert rep["status"].tolist() == [1, 2, 1]
    assert rep[1]["winner"] == 0 and rep[1]["n_taken"] == 4 and rep[1]["n_before"] == rep[1]["n_after"] == 5
    assert len(ref[1]["kept"]) == 8
    ctx.close()


# ---- 6. shapes ----------------------------------------------------------------------------------------------------------

def blob_state(n, R, counts, seed, size=256):
    """Random states with many clusters: the true objects of a 256-px tile sit on a 64-px lattice of places; every replica
    holds, per place it visits, the true object or rectangles at random within 10 px of it.  Places are 64 px apart, so
    two places never link.  counts[i][r]: points of replica r of tile i."""
    rng = np.random.default_rng(seed)
    places = np.array([(32 + 64 * a, 32 + 64 * b) for a in range(size // 64) for b in range(size // 64)])
    maps, configs = [], []
    for i in range(n):
        tm = true_marks(len(places), seed=seed + 10 * i)
        maps.append(scene(size, places, tm, seed=i))
        tile = []
        for r in range(R):
            pts = []
            where = rng.integers(0, len(places), counts[i][r])
            for k, p in enumerate(where):
                if rng.random() < 0.3 and not any(q[:2] == tuple(places[p]) for q in pts):
                    pts.append((*places[p].tolist(), *tm[p]))
                else:
                    x, y = places[p] + rng.integers(-10, 11, 2)
                    pts.append((int(x), int(y), rng.uniform(4.0, 9.0), rng.uniform(0.3, 0.9), rng.uniform(0.0, np.pi)))
            tile.append(pts)
        configs.append(tile)
    return maps, configs


@pytest.mark.parametrize("R,counts", [(3, [[63, 64, 65], [1, 128, 0]]),
                                      (4, [[127, 129, 64, 5], [40, 41, 39, 42], [192, 63, 65, 191]])])
def test_shapes(R, counts):
    n = len(counts)
    maps, configs = blob_state(n, R, counts, seed=100 + R)
    ctx = context(maps, R)
    put(ctx, n, configs)
    rep, src, ref, before, after = check(ctx, n, R, what=f"R {R}")
    assert np.any(rep["status"] == 1) and rep["n_clusters"].min() >= 8
    if R == 4:
        assert len(set(rep["winner"].tolist())) > 1              # tiles with different winners
    ctx.close()


def test_labels_in_lds_and_in_device_memory_agree():
    """``recombine_lds_points`` (default and upper limit RECOMBINE_LDS_POINTS = 2048): a tile whose replicas hold more points
    together labels in the call's device-memory workspace.  Lowered to 300 it puts tile 0 (260 points) on the LDS side and
    tile 1 (340) on the other; at 0 and at the default both tiles are on one side.  Same outputs."""
    assert hip_api.RECOMBINE_LDS_POINTS == 2048
    counts = [[65, 64, 66, 65], [85, 86, 84, 85]]
    maps, configs = blob_state(2, 4, counts, seed=7)
    got = []
    for bound in (300, 0, hip_api.RECOMBINE_LDS_POINTS):
        ctx = context(maps, 4, recombine_lds_points=bound)
        assert ctx.get_option("recombine_lds_points") == bound
        put(ctx, 2, configs)
        rep, src, ref, before, after = check(ctx, 2, 4, what=f"lds bound {bound}")
        got.append((rep.tobytes(), src.tobytes(), [(a.tobytes(), b.tobytes()) for a, b in after]))
        assert np.any(rep["status"] == 1)
        ctx.close()
    assert got[0] == got[1] == got[2]
    with pytest.raises(hip_api.MppError, match="recombine_lds_points"):
        context(maps[:1], 2, recombine_lds_points=hip_api.RECOMBINE_LDS_POINTS + 1)


def test_the_lds_bound_itself():
    """at the bound as shipped: 16 replicas of 128 points are 2048 points (LDS), of 129 points 2064 (device memory)"""
    counts = [[128] * 16, [129] * 16]
    maps, configs = blob_state(2, 16, counts, seed=21)
    ctx = context(maps, 16)
    put(ctx, 2, configs)
    assert ctx.counts().reshape(16, 2).sum(axis=0).tolist() == [2048, 2064]
    rep, src, ref, before, after = check(ctx, 2, 16, what="2048 / 2064 points")
    assert np.any(rep["status"] == 1)
    ctx.close()


# ---- 7. the candidate grids ---------------------------------------------------------------------------------------------

def test_scratch_grid_min_points_changes_nothing():
    counts = [[40, 12, 70], [15, 16, 17]]
    maps, configs = blob_state(2, 3, counts, seed=33)
    got = []
    for grid_min in (0, 16):
        ctx = context(maps, 3, scratch_grid_min_points=grid_min)
        put(ctx, 2, configs)
        rep, src, ref, before, after = check(ctx, 2, 3, what=f"scratch_grid_min_points {grid_min}")
        got.append((rep.tobytes(), src.tobytes(), [(a.tobytes(), b.tobytes()) for a, b in after]))
        ctx.close()
    assert got[0] == got[1]


# ---- 8. energies that are not finite ------------------------------------------------------------------------------------

def test_a_nan_in_the_maps():
    counts = [[30, 31, 29]]
    maps, configs = blob_state(1, 3, counts, seed=44)
    det = maps[0][0].copy()
    hit = [configs[0][0][3][:2], configs[0][1][5][:2], configs[0][2][0][:2]]       # under one point of every replica
    for x, y in hit:
        det[int(x), int(y)] = np.nan
    ctx = context([(det, maps[0][1])], 3)
    put(ctx, 1, configs)
    e = ctx.point_energies_all()
    assert np.isnan(e[0, 3]) and np.isnan(e[1, 5]) and np.isnan(e[2, 0]) and np.count_nonzero(np.isfinite(e[:, :29])) > 60
    rep, src, ref, before, after = check(ctx, 1, 3, what="NaN")
    assert np.isnan(rep[0]["E_winner"])                          # every chain energy is NaN: replica 0 wins
    assert rep[0]["winner"] == 0 and rep[0]["n_clusters"] >= 8
    ctx.close()


# ---- sampled states -----------------------------------------------------------------------------------------------------

def image_of(tile):
    return ImageWMaps(name="t", shape=tile.shape, image=None, detection_map=tile.det, param_dist_maps=tile.marks,
                      mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS, gt_config=[])


T_S, R_S = 2, 4
SAMPLED = dict(num_samples=1, init_temperature=0.3, alpha_t=0.998, burn_in=2500, samples_interval=500, target_temperature=0.0)


def sampled_tiles():
    return [image_of(synth.make_tile(256, 50, tile_id=300 + k, noise=0.2)) for k in range(T_S)]


def run_sampler(tiles, seed=5, **kw):
    setup, comb = log_model()
    alpha, Tt, total, snaps = resolve_schedule(1, SAMPLED["init_temperature"], SAMPLED["alpha_t"], SAMPLED["burn_in"],
                                               SAMPLED["samples_interval"], 0.0)
    assert snaps[-1] + 1 == total                                # (no trailing steps: the context holds the returned state)
    s = TileBatchSampler(tiles, setup, comb, spec_waves=8, point_capacity=CAP, **kw)
    s.init("naive")
    out = s.run(total, snaps, 1, SAMPLED["init_temperature"], alpha, Tt, seed=seed, chain0=0, as_arrays=True)
    return s, out


def test_sampled_states():
    """R = 4 restarts of two 256-px tiles after 3 001 steps: reference and properties, a tile that is recombined, and the
    equivalent state in a fresh context"""
    tiles = sampled_tiles()
    s, out = run_sampler(tiles, restarts=R_S)
    ctx = s.ctx
    rep, src, ref, before, after = check(ctx, T_S, R_S, what="sampled")
    assert np.any((rep["status"] == 1) & (rep["n_taken"] >= 1))  # not vacuous
    assert np.all(rep["E_after"] <= rep["E_winner"]) and np.any(rep["E_after"] < rep["E_winner"])
    for i in range(T_S):
        wc = int(rep[i]["winner"]) * T_S + i
        fresh = context([(tiles[i].detection_map, tiles[i].param_dist_maps)], 2)
        fresh.set_points(0, *after[wc])
        assert same_bits(fresh.total_energy(0), rep[i]["E_after"])
        assert same_bits(fresh.papangelou(0), ctx.papangelou(wc))
        fresh.close()
    ctx.close()


# ---- the layers ---------------------------------------------------------------------------------------------------------

def test_sampler_returns_the_composites():
    tiles = sampled_tiles()
    plain, out0 = run_sampler(tiles, restarts=R_S)
    assert plain.recombine is False and plain.recombine_report is None
    again, out00 = run_sampler(tiles, restarts=R_S, recombine=False)
    on, out1 = run_sampler(tiles, restarts=R_S, recombine=True)
    assert same_bits(on.replica_energy, plain.replica_energy) and on.replica_energy.shape == (R_S, T_S)
    assert on.replica_winner.tolist() == plain.replica_winner.tolist() == select_replicas(plain.replica_energy, T_S).tolist()
    rep = on.recombine_report
    assert rep.dtype == hip_api.RECOMBINE_REPORT_DTYPE and len(rep) == T_S and np.any(rep["status"] == 1)
    # the composites, as the reference forms them from the plain run's state (``check``: reference, locality, bounds)
    ref_rep, ref_src, ref, before, composite = check(plain.ctx, T_S, R_S, what="sampler")
    assert ref_rep.tobytes() == rep.tobytes()
    for i in range(T_S):
        w = int(rep[i]["winner"])
        assert same_bits(rep[i]["E_winner"], plain.replica_energy[w, i])
        (xy, mk), (cxy, cmk) = out1[i][-1], composite[w * T_S + i]
        assert xy.tobytes() == cxy.tobytes() and mk.tobytes() == cmk.tobytes() and len(xy) == rep[i]["n_after"]
        # recombine=False is the code path of today: the same bytes, with and without the argument
        (axy, amk), (bxy, bmk) = out0[i][-1], out00[i][-1]
        assert axy.tobytes() == bxy.tobytes() and amk.tobytes() == bmk.tobytes()
        if rep[i]["status"] == 1:
            assert (xy.tobytes(), mk.tobytes()) != (axy.tobytes(), amk.tobytes())
    for s in (plain, again, on):
        s.ctx.close()


def test_refusals():
    tiles = sampled_tiles()[:1]
    setup, comb = log_model()
    with pytest.raises(ValueError, match="restarts >= 2"):
        TileBatchSampler(tiles, setup, comb, point_capacity=CAP, recombine=True)
    with pytest.raises(ValueError, match="restarts >= 2"):
        sample_rjmcmc(tiles[0], np.random.default_rng(1), energy_combinator=comb, init_config="naive", energy_setup=setup,
                      point_capacity=CAP, restarts=1, recombine=True, **SAMPLED)
    with pytest.raises(ValueError, match="num_samples"):
        sample_rjmcmc_batch(tiles, np.random.default_rng(1), energy_combinator=comb, init_config="naive", energy_setup=setup,
                            point_capacity=CAP, restarts=2, recombine=True, **dict(SAMPLED, num_samples=2))
    # the library: one replica, no maps
    ctx = context([scene(64, [(30, 30)])], 1)
    with pytest.raises(hip_api.MppError, match="replicas"):
        ctx.recombine()
    ctx.close()
    bare = hip_api.MppContext(0, point_capacity=CAP, replicas=2)
    with pytest.raises(hip_api.MppError, match="mpp_set_maps"):
        bare.recombine()
    bare.close()
    from mpp_cnn_rs_object_detection_amd.mpp_model import check_recombine
    assert check_recombine({"inference": {}}) is False and check_recombine({"inference": {"restarts": 3, "recombine": True}}) is True
    assert check_recombine({"inference": {"restarts": 1, "recombine": False}}) is False
    with pytest.raises(ValueError, match="inference.restarts to 2 or more"):
        check_recombine({"inference": {"recombine": True}})
    with pytest.raises(ValueError, match="ranks share"):
        check_recombine({"inference": {"restarts": 2, "recombine": True}}, world_size=2)
    with pytest.raises(ValueError, match="true or false"):
        check_recombine({"inference": {"restarts": 2, "recombine": 1}})


def test_recombine_with_tempering():
    """The tempered replicas are configurations on the same maps like any others: the tempered run's state goes through
    ``check`` -- the reference, per-point locality and the bounds with the tile's own N and A, "never worse than the tempered
    winner" (E_after <= E_winner + 4 N u A) among them -- and the same run with ``recombine=True`` returns that report and
    those composites."""
    tiles = sampled_tiles()
    tempering = {"ratio": 1.25, "every": 1000}
    plain, out0 = run_sampler(tiles, restarts=R_S, tempering=tempering)
    assert plain.exchange_log is not None and len(plain.exchange_log) > 0 and np.any(plain.exchange_log["accepted"] != 0)
    rep0, src0, ref, before, after = check(plain.ctx, T_S, R_S, what="tempered")
    assert np.any(rep0["status"] == 1)
    on, out = run_sampler(tiles, restarts=R_S, tempering=tempering, recombine=True)
    rep = on.recombine_report
    assert rep.tobytes() == rep0.tobytes()
    assert on.exchange_log.tobytes() == plain.exchange_log.tobytes() and on.replica_rung.shape == (R_S, T_S)
    assert same_bits(on.replica_energy, plain.replica_energy)
    assert on.replica_winner.tolist() == select_replicas(on.replica_energy, T_S).tolist() == rep["winner"].tolist()
    for i in range(T_S):
        w = int(rep[i]["winner"])
        assert same_bits(rep[i]["E_winner"], on.replica_energy[w, i])
        (xy, mk), (cxy, cmk) = out[i][-1], after[w * T_S + i]
        assert xy.tobytes() == cxy.tobytes() and mk.tobytes() == cmk.tobytes()
    plain.ctx.close()
    on.ctx.close()


def model_with(**inference):
    from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel
    cfg = json.load(open(os.path.join(REPO, "model_configs", "mpp", "config_mpp_log.json")))
    cfg["inference"]["rjmcmc_params"].update(burn_in=2500, alpha_t=0.998, init_temperature=0.2)
    cfg["inference"].update(inference)
    cwd = os.getcwd()
    os.chdir(REPO)                       # paths_config.json is resolved from the working directory, as upstream
    try:
        return MPPModel(cfg, phase="val", load=True)
    finally:
        os.chdir(cwd)


def spy_on_recombine(monkeypatch):
    """every ``MppContext.recombine`` from here on also records, per tile, N (the points over all replicas) and A (the sum of
    their |e|) of the state BEFORE the call, next to the report: -> the list the records are appended to"""
    seen, plain = [], hip_api.MppContext.recombine

    def spy(self, src=False):
        e, counts = self.point_energies_all(), self.counts()
        out = plain(self, src)
        report = (out[0] if src else out).copy()
        R = len(counts) // len(report)
        seen.append({"N": counts.reshape(R, -1).sum(axis=0), "A": np.abs(e).sum(axis=1).reshape(R, -1).sum(axis=0), "report": report})
        return out
    monkeypatch.setattr(hip_api.MppContext, "recombine", spy)
    return seen


def assert_bounds(record):
    """the issue's two bounds with the tile's own N and A"""
    r, N, A = record["report"], record["N"], record["A"]
    assert np.all(np.isfinite(A)) and np.all(N > 0)
    print(f"N {N.tolist()}, A {A.tolist()}, E_after - E_winner {(r['E_after'] - r['E_winner']).tolist()}, "
          f"bound {(4 * N * U * A).tolist()}")
    assert np.all(r["E_after"] <= r["E_winner"] + 4 * N * U * A)
    ok = r["status"] != 2
    assert np.all(np.abs(r["E_after"] - r["E_sum"])[ok] <= (2 * N * U * A)[ok])


def test_model_image_path_equals_dataset_path_and_writes_the_key(caplog, tmp_path, monkeypatch):
    images, seeds = two_images(), [21, 22]
    model = model_with(restarts=3, recombine=True)
    seen = spy_on_recombine(monkeypatch)
    per_image, summaries = [], []
    with caplog.at_level(logging.INFO):
        for data, seed in zip(images, seeds):
            det, scores = model.infer_image(data, seed=seed)
            s = model.last_run["recombine"]
            assert set(s) == {"status", "n_clusters", "n_taken", "E_winner", "E_after"} and len(s["status"]) == 2
            w = model.last_run["replica_winner"]
            assert w.tolist() == select_replicas(model.last_run["replica_energy"], 2).tolist()
            assert same_bits(s["E_winner"], model.last_run["replica_energy"][w, np.arange(2)])
            # never worse than the winner, by the bound with the tiles' own N and A (taken before the call)
            assert len(seen) == len(per_image) + 1 and same_bits(seen[-1]["report"]["E_after"], s["E_after"])
            assert_bounds(seen[-1])
            per_image.append(rows(det, scores))
            summaries.append(s)
    lines = [r.getMessage() for r in caplog.records if "recombine:" in r.getMessage()]
    assert len(lines) == 2 and all(" cluster(s) in " in t and "taken from another replica, energy -" in t for t in lines)
    assert any(np.any(s["status"] == 1) for s in summaries)      # (a scene in which the option changes something)
    batch = model.infer_images(images, image_seeds=seeds)
    assert len(seen) == 3 and len(seen[-1]["report"]) == 4       # one call for the four tiles of the two images
    assert_bounds(seen[-1])
    for k in range(2):
        assert rows(*batch[k]) == per_image[k]
        for key in summaries[k]:
            assert same_bits(model.last_recombine[k][key], summaries[k][key]), key
    # the pickle's key
    data = images[0]
    data.labels = {"centers": np.zeros((0, 2)), "parameters": np.zeros((0, 3))}
    out_file = str(tmp_path / "0000_results.pkl")
    model._result_record(0, out_file, data, *model.infer_image(data, seed=21), recombine=model.last_run["recombine"])
    with open(out_file, "rb") as f:
        record = pickle.load(f)
    assert set(record["recombine"]) == {"status", "n_clusters", "n_taken", "E_winner", "E_after"}
    assert same_bits(record["recombine"]["E_after"], summaries[0]["E_after"])
    # without the key: no record, no line, today's results
    off, base = model_with(restarts=3, recombine=False), model_with(restarts=3)
    for data, seed in zip(images, seeds):
        a, b = rows(*off.infer_image(data, seed=seed)), rows(*base.infer_image(data, seed=seed))
        assert a == b and off.last_run["recombine"] is None and base.last_run["recombine"] is None


def test_main_infer_writes_the_key_into_every_pickle(synthetic_dataset):
    """``main.py -p infer --restarts 3 --recombine`` over a dataset of two images: the flag reaches ``MPPModel.infer``, whose
    batches hand every image's summary to its ``NNNN_results.pkl`` (key ``recombine``) and log one line per image."""
    root, _ = synthetic_dataset
    write_image(root, "val", 8, 23)
    cfg = json.load(open(root / "model_configs" / "mpp" / "config_mpp_log.json"))
    cfg["inference"]["rjmcmc_params"].update(burn_in=2500, alpha_t=0.998, init_temperature=0.2)
    with open(root / "cfg.json", "w") as f:
        json.dump(cfg, f)
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "-p", "infer", "-m", "mpp", "-c", str(root / "cfg.json"),
                        "-d", "SYNTH", "-o", "--restarts", "3", "--recombine"], cwd=root, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stderr.splitlines() if "recombine: " in ln and "taken from another replica, energy -" in ln]
    assert len(lines) == 2, r.stderr[-3000:]
    found = 0
    for k in (7, 8):
        files = [p for p in glob.glob(str(root / "data" / "inference" / "SYNTH" / "val" / "*" / f"{k:04}_results.pkl"))
                 if os.path.basename(os.path.dirname(p)) not in ("posvec_dota", "shape_dota")]
        assert len(files) == 1, files
        with open(files[0], "rb") as f:
            record = pickle.load(f)
        s = record["recombine"]
        assert set(s) == {"status", "n_clusters", "n_taken", "E_winner", "E_after"}
        assert len(s["status"]) == 4 and len(record["detection_score"]) > 20      # a 300 x 420 image: four tiles
        assert set(s["status"].tolist()) <= {0, 1, 2} and np.all(s["n_taken"] <= s["n_clusters"])
        assert np.all((s["status"] == 1) == ((s["n_taken"] > 0) & (s["status"] != 2)))
        keep = s["status"] != 1
        assert same_bits(s["E_after"][keep], s["E_winner"][keep])
        assert f"recombine: {int(s['n_taken'].sum())} of {int(s['n_clusters'].sum())} cluster(s) in " in r.stderr
        found += int(np.count_nonzero(s["status"] == 1))
    assert found > 0                                             # (a dataset in which the option changes something)
