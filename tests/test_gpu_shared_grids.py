"""The chains' candidate grids live in one workspace of the context (``grids_ws``, ``chain_grids_build`` in ``csrc/mpp_ctx.hpp``)
that every pass over all chains rebuilds right before it reads them, and ``mpp_birth_complete`` runs the descent's round loop in
the descent's workspace.  So calls that used to own their grids now follow each other through the same memory: every call of a
sequence on ONE context has to give, byte for byte, what the same call gives on a fresh context that made only that call.  No
tolerance anywhere: the kernels and their inputs are the same.

Small on purpose: the 40 x 48 tile and the twelve points of ``test_gpu_birth_map``, beside them a chain of 70 points so that
``merge_score`` (grids from 64 points on, whatever the option says) takes its grids too; 96 x 96 tiles where the workspace has
to grow."""
import numpy as np
import pytest

from mpp_cnn_rs_object_detection_amd import mappings
from test_gpu_birth_map import POINT_MARKS, POINTS, H, W, make_ctx, model_desc, tile_maps
from test_gpu_descent import MODELS

pytestmark = pytest.mark.gpu


def many_points(n=70, seed=3):
    """n distinct pixels of the small tile with marks taken in turn from POINT_MARKS"""
    pix = np.random.default_rng(seed).choice(H * W, n, replace=False)
    return np.stack([pix // W, pix % W], axis=1).astype(np.int32), POINT_MARKS[np.arange(n) % len(POINT_MARKS)]


def points_blob(ctx):
    return [a.tobytes() for pair in ctx.get_points_all() for a in pair]


def birth_map(ctx):
    dE, marks, summary = ctx.birth_energy_map(marks=True)
    return [dE.cpu().numpy().tobytes(), marks.cpu().numpy().tobytes(), summary.tobytes()]


def merge(ctx):
    tiles, removed = ctx.merge_score(4.0)                        # (two of POINTS lie 3 px apart)
    assert int(removed.sum()) > 0
    return [a.tobytes() for t in tiles for a in t] + [removed.tobytes()] + points_blob(ctx)


def descend(ctx):
    rep, src = ctx.descend(what=3, max_rounds=16, src=True)
    assert int(rep["n_removed"].sum()) > 0
    return [rep.tobytes(), src.tobytes()] + points_blob(ctx)


def complete(ctx):
    rep = ctx.birth_complete(max_rounds=16)
    assert int(rep["n_added"].sum()) > 0
    return [rep.tobytes()] + points_blob(ctx)


# (name, the call's result as a list of bytes, whether it changes the points)
SEQUENCE = [("total_energy_all", lambda c: [c.total_energy_all().tobytes()], False),
            ("birth_energy_map", birth_map, False),
            ("papangelou_all", lambda c: [c.papangelou_all().tobytes()], False),
            ("merge_score", merge, True),
            ("descend", descend, True),
            ("birth_complete", complete, True),
            ("total_energy_all again", lambda c: [c.total_energy_all().tobytes()], False)]


def small_state(name, grid_min):
    """a factory of contexts of two chains on the small tile -- POINTS and the 70 points -- and the function that puts the
    points (back)"""
    _, _, desc = model_desc(name)
    det, marks = tile_maps()
    xy70, mk70 = many_points()

    def put(ctx):
        ctx.set_points(0, POINTS, POINT_MARKS)
        ctx.set_points(1, xy70, mk70)

    def fresh():
        ctx = make_ctx(desc, det, marks, replicas=2, point_capacity=128)
        ctx.set_option("scratch_grid_min_points", grid_min)
        put(ctx)
        return ctx
    return desc, fresh, put


def large_state(desc, grid_min):
    """the same for six chains on three 96 x 96 tiles: more chains and more cells than the small state has"""
    maps3 = [tile_maps((96, 96), seed=30 + k) for k in range(3)]
    det, marks = np.stack([m[0] for m in maps3]), [np.stack([m[1][k] for m in maps3]) for k in range(3)]

    def put(ctx):
        for c in range(6):
            ctx.set_points(c, POINTS + 8 * c, POINT_MARKS)

    def load(ctx):
        ctx.set_maps(det, marks)
        ctx.set_model(desc, mappings.default_mappings())
        assert ctx.get_option("n_chains") == 6
        put(ctx)

    def fresh():
        ctx = make_ctx(desc, det, marks, replicas=2, point_capacity=128)
        ctx.set_option("scratch_grid_min_points", grid_min)
        put(ctx)
        return ctx
    return fresh, put, load


def assert_same_as_fresh(ctx, fresh, put, calls, what):
    for call, run, changes in calls:
        got = run(ctx)
        alone = fresh()
        want = run(alone)
        alone.close()
        print(f"{what}, {call}: {len(want)} arrays, {sum(len(b) for b in want)} bytes")
        assert len(got) == len(want) and all(g == w for g, w in zip(got, want)), (what, call)
        if changes:
            put(ctx)


@pytest.mark.parametrize("grid_min", [1, 0])
@pytest.mark.parametrize("name", MODELS)
def test_a_sequence_on_one_context_equals_fresh_contexts(name, grid_min):
    desc, fresh, put = small_state(name, grid_min)
    ctx = fresh()
    assert ctx.counts().tolist() == [len(POINTS), 70]
    assert_same_as_fresh(ctx, fresh, put, SEQUENCE, f"{name}, scratch_grid_min_points {grid_min}")
    assert ctx.get_option("birth_map_grid") == (1 if grid_min else 0)
    # larger tiles and more chains: the grids' workspace has to grow under the same context
    fresh_large, put_large, load = large_state(desc, grid_min)
    load(ctx)
    assert_same_as_fresh(ctx, fresh_large, put_large, [SEQUENCE[0], SEQUENCE[4]], f"{name}, {grid_min}, after set_maps")
    ctx.close()


def test_recombine_between_a_birth_map_and_papangelou_all():
    _, _, desc = model_desc("mpp_log")
    det, marks = tile_maps()

    def fresh(points=None):
        ctx = make_ctx(desc, det, marks, replicas=2, point_capacity=64)
        ctx.set_option("scratch_grid_min_points", 1)
        if points is None:                                           # two replicas that differ: each lacks what the other has
            points = [(POINTS[:8], POINT_MARKS[:8]), (POINTS[4:], POINT_MARKS[4:])]
        for c, (xy, mk) in enumerate(points):
            ctx.set_points(c, xy, mk)
        return ctx
    ctx = fresh()
    birth_map(ctx)
    rep, src = ctx.recombine(src=True)
    after = ctx.get_points_all()
    p = ctx.papangelou_all()
    print("recombine: " + ", ".join(f"{k} {rep[0][k]!r}" for k in rep.dtype.names))
    alone = fresh()
    rep1, src1 = alone.recombine(src=True)
    assert rep.tobytes() == rep1.tobytes() and src.tobytes() == src1.tobytes()
    assert points_blob(ctx) == points_blob(alone)
    alone.close()
    alone = fresh(after)
    assert p.tobytes() == alone.papangelou_all().tobytes() and np.any(p != 0.0)
    alone.close()
    ctx.close()
