"""The standard of the relocation's tests: state (m), the selection distance, and the host walk.

The walk is composed of calls that existed before ``mpp_relocate`` plus ``move_gains``: ``ctx.move_gains(radius)`` ->
``select_points_ref`` with the relocation's distance -> ``host_candidate_marks`` at the kept points' target pixels ->
``ctx.set_points(edited list)``, repeated, with sequential float64 sums.  It is what the device loop has to reproduce bit for
bit."""
import numpy as np

from descent_ref import papangelou_summary, select_points_ref

# state (m): the five objects of the 40 x 48 tile, each shifted by these offsets, the angle increased by 0.4
M_SHIFTS = np.array([[2, -1], [-1, 2], [1, 1], [-2, -2], [0, 2]], dtype=np.int32)
M_ANGLE = 0.4


def state_m(gt_xy, gt_marks):
    xy = (np.asarray(gt_xy, np.int32) + M_SHIFTS).astype(np.int32)
    mk = np.array(gt_marks, dtype=np.float64)
    mk[:, 2] += M_ANGLE
    return xy, mk


def distance(max_inter, radius):
    """2 * (max_inter + radius * sqrt(2)), float64: what two points moved in one round have to exceed"""
    return 2.0 * (float(max_inter) + float(radius) * float(np.sqrt(np.float64(2.0))))


def window_pixels(v, radius, shape):
    """the pixels of the (2 radius + 1)^2 window around v clipped to the tile, row-major"""
    xs = [x for x in range(int(v[0]) - radius, int(v[0]) + radius + 1) if 0 <= x < shape[0]]
    ys = [y for y in range(int(v[1]) - radius, int(v[1]) + radius + 1) if 0 <= y < shape[1]]
    return np.array([[x, y] for x in xs for y in ys], dtype=np.int32).reshape(-1, 2)


def shifted_scene(S=160, n_objects=24, radius=2, seed=3):
    """A S x S tile with rendered objects, every object shifted by a seeded offset within the radius, the objects' marks kept.
    Returns (det, marks, xy, point marks)."""
    from mpp_cnn_rs_object_detection_amd import synth
    gt_xy, gt_marks = synth.make_gt(S, n_objects, tile_id=47)
    det, marks = synth.render_maps((S, S), gt_xy, gt_marks, noise=0.2, noise_seed=13)
    rng = np.random.default_rng(seed)
    xy = np.clip(gt_xy + rng.integers(-radius, radius + 1, gt_xy.shape), 0, S - 1).astype(np.int32)
    return det, marks, xy, np.array(gt_marks, dtype=np.float64)


def walk_bound(n, K, B):
    """What E(before) - E(after) and the booked gain of K moves in a chain of n points may differ by.  Each total is a sum of n
    point energies of magnitude at most B / 2 (error at most g(n) n B / 2 each); each booked gain is a sum of at most n + 1
    terms of magnitude at most B (error at most g(n + 1) (n + 1) B in any order); their sequential sum of K values of
    magnitude at most (n + 1) B adds g(K) K (n + 1) B.  g(m) = (m - 1) u / (1 - (m - 1) u), u = 2^-53.  The point energies
    themselves are the same bits on both sides."""
    u = 2.0 ** -53
    g = lambda m: max(m - 1, 0) * u / (1.0 - max(m - 1, 0) * u)
    return g(n) * n * B + K * g(n + 1) * (n + 1) * B + g(K) * K * (n + 1) * B


def host_walk(ctx, tile, max_inter, cand, radius=2, max_rounds=16, min_gain=0.0):
    """The relocation of chain ``tile`` of ``ctx`` by the host walk; the chain's configuration is changed through
    ``set_points``.  ``cand`` [H,W,3]: ``host_candidate_marks`` of the tile's mark maps.  Returns a dict: xy, marks (the final
    configuration), moved (per slot), status, rounds, n_moved, gain (sequential float64 sum), per_round (the (slots, from, to,
    gains) of every round that moved something), summary ((max_gain, slot_max, n_positive) of a fresh gain pass)."""
    xy, mk = ctx.get_points(tile)
    xy, mk = xy.astype(np.int32).reshape(-1, 2).copy(), mk.astype(np.float64).reshape(-1, 3).copy()
    n = len(xy)
    moved, gain, rounds, n_moved, per_round = np.zeros(n, np.int32), 0.0, 0, 0, []
    dist = distance(max_inter, radius)
    while True:
        g, to = ctx.move_gains(radius)
        g, to = g[tile, :n], to[tile, :n]
        keep, _ = select_points_ref(xy, g, float(min_gain), dist)
        idx = np.flatnonzero(keep)
        if len(idx) == 0:
            status = 0
            break
        for s in idx:                                        # one after another, in slot order
            gain = gain + float(g[s])
        per_round.append((idx, xy[idx].copy(), to[idx].copy(), g[idx].copy()))
        xy[idx] = to[idx]
        mk[idx] = cand[to[idx, 0], to[idx, 1]]
        moved[idx] += 1
        ctx.set_points(tile, xy, mk)
        rounds, n_moved = rounds + 1, n_moved + len(idx)
        if rounds >= max_rounds:
            status = 1
            break
    g = ctx.move_gains(radius)[0][tile, :n]
    return dict(xy=xy, marks=mk, moved=moved, status=status, rounds=rounds, n_moved=n_moved, gain=gain, per_round=per_round,
                summary=papangelou_summary(g))
