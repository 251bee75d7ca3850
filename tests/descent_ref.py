"""The standard of the local descent's tests: the selection rule among points as a plain double loop, the states the
tests start from, and the host walk.

The walk is composed only of calls older than ``mpp_descend``: ``ctx.papangelou(tile)`` -> the loop's selection ->
``ctx.set_points(survivors)`` for the death half, ``ctx.birth_energy_map(marks=True)`` -> ``select_minima_ref`` ->
``ctx.set_points(old + new)`` for the birth half, repeated.  It is what a user could do before the device loop existed, and
what the device loop has to reproduce bit for bit."""
import numpy as np

from birth_complete_ref import numpy_summary, select_minima_ref

NO_MAP = (0.0, -1, -1, 0, 0)          # the map fields of a report when no map is computed (births off)


def select_points_ref(xy, values, above, distance):
    """``mpp_select_points`` as a plain double loop.  xy [n,2] integers, values [n] float64.  Returns (keep [n] uint8,
    n_candidates).

    candidate: values[i] > above (a NaN never, +inf is); key (-values[i], i); kept iff no OTHER candidate j with
    (double)(dx*dx + dy*dy) <= distance * distance has a smaller key."""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    n, d2 = len(values), float(distance) * float(distance)
    pts = [(int(xy[i, 0]), int(xy[i, 1]), float(values[i])) for i in range(n)]     # (plain numbers: the loop is Python's)
    cand = [i for i in range(n) if pts[i][2] > above]
    keep = np.zeros(n, np.uint8)
    for i in cand:
        xi, yi, vi = pts[i]
        ok = True
        for j in cand:
            xj, yj, vj = pts[j]
            if j == i or float((xj - xi) * (xj - xi) + (yj - yi) * (yj - yi)) > d2:
                continue
            if vj > vi or (vj == vi and j < i):
                ok = False
                break
        keep[i] = 1 if ok else 0
    return keep, len(cand)


def select_points_definition(xy, values, above, distance):
    """The same answer from the definition with arrays: a candidate is kept iff its key is the smallest among the candidates of
    the disc around it (the CPU test holds the loop above against this)."""
    xy = np.asarray(xy, dtype=np.int64).reshape(-1, 2)
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    n = len(values)
    with np.errstate(invalid="ignore"):
        is_cand = values > above
    d = xy[:, None, :] - xy[None, :, :]
    near = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float64) <= float(distance) * float(distance)
    slot = np.arange(n)
    with np.errstate(invalid="ignore"):
        better = (values[None, :] > values[:, None]) | ((values[None, :] == values[:, None]) & (slot[None, :] < slot[:, None]))
    beaten = np.any(near & is_cand[None, :] & better & (slot[None, :] != slot[:, None]), axis=1)
    return (is_cand & ~beaten).astype(np.uint8), int(is_cand.sum())


def papangelou_summary(p):
    """(max_p, slot_max, n_positive) of a chain's Papangelou values, as ``mpp_descent_report`` defines them"""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    ok = ~np.isnan(p)
    if not ok.any():
        return (-np.inf, -1, 0)
    i = int(np.argmax(np.where(ok, p, -np.inf)))             # the first of equal values
    return (float(p[i]), i, int(np.sum(p[ok] > 0)))


def death_walk(papangelou_of, xy, marks, max_inter, max_rounds=16, min_gain=0.0):
    """The death half alone, round after round, on any source of values: ``papangelou_of(xy, marks)`` -> float64 [n].
    Returns a dict: xy, marks (the survivors in slot order), src, status, rounds, n_removed, gain_deaths, per_round (the
    (slots, xy, values) each round removed, slots in the round's own numbering)."""
    xy, marks = np.asarray(xy, np.int32).reshape(-1, 2), np.asarray(marks, np.float64).reshape(-1, 3)
    src, gain, rounds, per_round = np.arange(len(xy)), 0.0, 0, []
    while True:
        p = papangelou_of(xy, marks) if len(xy) else np.zeros(0)
        keep, _ = select_points_ref(xy, p, float(min_gain), 2.0 * float(max_inter))
        gone = np.flatnonzero(keep)
        if len(gone) == 0:
            status = 0
            break
        for s in gone:                                       # one after another, in slot order
            gain = gain + float(p[s])
        per_round.append((gone, xy[gone], p[gone]))
        stay = keep == 0
        xy, marks, src = xy[stay], marks[stay], src[stay]
        rounds += 1
        if rounds >= max_rounds:
            status = 1
            break
    return dict(xy=xy, marks=marks, src=src, status=status, rounds=rounds, n_removed=sum(len(g[0]) for g in per_round),
                gain_deaths=gain, per_round=per_round)


def host_walk(ctx, tile, max_inter, what=3, max_rounds=16, min_gain=0.0):
    """The descent of chain ``tile`` of ``ctx`` by the host walk; the chain's configuration is changed through ``set_points``.
    Returns a dict: xy, marks (the final configuration in slot order), src (per final slot the slot at the start, -1 for a born
    point), status, rounds, n_added, n_removed, n_after, gain_births, gain_deaths (sequential float64 sums), removed / added
    (per round that changed the chain: the (xy, values) removed and appended, either possibly empty), papangelou (max_p,
    slot_max, n_positive of a fresh pass over the final state), summary (``numpy_summary`` of a fresh map of the final state;
    ``NO_MAP`` when births are off)."""
    cap = ctx.get_option("point_capacity")
    deaths, births = bool(what & 1), bool(what & 2)
    xy, mk = ctx.get_points(tile)
    xy, mk = xy.astype(np.int32).reshape(-1, 2), mk.astype(np.float64).reshape(-1, 3)
    src = np.arange(len(xy))
    gb, gd, rounds, n_added, n_removed, removed, added = 0.0, 0.0, 0, 0, 0, [], []
    empty = (np.zeros((0, 2), np.int32), np.zeros(0))
    while True:
        changed, full, rem, add = False, False, empty, empty
        if deaths:
            p = ctx.papangelou(tile)
            keep, _ = select_points_ref(xy, p, float(min_gain), 2.0 * float(max_inter))
            gone = np.flatnonzero(keep)
            if len(gone):
                for s in gone:                               # one after another, in slot order
                    gd = gd + float(p[s])
                rem = (xy[gone], p[gone])
                stay = keep == 0
                xy, mk, src = xy[stay], mk[stay], src[stay]
                ctx.set_points(tile, xy, mk)
                n_removed, changed = n_removed + len(gone), True
        if births:
            dE, cand, _ = ctx.birth_energy_map(marks=True)     # (with the summary: the call waits for the map)
            d, c = dE[tile].cpu().numpy(), cand[tile].cpu().numpy()
            kxy, kv, _ = select_minima_ref(d, -float(min_gain), 2.0 * float(max_inter))
            if len(xy) + len(kxy) > cap:
                full = True
            elif len(kxy):
                for v in kv:
                    gb = gb + float(v)
                add = (kxy, kv)
                xy = np.concatenate([xy, kxy]).astype(np.int32)
                mk = np.concatenate([mk, c[kxy[:, 0], kxy[:, 1]]])
                src = np.concatenate([src, np.full(len(kxy), -1)])
                ctx.set_points(tile, xy, mk)
                n_added, changed = n_added + len(kxy), True
        if changed:
            rounds += 1
            removed.append(rem)
            added.append(add)
        if full:
            status = 2
        elif not changed:
            status = 0
        elif rounds >= max_rounds:
            status = 1
        else:
            continue
        break
    summary = numpy_summary(ctx.birth_energy_map()[0][tile].cpu().numpy()) if births else NO_MAP
    return dict(xy=xy, marks=mk, src=src.astype(np.int32), status=status, rounds=rounds, n_added=n_added, n_removed=n_removed,
                n_after=len(xy), gain_births=gb, gain_deaths=gd, removed=removed, added=added,
                papangelou=papangelou_summary(ctx.papangelou(tile)), summary=summary)


def state_d(render_maps, make_gt):
    """State (d): a 96 x 96 tile with 20 rendered objects and 50 points -- the 20 objects, the same 20 shifted by (+1, +2)
    and clipped to the tile with the same marks, and 10 points on the 10 lowest detection pixels (stable argsort) with marks
    (6.0, 0.5, 0.4).  Returns (det, marks, xy, point marks)."""
    gt_xy, gt_marks = make_gt(96, 20, tile_id=31)
    det, marks = render_maps((96, 96), gt_xy, gt_marks, noise=0.2, noise_seed=9)
    shifted = np.clip(gt_xy + np.array([1, 2]), 0, 95)
    low = np.argsort(det.reshape(-1), kind="stable")[:10]
    xy = np.concatenate([gt_xy, shifted, np.stack([low // 96, low % 96], axis=1)]).astype(np.int32)
    mk = np.concatenate([gt_marks, gt_marks, np.tile([6.0, 0.5, 0.4], (10, 1))]).astype(np.float64)
    return det, marks, xy, mk
