"""The standard of the greedy completion's tests: the selection rule in numpy and the host walk.

The walk is composed only of calls older than ``mpp_birth_complete``: ``ctx.birth_energy_map(marks=True)`` -> ``.cpu()`` ->
the numpy selection -> ``ctx.set_points(old + new)``, repeated.  It is what a user could do before the device loop existed,
and what the device loop has to reproduce bit for bit."""
import numpy as np


def select_minima_ref(dE, below, distance):
    """``mpp_select_minima`` as a plain double loop over the candidates.  dE [H,W] float64.  Returns (xy [k,2] int32,
    values [k] float64, n_candidates), the kept pixels in ascending row-major order.

    candidate: dE < below (a NaN never, -inf is); key (dE, x * W + y); kept iff no OTHER candidate with
    (double)(dx*dx + dy*dy) <= distance * distance has a smaller key."""
    dE = np.asarray(dE, dtype=np.float64)
    H, W = dE.shape
    d2 = float(distance) * float(distance)
    with np.errstate(invalid="ignore"):
        cand = np.argwhere(dE < below)                      # row-major order
    pts = [(int(x), int(y), float(dE[x, y]), int(x) * W + int(y)) for x, y in cand]       # (plain numbers: the loop is Python's)
    kept = []
    for a, (xa, ya, va, ia) in enumerate(pts):
        ok = True
        for xb, yb, vb, ib in pts:
            if ib == ia or float((xb - xa) * (xb - xa) + (yb - ya) * (yb - ya)) > d2:
                continue
            if vb < va or (vb == va and ib < ia):
                ok = False
                break
        if ok:
            kept.append(a)
    xy = cand[kept].astype(np.int32).reshape(-1, 2)
    return xy, dE[xy[:, 0], xy[:, 1]].astype(np.float64), int(len(cand))


def select_minima_definition(dE, below, distance):
    """The same set from the definition, without a list of candidates: a candidate is kept iff its key is the smallest among
    the candidates of the whole disc around it (arrays over all pixels; the CPU test holds the loop above against this)."""
    dE = np.asarray(dE, dtype=np.float64)
    H, W = dE.shape
    with np.errstate(invalid="ignore"):
        is_cand = dE < below
    X, Y = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    flat = X * W + Y
    d2 = float(distance) * float(distance)
    kept = []
    for x, y in np.argwhere(is_cand):
        inside = ((X - x) ** 2 + (Y - y) ** 2).astype(np.float64) <= d2
        rivals = inside & is_cand & (flat != x * W + y)
        v = dE[x, y]
        beaten = np.any(rivals & ((dE < v) | ((dE == v) & (flat < x * W + y))))
        if not beaten:
            kept.append((x, y))
    xy = np.array(kept, dtype=np.int32).reshape(-1, 2)
    return xy, dE[xy[:, 0], xy[:, 1]].astype(np.float64), int(is_cand.sum())


def numpy_summary(dE):
    """(min_dE, x, y, n_negative, n_nan) of a map, as ``mpp_birth_summary`` defines them"""
    flat = np.asarray(dE, dtype=np.float64).reshape(-1)
    ok = ~np.isnan(flat)
    if not ok.any():
        return (np.inf, -1, -1, 0, int(flat.size))
    i = int(np.argmin(np.where(ok, flat, np.inf)))          # the first of equal values
    return (float(flat[i]), i // dE.shape[1], i % dE.shape[1], int(np.sum(flat[ok] < 0)), int(np.sum(~ok)))


def host_walk(ctx, tile, max_inter, max_rounds=16, min_gain=0.0):
    """Greedy completion of chain ``tile`` of ``ctx`` by the host walk; the chain's configuration is changed through
    ``set_points``.  Returns a dict: xy, marks (the final configuration in slot order), status, rounds, n_added, n_after,
    gain (the sequential float64 sum), per_round (the (xy, values) each round appended), summary (``numpy_summary`` of a
    fresh map of the final state)."""
    cap = ctx.get_option("point_capacity")
    xy, mk = ctx.get_points(tile)
    xy, mk = xy.astype(np.int32).reshape(-1, 2), mk.astype(np.float64).reshape(-1, 3)
    n0, gain, rounds, per_round = len(xy), 0.0, 0, []
    while True:
        dE, cand, _ = ctx.birth_energy_map(marks=True)         # (with the summary: the call waits for the map)
        d, c = dE[tile].cpu().numpy(), cand[tile].cpu().numpy()
        kxy, kv, _ = select_minima_ref(d, -float(min_gain), 2.0 * float(max_inter))
        if len(kxy) == 0:
            status = 0
            break
        if len(xy) + len(kxy) > cap:
            status = 2
            break
        for v in kv:                                         # one after another, in slot order
            gain = gain + float(v)
        xy = np.concatenate([xy, kxy]).astype(np.int32)
        mk = np.concatenate([mk, c[kxy[:, 0], kxy[:, 1]]])
        ctx.set_points(tile, xy, mk)
        rounds += 1
        per_round.append((kxy, kv))
        if rounds >= max_rounds:
            status = 1
            d = ctx.birth_energy_map()[0][tile].cpu().numpy()
            break
    return dict(xy=xy, marks=mk, status=status, rounds=rounds, n_added=len(xy) - n0, n_after=len(xy), gain=gain,
                per_round=per_round, summary=numpy_summary(d))
