"""A plain restatement of the dedupe rule of ``merge_patches(method='distance')`` (reference data_loaders.py:140-159, as
``data_loaders.distance_merge`` and DESIGN.md document it): an O(n^2) numpy walk, no KD-tree, no code shared with the
package.  The device merge (``mpp_merge_score``) and the host walk are both tested against it."""
import numpy as np


def _near(xy, i, distance):
    """indices within ``distance`` of point i, itself included: sqrt(dx^2 + dy^2) <= distance in float64 on the integer
    coordinates (the squares are formed in int64, exact for any coordinate a support can hold)"""
    d = xy - xy[i]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float64)) <= float(distance)


def _decisions(xy, scores, distance):
    """-> (removed mask, [(i, near, best)]): the walk, and every decision it takes (``near``: the not-yet-removed points
    within the distance of i when its turn comes, ascending; ``best``: the one of them that is kept)."""
    xy = np.asarray(xy).astype(np.int64).reshape(-1, 2)
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    n = len(xy)
    assert len(scores) == n
    removed = np.zeros(n, dtype=bool)
    taken = []
    for i in range(n):
        if removed[i]:
            continue
        near = np.nonzero(_near(xy, i, distance) & ~removed)[0]
        if len(near) <= 1:                              # alone within the distance: skipped
            continue
        sc = scores[near]
        top = np.max(sc)                                # (NaN if any score is NaN)
        if np.isfinite(top):
            best = near[np.nonzero(sc >= top - 1e-9 * abs(top))[0][0]]
        else:
            best = near[int(np.argmax(sc))]             # a NaN first, else the first infinity
        removed[near] = True
        removed[best] = False
        taken.append((i, near, int(best)))
    return removed, taken


def walk(xy, scores, distance) -> np.ndarray:
    """mask of the points the merge removes"""
    return _decisions(xy, scores, distance)[0]


def compact(xy, marks, removed):
    """The survivors in the order ``EPointsSet.remove`` leaves them: the removals go in ascending index, each moves the
    last point of the list into the hole.  -> (xy, marks, order) with ``order[k]`` = original index of survivor k."""
    xy, marks = np.asarray(xy).reshape(-1, 2), np.asarray(marks).reshape(-1, 3)
    order = list(range(len(xy)))
    slot = {k: k for k in order}
    for k in np.nonzero(np.asarray(removed, dtype=bool))[0]:
        k = int(k)
        s = slot.pop(k)
        last = order.pop()
        if last != k:
            order[s] = last
            slot[last] = s
    order = np.array(order, dtype=np.int64)
    return xy[order], marks[order], order


def decision_margins(xy, scores, distance):
    """For every decision of the walk: (i, best, losers, gaps) with ``gaps[k] = (top - score[losers[k]]) / |top|``, the
    relative distance of each losing candidate to the best score of its neighbourhood (NaN where a score involved is not
    finite).  An input whose gaps are all either large or those of constructed duplicates gives the same decisions under
    any scoring that agrees to less than the gap."""
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    out = []
    for i, near, best in _decisions(xy, scores, distance)[1]:
        losers = near[near != best]
        top = np.max(scores[near])
        with np.errstate(invalid="ignore", divide="ignore"):
            gaps = (top - scores[losers]) / abs(top)
        out.append((i, best, losers, gaps))
    return out
