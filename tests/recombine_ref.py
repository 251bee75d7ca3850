"""NumPy restatement of rules 2-10 of ``mpp_recombine`` (include/mpp_hip.h): from the replicas' points and their per-point
energies to the winner, the clusters, the per-cluster choice, the composite, the status, the report and ``src``.

Independent of the device code in method: union-find for the clusters, explicit slot-order loops in Python floats (IEEE
float64, one rounding per addition) for every sum.  ``E_after`` needs the energy model and is not computed here: it is the
winner's energy for status 0 and 2 and ``None`` for status 1."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

REPORT_FIELDS = ("status", "winner", "n_clusters", "n_taken", "n_before", "n_after", "E_winner", "E_sum")


def slot_sum(values) -> float:
    """the values added one after another, in order, to a float64 that starts at 0.0"""
    s = 0.0
    for v in np.asarray(values, dtype=np.float64).tolist():
        s = s + v
    return s


def better(candidate: float, best: float) -> bool:
    """rules 2 and 6: strictly lower, or finite where the best so far is not"""
    return candidate < best or (not math.isfinite(best) and math.isfinite(candidate))


def select_winner(energies: Sequence[float]) -> int:
    w = 0
    for r in range(1, len(energies)):
        if better(float(energies[r]), float(energies[w])):
            w = r
    return w


def linked(dx: int, dy: int, max_inter: float) -> bool:
    """rule 3, in float64: sqrt(dx*dx + dy*dy) <= max_inter"""
    dx, dy = np.float64(int(dx)), np.float64(int(dy))
    return bool(np.sqrt(dx * dx + dy * dy) <= np.float64(max_inter))


class _UnionFind:
    def __init__(self, n: int):
        self.parent = list(range(n))

    def find(self, a: int) -> int:
        while self.parent[a] != a:
            self.parent[a] = self.parent[self.parent[a]]
            a = self.parent[a]
        return a

    def union(self, a: int, b: int):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)


def recombine_tile(xy: Sequence[np.ndarray], e: Sequence[np.ndarray], cap: int, max_inter: float,
                   energies: Optional[Sequence[float]] = None) -> dict:
    """One tile.  ``xy[r]`` int [n_r, 2] and ``e[r]`` float64 [n_r]: replica r's points and their energies in slot order;
    ``energies[r]``: its chain energy (default: ``slot_sum(e[r])``, which is what the device forms).  Returns the report's
    fields, ``cluster`` (per replica, the cluster id ``r * cap + slot`` of every point), ``choice`` {cluster id: replica},
    ``S`` {cluster id: [S[r] for r]}, ``kept`` [(replica, slot)] in composite order (whatever the status) and ``src`` int32
    [cap, 2] as rule 10 states it."""
    R = len(xy)
    xy = [np.asarray(a, dtype=np.int64).reshape(-1, 2) for a in xy]
    e = [np.asarray(a, dtype=np.float64).reshape(-1) for a in e]
    counts = [len(a) for a in xy]
    assert all(len(e[r]) == counts[r] <= cap for r in range(R))
    energies = [slot_sum(e[r]) for r in range(R)] if energies is None else [float(v) for v in energies]
    w = select_winner(energies)

    members = [(r, s) for r in range(R) for s in range(counts[r])]            # ascending global index r * cap + slot
    uf = _UnionFind(len(members))
    pos = np.concatenate(xy).astype(np.float64).reshape(-1, 2)                # (the predicate of ``linked``, a row at a time)
    for a in range(len(members) - 1):
        dx, dy = pos[a + 1:, 0] - pos[a, 0], pos[a + 1:, 1] - pos[a, 1]
        for b in np.nonzero(np.sqrt(dx * dx + dy * dy) <= np.float64(max_inter))[0].tolist():
            uf.union(a, a + 1 + b)
    gid = [r * cap + s for r, s in members]
    root = [gid[uf.find(a)] for a in range(len(members))]                      # (the union keeps the smaller index as root)
    cluster = [np.zeros(counts[r], np.int64) for r in range(R)]
    for (r, s), c in zip(members, root):
        cluster[r][s] = c

    ids = sorted(set(root))
    S, choice = {c: [0.0] * R for c in ids}, {}
    for r in range(R):
        for s, (c, v) in enumerate(zip(cluster[r].tolist(), e[r].tolist())):   # ascending slot order, from 0.0
            S[c][r] = S[c][r] + v
    for c in ids:
        sums = S[c]
        best = w
        for r in range(R):
            if r != w and better(sums[r], sums[best]):
                best = r
        choice[c] = best
    n_taken = sum(1 for c in ids if choice[c] != w)
    E_sum = 0.0
    for c in ids:                                                              # ascending cluster id, from 0.0
        E_sum = E_sum + S[c][choice[c]]

    kept = [(r, s) for r in [w] + [q for q in range(R) if q != w] for s in range(counts[r]) if choice[int(cluster[r][s])] == r]
    status = 0 if n_taken == 0 else (2 if len(kept) > cap else 1)
    final = kept if status == 1 else [(w, k) for k in range(counts[w])]
    src = np.full((cap, 2), -1, np.int32)
    if final:
        src[:len(final)] = np.asarray(final, dtype=np.int32)
    return {"status": status, "winner": w, "n_clusters": len(ids), "n_taken": n_taken, "n_before": counts[w],
            "n_after": len(final), "E_winner": energies[w], "E_sum": E_sum,
            "E_after": None if status == 1 else energies[w],
            "cluster": cluster, "choice": choice, "S": S, "kept": kept, "src": src}


def recombine_ref(points: Sequence, e_rows: np.ndarray, n_tiles: int, replicas: int, cap: int, max_inter: float,
                  energies: Optional[np.ndarray] = None) -> List[dict]:
    """Every tile of a context: ``points[c]`` = (xy, marks) of chain c = r * n_tiles + i (``MppContext.get_points_all``),
    ``e_rows`` [n_chains, cap] (``MppContext.point_energies_all``), ``energies`` [n_chains] or None.  One dict per tile, as
    ``recombine_tile`` returns it, plus ``xy`` / ``marks`` of the chain the call leaves at the winner's place."""
    out = []
    for i in range(n_tiles):
        chains = [r * n_tiles + i for r in range(replicas)]
        xy = [np.asarray(points[c][0]).reshape(-1, 2) for c in chains]
        marks = [np.asarray(points[c][1], dtype=np.float64).reshape(-1, 3) for c in chains]
        t = recombine_tile(xy, [np.asarray(e_rows[c])[:len(points[c][0])] for c in chains], cap, max_inter,
                           None if energies is None else [energies[c] for c in chains])
        k = t["n_after"]
        t["xy"] = np.array([xy[r][s] for r, s in t["src"][:k]], dtype=np.int32).reshape(-1, 2)
        t["marks"] = np.array([marks[r][s] for r, s in t["src"][:k]], dtype=np.float64).reshape(-1, 3)
        out.append(t)
    return out


def same_bits(a, b) -> bool:
    """float64 equality by bit pattern, every NaN equal to every NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.uint64) == b.view(np.uint64))))
