"""The exchange rule of parallel tempering (include/mpp_hip.h: mpp_run_tempered), stated in NumPy.

A context holds R replicas of each of n tiles; chain ``r * n + i`` is replica r of tile i.  ``rung[chain]`` is the chain's
place on its tile's temperature ladder, ``sched[chain]`` its (current T, alpha, T_target).  The exchange at absolute step
``s`` with exchanges every ``every`` steps is number ``e = s // every``:

* pairs ``(k, k + 1)`` with ``k + 1 < R``; R = 2 attempts its only pair at every exchange, R > 2 those with ``k % 2 == e % 2``;
* a / b: the chains of the tile on rungs k / k + 1; ``d = (1 / Ta - 1 / Tb) * (Ea - Eb)`` in float64;
* ``u = u53(w[0], w[1])``, ``w = Philox4x32-10(ctr = (lo32(s), hi32(s), 0x80000000 | k, chain id), key = seed)`` with the chain
  id and seed of replica 0 of the tile;
* accept iff Ta > 0, Tb > 0, both energies finite and (d >= 0 or u < exp(d)); an accepted pair swaps its two schedule
  triples and its two rungs.
"""
import numpy as np

from mpp_cnn_rs_object_detection_amd import hip_api

RECORD_DTYPE = np.dtype([("step", "<i8"), ("tile", "<i4"), ("k", "<i4"), ("chain_a", "<i4"), ("chain_b", "<i4"),
                         ("accepted", "<i4"), ("Ea", "<f8"), ("Eb", "<f8"), ("Ta", "<f8"), ("Tb", "<f8"), ("u", "<f8"),
                         ("d", "<f8")])


def u53(a: int, b: int) -> float:
    """the 53-bit uniform in [0, 1) the chains form from two Philox words"""
    return float(((int(a) >> 5) << 26) | (int(b) >> 6)) * (1.0 / 9007199254740992.0)


def pairs_of(R: int, e: int):
    """the lower rungs k of the pairs (k, k + 1) that exchange number e attempts, ascending"""
    if R == 2:
        return [0]
    return [k for k in range(R - 1) if k % 2 == e % 2]


def ladder(T0: float, alpha: float, T_target: float, ratio: float, R: int, n: int):
    """-> (sched [R * n, 3], rung [R * n]) as mpp_set_ladder sets them: f_r by repeated multiplication in float64"""
    sched, f = np.zeros((R * n, 3), np.float64), np.float64(1.0)
    for r in range(R):
        if r > 0:
            f = f * np.float64(ratio)
        sched[r * n:(r + 1) * n] = (np.float64(T0) * f, alpha, np.float64(T_target) * f)
    return sched, np.repeat(np.arange(R, dtype=np.int32), n)


def draw(s: int, k: int, chain_id: int, seed: int) -> float:
    w = hip_api.philox([s & 0xffffffff, (s >> 32) & 0xffffffff, 0x80000000 | k, chain_id & 0xffffffff],
                       [seed & 0xffffffff, (seed >> 32) & 0xffffffff])
    return u53(w[0], w[1])


def decide(Ea, Eb, Ta, Tb, u):
    """-> (accepted, d), for scalars or arrays alike.  All float64; exp is NumPy's."""
    Ea, Eb, Ta, Tb = (np.asarray(v, dtype=np.float64) for v in (Ea, Eb, Ta, Tb))
    with np.errstate(all="ignore"):
        d = (np.float64(1.0) / Ta - np.float64(1.0) / Tb) * (Ea - Eb)
        ok = (Ta > 0) & (Tb > 0) & np.isfinite(Ea) & np.isfinite(Eb) & ((d >= 0) | (np.asarray(u) < np.exp(d)))
    return ok, d


def exchange(sched, rung, energy, s: int, every: int, n: int, R: int, keys, draw_fn=draw):
    """One exchange at absolute step s, in place on ``sched`` [R * n, 3] and ``rung`` [R * n].  ``keys`` = (seeds [n],
    chain ids [n]) of replica 0 of every tile.  -> the records in (tile, pair) order."""
    e = s // every
    out = []
    for i in range(n):
        for k in pairs_of(R, e):
            chains = np.arange(R) * n + i
            a, b = int(chains[rung[chains] == k][0]), int(chains[rung[chains] == k + 1][0])
            Ea, Eb, Ta, Tb = energy[a], energy[b], sched[a, 0], sched[b, 0]
            u = draw_fn(s, k, int(keys[1][i]), int(keys[0][i]))
            ok, d = decide(Ea, Eb, Ta, Tb, u)
            if ok:
                sched[[a, b]] = sched[[b, a]]
                rung[a], rung[b] = k + 1, k
            out.append((s, i, k, a, b, int(ok), Ea, Eb, Ta, Tb, u, float(d)))
    return np.array(out, dtype=RECORD_DTYPE)
