"""Reports that outlive the deep round they were made in (host side: no GPU is used here).

A queue round of the deep-round kernel ends at the first report a committed change makes untrustworthy; the reports behind it
that no committed change conflicts with are the reports the next round would write again, and with the option ``deep_carry``
the kernel keeps them (csrc/mpp_commit.hpp, ``carry_keeps``; csrc/mpp_deep.hip, phase C).  ``walk`` takes the oracle's trace
of a chain through deep rounds of adaptive depth under a simplified commit rule -- a committed move / transform conflicts
with a later step on the same slot, with one whose points lie within the longest interaction range of its own, and, when it crosses a cell
border, with one in the cells around; an accepted birth or death ends the round; no neighbour words, no ``DI_RESC`` /
``DI_NBOV``, no queue cut -- and counts the rounds by how they end, the steps of their windows and the steps evaluated
afresh when non-changing, unconflicted reports are kept.  The distance test with the full range for every pair is harsher
than ``commit_conflict`` (which asks how far the two rectangles reach), and the same for a round's end and for keeping:
the walk's rounds are close to the kernel's, not equal to them.

``CASES`` are the chains of tests/test_gpu_deep_carry.py; tests/test_carry_cases_host.py holds each of them to floors counted
here, so that no case compares two runs that never keep a report or never lose one."""
from __future__ import annotations

import functools

import numpy as np

import same_value_cases as sv
from mpp_cnn_rs_object_detection_amd import kernels

K = kernels
BIRTHS, DEATHS = (K.K_UBIRTH, K.K_DBIRTH), (K.K_UDEATH, K.K_DDEATH)
WAVES = 8
ENDS = ("slot", "distance", "cell", "birth_death", "none")


def walk(props, out, xy0, mk0, first=0, res=32, range2=1024, nmax=128, gain8=12, fixed=0):
    """-> dict(rounds, window_steps, fresh, ends={how: rounds}, kept_twice, kept_lost) over the steps from `first` on.
    fresh: window steps without a kept report; kept_twice: reports kept over two or more round ends; kept_lost: kept
    reports a later round's commit conflicts with (they are evaluated again after all)"""
    kern, targ, acc = props["kernel"], props["target"], out["accepted"]
    order = list(range(len(xy0)))
    val = {i: (int(xy0[i][0]), int(xy0[i][1]), float(mk0[i][0]), float(mk0[i][1]), float(mk0[i][2])) for i in range(len(xy0))}
    next_id = len(order)
    new_of = lambda st: (int(props["ax"][st]), int(props["ay"][st]), float(props["as"][st]), float(props["ar"][st]), float(props["aa"][st]))
    cell = lambda p: (p[0] // res, p[1] // res)

    def apply(st):
        """the sequential step st on the tracked state"""
        nonlocal next_id
        k, t = int(kern[st]), int(targ[st])
        if not acc[st]:
            return
        if k in BIRTHS:
            order.append(next_id); val[next_id] = new_of(st); next_id += 1
        elif t >= 0:
            if k in DEATHS:
                slot = order[t]
                order[t] = order[-1]; order.pop(); del val[slot]
            else:
                val[order[t]] = new_of(st)

    for st in range(first):
        apply(st)
    N = len(props)
    s, depth, ema16 = first, WAVES, WAVES * 16
    res_ = dict(rounds=0, window_steps=0, fresh=0, ends={k: 0 for k in ENDS}, kept_twice=0, kept_lost=0)
    kept = {}                                   # step -> round ends it has outlived
    while s < N:
        lim = min(fixed if fixed > 0 else depth, nmax, N - s)
        recs = []                               # (has_rem, has_add, slot, points, changing, birth / death) against the round's start
        past_bd = False                         # behind an accepted birth / death the traced targets are indices of another n:
        for i in range(lim):                    # the round ends there at the latest, and nothing behind it is kept
            st = s + i
            k, t = int(kern[st]), int(targ[st])
            if past_bd:
                recs.append((False, False, None, [], False, False))
                continue
            past_bd = bool(acc[st]) and (k in BIRTHS or (k in DEATHS and t >= 0))
            if k in BIRTHS:
                ap = new_of(st)
                recs.append((False, True, None, [ap[:2]], bool(acc[st]), True))
            elif t < 0:
                recs.append((False, False, None, [], False, False))
            else:
                slot = order[t]
                old = val[slot]
                if k in DEATHS:
                    recs.append((True, False, slot, [old[:2]], bool(acc[st]), True))
                else:
                    new = new_of(st)
                    recs.append((True, True, slot, [old[:2], new[:2]], bool(acc[st]) and new != old, False))
        res_["rounds"] += 1
        res_["window_steps"] += lim
        res_["fresh"] += sum(1 for i in range(lim) if s + i not in kept)
        why = [None] * lim                      # why a report is no longer trustworthy
        committed, how = lim, "none"
        for w in range(lim):
            if why[w] is not None:
                committed, how = w, why[w]
                break
            hr, ha, slot, pts, chg, bd = recs[w]
            if not chg:
                continue
            if bd:
                committed, how = w + 1, "birth_death"
                break
            crosses = cell(pts[0]) != cell(pts[1])
            for o in range(w + 1, lim):
                if why[o] is not None:
                    continue
                ohr, oha, oslot, opts, _, _ = recs[o]
                if ohr and oslot == slot:
                    why[o] = "slot"
                elif any((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 <= range2 for p in opts for q in pts):
                    why[o] = "distance"
                elif crosses and any(abs(cell(p)[0] - cell(q)[0]) <= 1 and abs(cell(p)[1] - cell(q)[1]) <= 1 for p in opts for q in pts):
                    why[o] = "cell"
        res_["ends"][how] += 1
        # the kept reports of the next round (carry_keeps): behind the end, not the report the round ended at, unchanging,
        # no conflict with a change that committed (why[] holds exactly those: every changing step below the end committed)
        now = {}
        for o in range(committed, lim):
            st = s + o
            keep = how != "birth_death" and not (o == committed and how != "none") and not recs[o][4] and why[o] is None
            if keep:
                now[st] = kept.get(st, 0) + 1
                if now[st] == 2:
                    res_["kept_twice"] += 1
            elif st in kept and why[o] is not None:
                res_["kept_lost"] += 1
        kept = now
        for st in range(s, s + committed):
            apply(st)
        s += committed
        ema16 += committed - (ema16 >> 4)
        want = ((ema16 * gain8) >> 7) + WAVES
        want = (want + WAVES - 1) // WAVES * WAVES
        depth = max(WAVES, min(nmax, want))
    assert len(order) == int(out["n_after"][-1])
    return res_


def bench_chain_walk(n_steps=100001, first=2694):
    """the chain bench.py times (512 x 512, 200 objects, seed 0), from the step at which its hot start hands over"""
    import hot_commit_walk as hw
    import oracle
    from helpers import model_for
    from mpp_cnn_rs_object_detection_amd import mappings, synth
    props, out, xy0, res, d2 = hw.oracle_trace(512, 200, n_steps, seed=0, T0=1.0, alpha=0.999)
    t = synth.make_tile(512, 200, tile_id=0)
    setup, _, model = model_for("legacy")
    o = oracle.Oracle(t.shape, t.det, t.marks, model, kernels.make_kernels(mappings.default_mappings(), 1.0))
    _, mk0 = o.naive_detection(setup.detection_threshold, 6.0)
    return walk(props, out, xy0, np.asarray(mk0).reshape(-1, 3), first, res, (d2 - 1) // 4)


# ---- the GPU cases: chains of tests/same_value_cases.py (its builders; the transform-heavy mixture re-targets a slot often)
CASES = ["tile112", "packed", "empty", "capacity", "hot-start"]
FLOORS = dict(slot=50, distance=20, kept_twice=10, kept_lost=5)


def geometry(b):
    """cell size and longest interaction range (squared) of the case's model, as the library derives them"""
    max_inter = max([p[4] for p in b.model.pair] or [1.0])
    return int(max(max_inter, 32.0)), int(max_inter * max_inter)


@functools.lru_cache(maxsize=None)
def case_walk(name):
    b = sv.build(name)
    out, props, _ = sv.oracle_chain(name)
    res, d2 = geometry(b)
    return walk(props, out, b.xy, b.mk, 0, res, d2)
