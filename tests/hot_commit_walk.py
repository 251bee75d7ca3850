"""A host walk of the hot start's commit loop (csrc/mpp_chain_body.inc, the ``par_commit`` branch of ``mpp_hot_kernel``)
over a trace of the sequential chain: which steps of a round of eight speculative steps commit, under the rule that ends
the round with an accepted birth or death (``past=False``) and under the one that goes on past it (``past=True``,
MPP_HOT_PAST / option ``hot_past_births``).

What the walk knows of a step is what the trace holds: its kernel type, its target INDEX and added pixel in the sequential
chain, its decision and the population after it.  The walk keeps the sequential state from those -- order[] as the kernel
keeps it (a birth takes the next index, the last index takes a death's hole), and every point's pixel -- and forms a round's
records against the state at the round's start: a record's speculative target is ``order[mulhi32(w2, n)]`` there.  ``w2``
(Philox word 2 of the step) is not traced: ``target_words`` draws one per step from the interval that gives the traced index,
``philox_target_words`` computes the steps' own words (the oracle's Philox), with which the walk's rounds are the kernel's.

A record that commits is treated as the sequential step (its traced decision and pixel are applied).  That is what the commit
rule has to guarantee, so ``walk`` checks it for every record either rule lets through, from the sequentially tracked state:
the record's speculative target is the sequential one, and no point changed earlier in the round shares a cell with one of
its points or lies within ``conflict_d2`` of it.  (The pixel a record with a wrong target would add is unknown to the
walk; the traced one stands in.  Such a record never passes: the commit that changed order[] re-draws its target.)
Apply rounds (a stash overflow) and capacity stops are not modelled."""
import numpy as np

BIRTHS, DEATHS = (0, 2), (1, 3)           # MPP_K_UBIRTH, MPP_K_DBIRTH / MPP_K_UDEATH, MPP_K_DDEATH
SPEC = 8


def oracle_trace(tile, n_obj, n_steps, seed, T0=1.0, alpha=0.999, points=None, setup_name="legacy"):
    """the sequential chain of a synthetic tile from its naive initialisation (or `points` = (xy, marks)), as the bench and
    tests/test_gpu_chain.py's setup_case build it -> (proposals, step records, initial pixels, cell size, conflict_d2)"""
    import oracle
    from helpers import model_for
    from mpp_cnn_rs_object_detection_amd import kernels, mappings, synth
    t = synth.make_tile(tile, n_obj, tile_id=0)
    setup, _, model = model_for(setup_name)
    o = oracle.Oracle(t.shape, t.det, t.marks, model, kernels.make_kernels(mappings.default_mappings(), 1.0))
    xy, marks = o.naive_detection(setup.detection_threshold, 6.0)
    o = oracle.Oracle(t.shape, t.det, t.marks, model, kernels.make_kernels(mappings.default_mappings(), max(1, len(xy))))
    if points is not None:
        xy, marks = points
    o.set_points(xy, marks)
    o.set_temperature(T0, alpha, 0.0)
    out, props = o.run(n_steps, seed, chain=0, trace=True)
    max_inter = max([p[4] for p in model.pair] or [1.0])
    return props, out, np.asarray(xy).reshape(-1, 2), int(max(max_inter, 32.0)), int(4.0 * max_inter * max_inter) + 1


def philox_target_words(n_steps, seed, chain=0, step0=0):
    """the steps' own target words: word 2 of Philox block 0 (counter: step, block, chain; key: seed), as the kernels draw it"""
    import oracle
    key = [seed & 0xffffffff, seed >> 32]
    return np.array([oracle.philox([s & 0xffffffff, s >> 32, 0, chain], key)[2] for s in range(step0, step0 + n_steps)],
                    dtype=np.uint64)


def mulhi32(a, n):
    return (int(a) * int(n)) >> 32


def target_words(props, out, n0, rng):
    """one 32-bit word per step: uniform among those with mulhi32(word, n before the step) == the traced target index"""
    n_before = np.concatenate([[n0], out["n_after"][:-1]]).astype(np.int64)
    w = rng.integers(0, 1 << 32, size=len(props), dtype=np.uint64)
    t = props["target"].astype(np.int64)
    for i in np.nonzero((t >= 0) & (n_before > 0))[0]:
        n = int(n_before[i])
        lo, hi = -((-int(t[i]) << 32) // n), -((-(int(t[i]) + 1) << 32) // n) - 1        # ceil(t 2^32 / n) .. ceil((t+1) 2^32 / n) - 1
        w[i] = rng.integers(lo, hi + 1, dtype=np.uint64)
        assert mulhi32(w[i], n) == t[i]
    return w


def walk(props, out, xy0, w2, past, res=32, conflict_d2=4097, handover_at=0, n_steps=None, check=True):
    """-> dict(rounds, steps (walked), handover (step at which ho_ema reached handover_at, or None), bd_per_round (list:
    births / deaths committed in each round), kinds (per round: its committed births and deaths in order, e.g. "db"),
    n_start (per round: the population it started with), checked (records verified))"""
    kern, targ, acc = props["kernel"], props["target"], out["accepted"]
    ax, ay = props["ax"], props["ay"]
    N = len(props) if n_steps is None else n_steps
    order = list(range(len(xy0)))
    pos = {i: (int(p[0]), int(p[1])) for i, p in enumerate(xy0)}
    next_id = len(xy0)
    cell = lambda p: (p[0] // res, p[1] // res)

    def near(p, q):
        return cell(p) == cell(q) or (p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 <= conflict_d2

    s, rounds, ho_ema, ho_rounds, handover, checked = 0, 0, 0, 0, None, 0
    bd_per_round, kinds, n_start = [], [], []
    while s < N:
        lim = min(SPEC, N - s)
        n = len(order)
        recs = []                               # (has_rem, has_add, slot, removed pixel, added pixel) against the round's start
        for i in range(lim):
            k = int(kern[s + i])
            if k in BIRTHS:
                recs.append((False, True, None, None, (int(ax[s + i]), int(ay[s + i]))))
            elif n == 0:
                recs.append((False, False, None, None, None))
            else:
                slot = order[mulhi32(w2[s + i], n)]
                recs.append((True, k not in DEATHS, slot, pos[slot], (int(ax[s + i]), int(ay[s + i])) if k not in DEATHS else None))
        ok = [True] * lim
        changed = []                            # pixels changed by this round's commits
        committed, first_bd, n_bd, kind = lim, -1, 0, ""
        for w in range(lim):
            if not ok[w]:
                committed = w
                break
            hr, ha, slot, rp, ap = recs[w]
            st = s + w
            if check:                           # the record is taken for the sequential step: is it?
                if hr:
                    assert 0 <= targ[st] < len(order) and order[targ[st]] == slot, (st, "target")
                else:
                    assert targ[st] < 0 and (ha or len(order) == 0), (st, "no target")
                for p in ([rp] if hr else []) + ([ap] if ha else []):
                    assert not any(near(p, q) for q in changed), (st, "a point changed within reach")
                checked += 1
            if not (acc[st] and (hr or ha)):
                continue
            if hr and ha:                       # move / transform: same slot
                pos[slot] = ap
                pts = [rp, ap]
            elif hr:                            # death: the last index takes the hole
                t = order.index(slot)
                order[t] = order[-1]
                order.pop()
                del pos[slot]
                pts = [rp]
                kind += "d"
            else:                               # birth: the next index
                order.append(next_id)
                pos[next_id] = ap
                next_id += 1
                pts = [ap]
                kind += "b"
            changed += pts
            bd = not (hr and ha)
            if bd:
                n_bd += 1
                if first_bd < 0:
                    first_bd = w + 1
                if not past:
                    committed = w + 1
                    break
            for o in range(w + 1, lim):         # which later records are still trustworthy?
                if not ok[o]:
                    continue
                ohr, oha, oslot, orp, oap = recs[o]
                bad = False
                if bd:
                    if ohr:
                        bad = len(order) == 0 or order[mulhi32(w2[s + o], len(order))] != oslot
                    elif not oha:
                        bad = True              # drawn at n == 0
                else:
                    bad = ohr and oslot == slot
                for p in ([orp] if ohr else []) + ([oap] if oha else []):
                    bad = bad or any(near(p, q) for q in pts)
                if bad:
                    ok[o] = False
        s += committed
        rounds += 1
        bd_per_round.append(n_bd)
        kinds.append(kind)
        n_start.append(n)
        if handover_at and handover is None:
            d = ((first_bd if first_bd >= 0 else committed) << 8) - ho_ema
            ho_ema += abs(d) // 16 * (1 if d >= 0 else -1)      # (C's division: towards zero)
            ho_rounds += 1
            if ho_rounds >= 48 and ho_ema >= handover_at:
                handover = s
                break
    return dict(rounds=rounds, steps=s, handover=handover, bd_per_round=bd_per_round, kinds=kinds, n_start=n_start,
                checked=checked)
