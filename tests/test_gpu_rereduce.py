"""rereduce_wave (csrc/mpp_chain.hpp), the one re-reduction that eval_delta<FAST> and the deep round's deep_delta share: a
neighbour u loses the point that carried its overlap maximum or its alignment minimum, the added rectangle does not take
over, and the whole wave re-reduces u over its own 3 x 3 cells.  The crowd tapes of test_gpu_overlap_exact.py reach it
only incidentally; here the cases are built on purpose, at the smallest shapes where the function can still go wrong.

Model F (overlap / max over 32 px, alignment / min over 16 px: the FAST class), 32-px cells.  Three configurations:
  direct      a 96-px tile (3 x 3 cells), no cell with more than 3 points: lane 3k+e reads entry e of cell k;
  flattened   the same tile with 7 points in u's cell, 12 in its 3 x 3 block: the flattened index space, one turn of 64;
  two turns   a 32-px tile, one cell with 68 points: two turns, the eight cells around it lie outside the grid
              (cell2 = -1), and the points that become u's new extrema are entries 66 and 67, i.e. of the second turn.
In each, R carries both extrema of u; P carries the overlap maximum and Q the alignment minimum once R is gone.  One tape
(ctx.replay, u_accept = 1e-300, every step accepted) does four things, in the order in which one tape can do them:
  0  a translation of R to where its overlap with u is smaller but not zero, its alignment value unchanged: the added
     rectangle does not take over pair 0, pair 0 alone is re-reduced;
  1  a rotation-free move of R onto u's own pixel with other marks (long and thin: a smaller overlap again): inside the
     re-reduction the order of u and the added rectangle is a tie on the coordinates, decided by the marks (slot_first);
  2  the death of R (no added rectangle): both pairs are re-reduced;
  3  the death of Q: only the alignment minimum is lost.
Every |dE - exact| is within the tolerance of overlap_ref.step_delta (area_bound carried through the energy, not fitted),
and dE, n_after and the final points are byte-identical between spec_waves 1, spec_waves 8 and chain_state 2.

Before anything is launched the inputs are checked on the CPU with the reference alone: at every step the value dE would
have if u kept its old extremum -- the exact dE plus u's energy with the old reductions minus u's energy with the new ones
-- differs from the exact dE by more than 1000 tolerances, also for each re-reduced pair on its own.  A re-reduction that is
skipped or wrong cannot pass.

The deep round takes no tape: test_deep_rounds_re_reduce_as_the_sequential_chain runs a crowded tile and counts, from the
oracle's walk of the trace, the steps that take away a point carrying a neighbour's extremum."""
import numpy as np
import pytest

import oracle
import overlap_cases as OC
import overlap_ref as R
from helpers import model_for
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings, synth

pytestmark = pytest.mark.gpu

ANGLE = 0.3                      # of u; R is 0.02 off it, Q 0.1, P 0.5, the fillers a quarter turn


def _tape(rows, r_slot, q_slot, r_moved, r_on_u):
    """(tape, configurations [5], pairs re-reduced per step): the four steps of the module's docstring"""
    tape = np.zeros(4, hip_api.PROPOSAL_DTYPE)
    cur = [np.array(r, np.float64) for r in rows]
    configs = [np.array(cur)]
    for k, new in enumerate((r_moved, r_on_u)):
        new = np.array(new, np.float64)
        step = new[:2] - cur[r_slot][:2]
        tape[k]["kernel"], tape[k]["target"] = kernels.K_GTRANS, r_slot
        tape[k]["ax"], tape[k]["ay"], tape[k]["as"], tape[k]["ar"], tape[k]["aa"] = int(new[0]), int(new[1]), new[2], new[3], new[4]
        tape[k]["aux0"], tape[k]["aux1"] = float(step[0]), float(step[1])
        cur[r_slot] = new
        configs.append(np.array(cur))
    assert q_slot == len(cur) - 1                            # the death of R moves the last point, Q, into R's slot
    for k in (2, 3):
        tape[k]["kernel"], tape[k]["target"] = kernels.K_UDEATH, r_slot
        cur[r_slot] = cur[-1]
        cur.pop()
        configs.append(np.array(cur))
    tape["u_accept"] = 1e-300
    return tape, configs, [(0,), (0,), (0, 1), (1,)]


def _config(name):
    """(tile size, cell capacity, rows, tape, configurations, re-reduced pairs).  Row 0 is u, row 1 is R; P and Q are the
    last two rows, behind the fillers: the last entries of their cells."""
    if name == "two turns":
        tile, cell_cap, ux, uy = 32, 128, 15, 15
        # 64 fillers of 2 x 1 px on the border rows and columns of the tile: their circumscribed circles stay clear of u's
        ring = [(x, y) for x in range(0, 32, 2) for y in (1, 3, 28, 30)]
        fillers = [OC.rect(x, y, 2.0, 1.0, ANGLE + OC.PI / 2 + 0.01 * k) for k, (x, y) in enumerate(ring)]
        assert len(fillers) == 64
    else:
        tile, cell_cap, ux, uy = 96, 32, 60, 48
        fillers = []
        if name == "flattened":                               # four more in u's cell (7 there), three in the cell above
            spots = [(36, 36), (38, 52), (44, 40), (50, 60), (20, 40), (25, 50), (28, 44)]
            fillers = [OC.rect(x, y, 4.0, 2.0, ANGLE + OC.PI / 2 + 0.02 * k) for k, (x, y) in enumerate(spots)]
    u = OC.rect(ux, uy, 12.0, 6.0, ANGLE)
    r = OC.rect(ux + 2, uy + 1, 10.0, 5.0, ANGLE + 0.02)
    p = OC.rect(ux - 5, uy + 5, 10.0, 4.0, ANGLE + 0.5)
    q = OC.rect(ux + 10, uy - 3, 8.0, 4.0, ANGLE + 0.1) if tile == 96 else OC.rect(ux + 9, uy - 4, 6.0, 3.0, ANGLE + 0.1)
    r_moved = OC.rect(ux + 3, uy + 1, 10.0, 5.0, ANGLE + 0.02)
    r_on_u = OC.rect(ux, uy, 28.0, 1.0, ANGLE + 0.02)
    rows = [u, r] + fillers + [p, q]
    tape, configs, lost = _tape(rows, 1, len(rows) - 1, r_moved, r_on_u)
    return tile, cell_cap, np.array(rows, np.float64), tape, configs, lost


CONFIGS = ["direct", "flattened", "two turns"]
_CASES = {}


def case(name):
    """the configuration with its exact steps [(dE, tol)], computed once"""
    if name not in _CASES:
        tile, cell_cap, rows, tape, configs, lost = _config(name)
        model = OC.model_f()
        exact = [R.step_delta(configs[k], configs[k + 1], model)[:2] for k in range(len(tape))]
        _CASES[name] = (tile, cell_cap, rows, tape, configs, lost, model, exact)
    return _CASES[name]


def check_inputs(name):
    """the conditions on the inputs, with the reference alone; returns the smallest |stale dE - exact dE| / tolerance"""
    tile, cell_cap, rows, tape, configs, lost, model, exact = case(name)
    cells = {}
    for x, y in rows[:, :2].astype(int):
        assert 0 <= x < tile and 0 <= y < tile
        cells[(x // 32, y // 32)] = cells.get((x // 32, y // 32), 0) + 1
    ci, cj = int(rows[0, 0]) // 32, int(rows[0, 1]) // 32
    block = sum(n for (i, j), n in cells.items() if abs(i - ci) <= 1 and abs(j - cj) <= 1)
    if name == "direct":
        assert max(cells.values()) <= 3
    elif name == "flattened":
        assert max(cells.values()) >= 4 and block <= 64
    else:
        assert block >= 65 and tile == 32                     # one cell: all eight cells around it are outside the grid
    nu = len(model.unit)
    coef = [pt[3] for pt in model.pair]
    p0 = model.pair[1][5][0]
    smallest = np.inf
    for k in range(len(tape)):
        before, after = configs[k], configs[k + 1]
        vb, _ = R.point_vectors(before, model, only=[0])
        va, _ = R.point_vectors(after, model, only=[0])          # u is row 0 before and after every step
        assert before[0].tobytes() == after[0].tobytes() == rows[0].tobytes()
        gone = before[1]                                      # what the step takes away: the point in slot 1
        assert not any(gone.tobytes() == a.tobytes() for a in after)
        added = after[1] if tape[k]["kernel"] == kernels.K_GTRANS else None
        carried = (R.overlap(before[0], gone), R.align(before[0], gone, p0))
        dE, tol = exact[k]
        for p in (0, 1):
            if p in lost[k]:
                # the point taken away carried u's extremum, and neither the added rectangle nor anyone else restores it
                assert vb[0, nu + p] == carried[p] and carried[p] != 0.0, (name, k, p)
                if added is not None:
                    v_add = R.overlap(before[0], added) if p == 0 else R.align(before[0], added, p0)
                    assert (v_add < carried[p]) if p == 0 else (v_add > carried[p]), (name, k, p)
                assert abs(coef[p] * (vb[0, nu + p] - va[0, nu + p])) > 1000.0 * tol, (name, k, p, vb[0], va[0], tol)
            else:
                assert vb[0, nu + p] == va[0, nu + p], (name, k, p)   # the other pair keeps its value: it is not re-reduced
        stale = dE + float(R.combine(vb[0], model)[0]) - float(R.combine(va[0], model)[0])
        assert abs(stale - dE) > 1000.0 * tol, (name, k, stale, dE, tol)
        smallest = min(smallest, abs(stale - dE) / tol)
    # step 1: u and the added rectangle share the pixel, their marks differ
    assert np.array_equal(configs[2][1][:2], rows[0, :2]) and not np.array_equal(configs[2][1][2:], rows[0, 2:])
    return smallest


@pytest.mark.parametrize("name", CONFIGS)
def test_replayed_re_reductions(name):
    smallest = check_inputs(name)                             # on the CPU, before anything is launched
    tile, cell_cap, rows, tape, configs, lost, model, exact = case(name)
    results, worst = [], 0.0
    for spec, state in ((1, 1), (8, 1), (1, 2)):
        ctx = hip_api.MppContext(0, point_capacity=256, cell_capacity=cell_cap, spec_waves=spec, chain_state=state, deep=0)
        ctx.set_maps(np.zeros((tile, tile), np.float32), [np.zeros((tile, tile, 32), np.float32)] * 3)
        ctx.set_model(model, mappings.default_mappings())
        assert (ctx.get_option("spec_waves"), ctx.get_option("chain_state"), ctx.get_option("grid_res")) == (spec, state, 32)
        assert ctx.get_option("grid_nx") == ctx.get_option("grid_ny") == tile // 32
        ctx.set_kernels(kernels.make_kernels(mappings.default_mappings(), 1.0))
        ctx.set_points(0, rows[:, :2].astype(np.int32), rows[:, 2:])
        ctx.set_schedule(1e12, 1.0, 0.0)
        out = ctx.replay(0, tape)
        assert ctx.get_option("hbm_chains") == (1 if state == 2 else 0)
        assert np.all(out["accepted"] == 1)
        for k in range(len(tape)):
            dE, tol = exact[k]
            print(f"{name}, spec {spec} state {state}, step {k}: dE {out['dE'][k]!r}, exact {dE!r}, tolerance {tol:.3g}")
            worst = max(worst, abs(out["dE"][k] - dE) / tol)
            assert abs(out["dE"][k] - dE) <= tol, (name, spec, state, k, out["dE"][k], dE, tol)
            assert out["n_after"][k] == len(configs[k + 1])
        gxy, gm = ctx.get_points()
        final = configs[-1]
        assert np.array_equal(gxy, final[:, :2].astype(np.int32)) and gm.tobytes() == np.ascontiguousarray(final[:, 2:]).tobytes()
        results.append((out["dE"].tobytes(), out["n_after"].tobytes(), gxy.tobytes(), gm.tobytes()))
        ctx.close()
    assert results[0] == results[1] == results[2]
    print(f"{name}: largest |dE - exact| / tolerance = {worst:.3g}; a stale extremum is off by at least {smallest:.3g} tolerances")


# ---- the deep round ---------------------------------------------------------------------------------------------------------
DEEP_STEPS, DEEP_SEED, DEEP_T0, DEEP_ALPHA = 2000, 12, 0.05, 0.999    # (the oracle alone: 1206 such steps, 24 points left)


def deep_case():
    """the crowded 96-px tile of the soak (test_gpu_chain.py, case 1): every object of the start twice, shifted by (3, 2)"""
    t = synth.make_tile(96, 45, tile_id=101, noise=0.2)
    setup, comb, model = model_for("legacy")
    o = oracle.Oracle(t.shape, t.det, t.marks, model, kernels.make_kernels(mappings.default_mappings(), 1.0))
    xy, mk = o.naive_detection(setup.detection_threshold, 6.0)
    kd = kernels.make_kernels(mappings.default_mappings(), max(1, len(xy)))
    xy = np.concatenate([xy, np.clip(xy + np.array([3, 2]), 0, 95)]).astype(np.int32)
    mk = np.concatenate([mk, mk])
    return t, model, kd, xy, mk


def count_lost_extrema(t, model, kd, xy, mk, props, accepted):
    """evaluated steps that take away a point which carries the overlap maximum or the alignment minimum of a neighbour: the
    pair's value, as the oracle computes it for the two of them alone, equals the neighbour's reduction (float64 equality,
    as the device decides it) and is not 0"""
    nu = len(model.unit)
    assert [(p[0], p[2]) for p in model.pair] == [(0, 0), (1, 1)]            # overlap / max, alignment / min
    walker = oracle.Oracle(t.shape, t.det, t.marks, model, kd)
    two = oracle.Oracle(t.shape, t.det, t.marks, model, kd)
    walker.set_points(xy, mk)
    memo = {}

    def pair_values(a, b):
        key = a.tobytes() + b.tobytes()
        if key not in memo:
            two.set_points(np.array([a[:2], b[:2]], np.int32), np.array([a[2:], b[2:]]))
            memo[key] = two.total_energy(return_vectors=True)[1][0, nu:nu + 2].copy()
        return memo[key]

    count = 0
    one = np.ones(1, np.int32)
    for i in range(len(props)):
        bxy, bm = walker.get_points()
        target = int(props["target"][i])
        if props["kernel"][i] not in (kernels.K_UBIRTH, kernels.K_DBIRTH) and 0 <= target < len(bxy):
            _, vec = walker.total_energy(return_vectors=True)
            pts = np.concatenate([bxy.astype(np.float64), bm], axis=1)
            d2 = ((bxy - bxy[target]) ** 2).sum(axis=1)
            hit = False
            for j in np.nonzero(d2 <= 32 * 32)[0]:
                if j != target:
                    v = pair_values(pts[j], pts[target])
                    hit = hit or any(v[p] != 0.0 and v[p] == vec[j, nu + p] for p in (0, 1))
            count += hit
        if accepted[i]:
            walker.replay_forced(props[i:i + 1], one)
    return count


def test_deep_rounds_re_reduce_as_the_sequential_chain():
    t, model, kd, xy, mk = deep_case()
    runs = []
    for spec, deep, fixed in ((1, 0, 0), (8, 128, 96)):
        ctx = hip_api.MppContext(0, point_capacity=512, spec_waves=spec, deep=deep)
        ctx.set_option("deep_fixed", fixed)
        ctx.set_maps(t.det, t.marks)
        ctx.set_model(model, mappings.default_mappings())
        ctx.set_kernels(kd)
        ctx.set_points(0, xy, mk)
        ctx.set_schedule(DEEP_T0, DEEP_ALPHA, 0.0)
        out, props = ctx.run(DEEP_STEPS, DEEP_SEED, trace_tile=0)
        assert (ctx.get_option("spec_waves"), ctx.get_option("deep"), ctx.get_option("deep_fixed")) == (spec, deep, fixed)
        st = ctx.deep_stats()
        assert st["committed"] == (DEEP_STEPS if deep else 0), st
        runs.append((out, props, ctx.get_points()))
        ctx.close()
    (out1, props1, (xy1, m1)), (outd, propsd, (xyd, md)) = runs
    assert out1.tobytes() == outd.tobytes() and props1.tobytes() == propsd.tobytes()
    assert xy1.tobytes() == xyd.tobytes() and m1.tobytes() == md.tobytes()
    n = count_lost_extrema(t, model, kd, xy, mk, props1, out1["accepted"])
    print(f"deep rounds: {n} of {DEEP_STEPS} evaluated steps take away a point that carries a neighbour's extremum")
    assert n >= 30
