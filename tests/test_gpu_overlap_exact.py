"""Every device implementation of the rectangle clipper against exact rational geometry (tests/overlap_ref.py) on the
pair families of tests/overlap_cases.py: collinear edges, identical rectangles, a vertex on an edge, octagons, slivers.

  clip_area          from-scratch kernels (total_energy, delta_batch, papangelou), grid pass and scan pass, and k_quad_iou
  clip_area_wave     one wave per step: replayed tapes at spec_waves 1 and 8, and with the chain's state in device memory
  clip_area_lds      lane mode (spec_lanes 4 and 8): lanes that need a clip take turns on CLIP_SLOTS = 4 buffers
  clip_area_groups   deep rounds on a tile where nearly every proposal lands on an occupied place

Every tolerance is overlap_ref.area_bound (41 eps M^2, derived there) carried through the energy; none is fitted.  Each
test prints the largest |device - exact| / tolerance it saw (pytest -s); profiles/overlap_tests.md keeps the figures."""
import time

import numpy as np
import pytest

import oracle
import overlap_cases as OC
import overlap_ref as R
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings
from oracle import voc_eval

pytestmark = pytest.mark.gpu

TILE = 512
_ZEROS = {}


def zero_maps(tile=TILE):
    if tile not in _ZEROS:
        _ZEROS[tile] = (np.zeros((tile, tile), np.float32), [np.zeros((tile, tile, 32), np.float32)] * 3)
    return _ZEROS[tile]


def make_ctx(model, cap=512, **kw):
    ctx = hip_api.MppContext(0, point_capacity=cap, **kw)
    ctx.set_maps(*zero_maps())
    ctx.set_model(model, mappings.default_mappings())
    return ctx


def pack(pairs, spacing):
    """groups of pairs such that any two points of different pairs of a group are at least ``spacing`` px apart: every pair
    is its own neighbourhood (max_dist is 32).  Greedy, first fit, in the families' order."""
    groups = []
    for a, b in pairs:
        pa = np.array([a[:2], b[:2]], np.float64)
        for g in groups:
            if np.min(np.hypot(g["xy"][:, None, 0] - pa[None, :, 0], g["xy"][:, None, 1] - pa[None, :, 1])) >= spacing:
                break
        else:
            g = dict(pairs=[], xy=np.zeros((0, 2)))
            groups.append(g)
        g["pairs"].append((a, b))
        g["xy"] = np.concatenate([g["xy"], pa])
    return [g["pairs"] for g in groups]


def rows(pairs):
    return np.array([r for p in pairs for r in p], np.float64)


def set_rows(ctx, pts):
    ctx.set_points(0, pts[:, :2].astype(np.int32), pts[:, 2:])


# ---- from scratch: clip_area ---------------------------------------------------------------------------------------------
def check_vectors(ctx, pts, model, worst, label):
    """total_energy(return_vectors=True) with the scan pass and with the grid pass: same bits, overlap column within bound"""
    set_rows(ctx, pts)
    ctx.set_option("scratch_grid_min_points", 0)
    assert ctx.get_option("scratch_grid_min_points") == 0                    # no candidate grid: every point scans all
    e_scan, v_scan = ctx.total_energy(return_vectors=True)
    ctx.set_option("scratch_grid_min_points", 1)
    assert ctx.get_option("scratch_grid_min_points") == 1                    # the grid from the first point on
    e_grid, v_grid = ctx.total_energy(return_vectors=True)
    assert v_scan.tobytes() == v_grid.tobytes() and e_scan == e_grid, label
    vec, tol = R.point_vectors(pts, model)
    col = len(model.unit)
    err = np.abs(v_scan[:, col] - vec[:, col])
    bad = np.nonzero(err > tol)[0]
    assert len(bad) == 0, (label, pts[bad[:4]], v_scan[bad[:4], col], vec[bad[:4], col], tol[bad[:4]])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst[label] = max(worst.get(label, 0.0), float(np.nanmax(np.where(tol > 0, err / tol, 0.0), initial=0.0)))
    e_ref, e_tol = R.total_energy(pts, model, with_tol=True)
    assert abs(e_scan - e_ref) <= e_tol, (label, e_scan, e_ref, e_tol)
    return v_scan


@pytest.mark.parametrize("name", list(OC.FAMILIES))
def test_from_scratch_vectors_of_every_pair(name):
    t0 = time.time()
    model = OC.model_o()
    ctx = make_ctx(model)
    worst = {}
    for group in pack(OC.family(name), 64.0):
        pts = rows(group)
        v = check_vectors(ctx, pts, model, worst, name)
        assert np.array_equal(v[0::2, 1], v[1::2, 1])                       # a function of the unordered pair
    print(f"from scratch, {name}: {len(OC.family(name))} pairs, largest |device - exact| / bound = {worst[name]:.3g}, "
          f"{time.time() - t0:.1f} s")


def test_from_scratch_grid_pass_above_256_points_and_crowds():
    """more than 256 points in one configuration, so that the default threshold (256, read back) takes the grid pass; 150
    pairs that share their centre (octagons, identical rectangles, crosses), moved onto a lattice of 34 px: still each its own
    neighbourhood.  Then the crowds, a block of their own."""
    model_o, model_f = OC.model_o(), OC.model_f()
    same_centre = [(a, b) for _, a, b in OC.all_pairs() if a[0] == b[0] and a[1] == b[1]][::2][:150]
    pts = rows(same_centre)
    site = np.arange(len(same_centre))
    pts[:, 0] = np.repeat(40 + 34 * (site % 13), 2)                        # moved onto a lattice of 34 px
    pts[:, 1] = np.repeat(40 + 34 * (site // 13), 2)
    assert len(pts) == 300
    for model in (model_o, model_f):
        ctx = make_ctx(model)
        assert ctx.get_option("scratch_grid_min_points") == 256
        set_rows(ctx, pts)
        e_default, v_default = ctx.total_energy(return_vectors=True)
        worst = {}
        v = check_vectors(ctx, pts, model, worst, "dense")
        assert v.tobytes() == v_default.tobytes()
        crowd = np.concatenate(OC.crowds())
        check_vectors(ctx, crowd, model, worst, "crowds")
        print(f"from scratch, {len(model.pair)} pair terms: {len(pts)} points at once and the crowds, largest ratio {worst}")


def test_from_scratch_delta_batch_and_papangelou():
    model = OC.model_f()
    ctx = make_ctx(model)
    pairs = [(a, b) for _, a, b in OC.all_pairs()][3::40]
    worst_d = worst_p = 0.0
    for group in pack(pairs, 64.0)[:2] + [None]:
        pts = rows(group) if group is not None else np.concatenate(OC.crowds())
        set_rows(ctx, pts)
        n = len(pts)
        slots = list(range(1, n, 2))[:12]
        # remove one point; remove it and add it one pixel further; add a copy of it
        rem = [[s] for s in slots] + [[s] for s in slots] + [[] for _ in slots]
        moved = pts[slots].copy()
        moved[:, 0] += 1.0
        add = [np.zeros((0, 5))] * len(slots) + [moved[k:k + 1] for k in range(len(slots))] + \
              [pts[s:s + 1] for s in slots]
        dE = ctx.delta_batch(0, rem, [a[:, :2].astype(np.int32) for a in add], [a[:, 2:] for a in add])
        for k in range(len(rem)):
            after = np.concatenate([np.delete(pts, rem[k], axis=0), add[k]])
            ref, tol, _ = R.step_delta(pts, after, model)
            worst_d = max(worst_d, abs(dE[k] - ref) / tol)
            assert abs(dE[k] - ref) <= tol, (k, rem[k], add[k], dE[k], ref, tol)
        pap = ctx.papangelou(0)
        for s in slots:
            ref, tol, _ = R.step_delta(pts, np.delete(pts, [s], axis=0), model)
            worst_p = max(worst_p, abs(pap[s] + ref) / tol)
            assert abs(pap[s] + ref) <= tol, (s, pap[s], -ref, tol)
    print(f"delta_batch: largest |dE - exact| / tolerance = {worst_d:.3g}; papangelou: {worst_p:.3g}")


# ---- replayed tapes: clip_area_wave, clip_area_lds -------------------------------------------------------------------------
def proposal(tape, i, kernel, target, r, aux=(0.0, 0.0)):
    tape[i]["kernel"], tape[i]["target"] = kernel, target
    tape[i]["ax"], tape[i]["ay"], tape[i]["as"], tape[i]["ar"], tape[i]["aa"] = int(r[0]), int(r[1]), r[2], r[3], r[4]
    tape[i]["aux0"], tape[i]["aux1"] = aux
    tape[i]["u_accept"] = 1e-300


def pair_tape(group):
    """(initial rows, tape, configurations [len(tape) + 1]): the first rectangle of every pair is there; births of the
    second ones, Gaussian translations of every other one to the mirrored pose (for the lattice poses another
    degenerate pose) or one pixel on, then deaths of slot n until only the first ones are left (each moves the last
    point into the hole)."""
    first = np.array([a for a, _ in group], np.float64)
    second = [np.array(b, np.float64) for _, b in group]
    n = len(group)
    moves = list(range(0, n, 2))
    tape = np.zeros(2 * n + len(moves), hip_api.PROPOSAL_DTYPE)
    cur = [r for r in first]
    configs = [np.array(cur)]
    k = 0
    for b in second:
        proposal(tape, k, kernels.K_UBIRTH, -1, b)
        cur.append(b)
        configs.append(np.array(cur)); k += 1
    for i in moves:
        b = second[i].copy()
        d = first[i, :2] - b[:2]
        step = 2.0 * d if np.any(d != 0) else np.array([1.0, 0.0])
        b[:2] += step
        proposal(tape, k, kernels.K_GTRANS, n + i, b, aux=(float(step[0]), float(step[1])))
        cur[n + i] = b
        configs.append(np.array(cur)); k += 1
    for _ in range(n):
        proposal(tape, k, kernels.K_UDEATH, n, cur[n])
        cur[n] = cur[-1]
        cur.pop()
        configs.append(np.array(cur)); k += 1
    return first, tape, configs


def crowd_tape():
    """all crowds in one block; per crowd: birth of its last rectangle (>= 9 clips in the step), a translation of it by
    one pixel, its death, its birth again"""
    crowds = OC.crowds()
    init = np.concatenate([c[:-1] for c in crowds])
    tape = np.zeros(4 * len(crowds), hip_api.PROPOSAL_DTYPE)
    cur = [r for r in init]
    configs = [np.array(cur)]
    k = 0
    for c in crowds:
        last = c[-1]
        moved = last.copy()
        moved[0] += 1.0
        slot = len(cur)
        for kern, target, r in ((kernels.K_UBIRTH, -1, last), (kernels.K_GTRANS, slot, moved),
                                (kernels.K_UDEATH, slot, moved), (kernels.K_UBIRTH, -1, last)):
            proposal(tape, k, kern, target, r, aux=(1.0, 0.0) if kern == kernels.K_GTRANS else (0.0, 0.0))
            if kern == kernels.K_UDEATH:
                cur.pop()
            elif kern == kernels.K_GTRANS:
                cur[slot] = r
            else:
                cur.append(r)
            configs.append(np.array(cur)); k += 1
    return init, tape, configs


REPLAY_PAIRS = None


def replay_groups():
    global REPLAY_PAIRS
    if REPLAY_PAIRS is None:
        REPLAY_PAIRS = [pair_tape(g) for g in pack([(a, b) for _, a, b in OC.all_pairs()], 64.0)] + [crowd_tape()]
    return REPLAY_PAIRS


@pytest.mark.parametrize("model_name", ["O", "F"])
@pytest.mark.parametrize("spec,lanes,state", [(1, 0, 1), (8, 0, 1), (1, 4, 1), (1, 8, 1), (8, 0, 2)],
                         ids=["one wave", "8 waves", "4 lanes", "8 lanes", "state in device memory"])
def test_replayed_steps_of_every_pair(spec, lanes, state, model_name):
    """mpp_launch_chain takes the lane kernels (LANE = true: overlap_energy_chain -> clip_area_lds) whenever
    spec_lanes > 0 and the wave kernels (clip_area_wave) otherwise; chain_state 1 keeps the state in LDS or fails,
    chain_state 2 sends every chain to mpp_chain_hbm_kernel (wave clips).  The options are read back."""
    t0 = time.time()
    model = OC.model_o() if model_name == "O" else OC.model_f()
    ctx = make_ctx(model, cap=256, spec_waves=spec, spec_lanes=lanes, chain_state=state, deep=0)
    assert (ctx.get_option("spec_waves"), ctx.get_option("spec_lanes"), ctx.get_option("chain_state")) == (spec, lanes, state)
    ctx.set_kernels(kernels.make_kernels(mappings.default_mappings(), 1.0))
    worst, n_steps, most_clips = 0.0, 0, 0
    for init, tape, configs in replay_groups():
        set_rows(ctx, init)
        ctx.set_schedule(1e12, 1.0, 0.0)
        out = ctx.replay(0, tape)
        assert ctx.get_option("hbm_chains") == (1 if state == 2 else 0)
        assert np.all(out["accepted"] == 1)
        for k in range(len(tape)):
            ref, tol, pairs = R.step_delta(configs[k], configs[k + 1], model)
            most_clips = max(most_clips, len(pairs))
            worst = max(worst, abs(out["dE"][k] - ref) / tol)
            assert abs(out["dE"][k] - ref) <= tol, (k, tape[k], out["dE"][k], ref, tol)
            assert out["n_after"][k] == len(configs[k + 1])
        n_steps += len(tape)
        gxy, gm = ctx.get_points()
        final = configs[-1]
        assert np.array_equal(gxy, final[:, :2].astype(np.int32)) and gm.tobytes() == np.ascontiguousarray(final[:, 2:]).tobytes()
        e_ref, e_tol = R.total_energy(final, model, with_tol=True)
        assert abs(ctx.total_energy() - e_ref) <= e_tol
    assert most_clips >= 9                                   # the crowd steps: more clips than CLIP_SLOTS, last turn partly filled
    print(f"replay, spec {spec} lanes {lanes} chain_state {state}, model {model_name}: {n_steps} steps, most clips in a step "
          f"{most_clips}, largest |dE - exact| / tolerance = {worst:.3g}, {time.time() - t0:.1f} s")


# ---- deep rounds: clip_area_groups and the wave clips of deep_delta ------------------------------------------------------------
@pytest.mark.parametrize("spec,deep,fixed", [(1, 128, 0), (8, 128, 0), (8, 128, 96)])
def test_deep_rounds_on_the_parking_lot(spec, deep, fixed):
    t0 = time.time()
    det, maps, model, kd, xy, m = OC.lot_case()
    ctx = hip_api.MppContext(0, point_capacity=512, spec_waves=spec, deep=deep)
    ctx.set_option("deep_fixed", fixed)
    ctx.set_maps(det, maps)
    ctx.set_model(model, mappings.default_mappings())
    ctx.set_kernels(kd)
    ctx.set_points(0, xy, m)
    ctx.set_schedule(OC.LOT_T0, OC.LOT_ALPHA, 0.0)
    out, props = ctx.run(OC.LOT_STEPS, OC.LOT_SEED, trace_tile=0)
    st = ctx.deep_stats()
    assert st["committed"] == OC.LOT_STEPS and st["rounds"] > 0, st
    assert (ctx.get_option("deep"), ctx.get_option("deep_fixed"), ctx.get_option("spec_waves")) == (deep, fixed, spec)
    o = oracle.Oracle((OC.LOT_TILE, OC.LOT_TILE), det, maps, model, kd)          # the keeper of the state, nothing else
    o.set_points(xy, m)
    n_par = n_same = n_pop = 0
    n, worst = len(xy), 0.0
    for i, (before, after) in enumerate(OC.lot_walk(o, props, out["accepted"])):
        ref, tol, pairs = R.step_delta(before, after, model)
        par, same = OC.lot_census(pairs)
        n_par, n_same = n_par + par, n_same + same
        n_pop += bool(out["accepted"][i]) and out["n_after"][i] != n
        n = out["n_after"][i]
        worst = max(worst, abs(out["dE"][i] - ref) / tol)
        assert abs(out["dE"][i] - ref) <= tol, (i, props[i], out["dE"][i], ref, tol)
        assert out["n_after"][i] == (len(after) if out["accepted"][i] else len(before))
    gxy, gm = ctx.get_points()
    oxy, om = o.get_points()
    assert np.array_equal(gxy, oxy) and gm.tobytes() == om.tobytes()
    e_ref, e_tol = R.total_energy(np.concatenate([oxy.astype(np.float64), om], axis=1), model, with_tol=True)
    assert abs(ctx.total_energy() - e_ref) <= e_tol
    assert n_par >= 200 and n_same >= 50 and n_pop >= 20, (n_par, n_same, n_pop)
    print(f"deep rounds, spec {spec} deep {deep} fixed {fixed}: {st}, {n_par} steps clip parallel edges, {n_same} identical "
          f"rectangles, {n_pop} accepted steps change the population; largest |dE - exact| / tolerance = {worst:.3g}, "
          f"{time.time() - t0:.1f} s")


# ---- k_quad_iou: load_ccw + clip_area -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OC.FAMILIES))
def test_quad_iou_of_every_pair(name):
    """the families' corner quads; every third quad is reversed to clockwise, every fifth cyclically rotated.  IoU = I / U
    with U = A + B - I and every area within b = area_bound: |d IoU| <= (dI + IoU dU) / U <= 4 b / U."""
    ctx = hip_api.MppContext(0)
    A = np.array([R.corners(a) for a, _ in OC.family(name)])
    B = np.array([R.corners(b) for _, b in OC.family(name)])
    for k in range(len(A)):
        if k % 3 == 0:
            A[k] = A[k][::-1]
        if k % 3 == 1:
            B[k] = B[k][::-1]
        if k % 5 == 2:
            A[k] = np.roll(A[k], 1, axis=0)
        if k % 5 == 3:
            B[k] = np.roll(B[k], 2, axis=0)
    worst = 0.0
    chunk = 64                                              # the kernel fills an [n][m] matrix; the pairs are its diagonal
    for c0 in range(0, len(A), chunk):
        a, b = A[c0:c0 + chunk].reshape(-1, 8), B[c0:c0 + chunk].reshape(-1, 8)
        got = ctx.quad_iou(a, b)
        for i in range(len(a)):
            pre = voc_eval.hbb_overlaps(a[i], b)
            assert np.array_equal(got[i] == -1.0, ~(pre > 0)), (name, c0 + i)      # the axis-aligned pre-filter
            if got[i, i] == -1.0:
                assert float(R.exact_intersection(a[i].reshape(4, 2), b[i].reshape(4, 2))) == 0.0
                continue
            inter = float(R.exact_intersection(a[i].reshape(4, 2), b[i].reshape(4, 2)))
            union = float(R.exact_area(a[i].reshape(4, 2))) + float(R.exact_area(b[i].reshape(4, 2))) - inter
            if not union > 0.0:
                continue
            tol = 4.0 * R.area_bound(max(np.abs(a[i]).max(), np.abs(b[i]).max())) / union
            worst = max(worst, abs(got[i, i] - inter / union) / tol)
            assert abs(got[i, i] - inter / union) <= tol, (name, c0 + i, a[i], b[i], got[i, i], inter / union, tol)
    print(f"quad_iou, {name}: {len(A)} quads, largest |IoU - exact| / tolerance = {worst:.3g}")


def test_quad_iou_degenerate_union():
    """zero-area quads: union 0 gives (inter + 1) / (union + 1) = 1, the devkit's rule (voc_eval.iou_poly)"""
    ctx = hip_api.MppContext(0)
    point = np.array([[100.0, 100.0] * 4])
    segment = np.array([[100.0, 100.0, 104.0, 100.0, 104.0, 100.0, 100.0, 100.0]])
    square = np.array([[98.0, 98.0, 106.0, 98.0, 106.0, 106.0, 98.0, 106.0]])
    far = square + 300.0
    quads = np.concatenate([point, segment, square, far])
    got = ctx.quad_iou(quads, quads)
    for i in range(4):
        for j in range(4):
            want = -1.0 if (i == 3) != (j == 3) else voc_eval.iou_poly(quads[i], quads[j])
            assert got[i, j] == pytest.approx(want, abs=1e-12), (i, j, got[i, j], want)
    assert got[0, 0] == 1.0 and got[1, 1] == 1.0 and got[0, 1] == 1.0     # zero union
    assert got[0, 2] == 0.0 and got[1, 2] == 0.0 and got[2, 2] == 1.0     # a zero-area quad inside a square: inter 0
