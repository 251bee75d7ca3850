"""The exact overlap reference (tests/overlap_ref.py) against closed forms, and every CPU implementation of the clipper
against it: the C oracle (the yardstick of all chain tests), the shapely stand-in that recorded the tapes, and the
triangle fan of oracle.voc_eval.  Runs without a GPU."""
import functools
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest

import oracle
import overlap_cases as OC
import overlap_ref as R
from oracle import voc_eval
from test_geometry import CASES

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILY_NAMES = list(OC.FAMILIES)


@functools.lru_cache(maxsize=None)
def facts(name):
    """per pair of a family: corners, exact intersection, number of vertices of the exact intersection, parallel edges"""
    out = []
    for r1, r2 in OC.family(name):
        A, B = R.corners(r1), R.corners(r2)
        H = R.exact_polygon(A, B)
        inter = float(abs(R._shoelace2(H)) / 2) if len(H) >= 3 else 0.0
        out.append(dict(r1=r1, r2=r2, A=A, B=B, inter=inter, nv=len(H), par=R.parallel_edges(A, B),
                        M=float(max(np.abs(A).max(), np.abs(B).max()))))
    return out


@functools.lru_cache(maxsize=None)
def shim_geometry():
    spec = importlib.util.spec_from_file_location("_overlap_shim_geometry",
                                                  os.path.join(HERE, "golden", "_shim", "shapely", "geometry.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the reference against closed forms -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r1,r2,inter", CASES, ids=[c[0] for c in CASES])
def test_reference_on_the_analytic_cases(name, r1, r2, inter):
    A, B = R.corners(r1), R.corners(r2)
    M = max(np.abs(A).max(), np.abs(B).max())
    # the corner doubles are within 2^-53 * M of the ideal corners: the exact area of THESE quads is within the sincos /
    # rounding part of the bound of the closed form
    assert float(R.exact_intersection(A, B)) == pytest.approx(inter, abs=R.area_bound(M))
    assert R.exact_intersection(A, B) == R.exact_intersection(B, A)
    e = R.overlap(r1, r2)
    mn = min(float(R.exact_area(A)), float(R.exact_area(B)))
    assert e == pytest.approx(0.0 if mn < 1e-12 else inter / (mn + 1e-6), abs=R.area_bound(M) / (mn + 1e-6))


def test_reference_regular_octagon():
    # two axis-parallel squares of side 2 about the origin, one turned by 45 degrees, with RATIONAL corners: the square
    # with corners (+-7/5, 0), (0, +-7/5) has side 7 sqrt(2) / 5 -- not the regular octagon, but an octagon whose area
    # is rational: the square |x|+|y| <= 7/5 minus the four corner triangles beyond |x| = 1 or |y| = 1 (legs 2/5)
    sq = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], float)
    dm = np.array([[1.4, 0], [0, 1.4], [-1.4, 0], [0, -1.4]], float)
    d = Fraction(1.4)                                   # the double nearest 7/5, taken exactly
    expect = 2 * d * d - 4 * (d - 1) * (d - 1)
    assert R.exact_intersection(sq, dm) == expect
    assert len(R.exact_polygon(sq, dm)) == 8
    assert R.exact_intersection(dm[::-1], sq) == expect                 # clockwise input, swapped
    # the regular octagon of test_geometry through corners(): 2 * 16 * (sqrt(2) - 1)
    A, B = R.corners([50, 50, 4.0, 1.0, 0.0]), R.corners([50, 50, 4.0, 1.0, np.pi / 4])
    assert len(R.exact_polygon(A, B)) == 8
    assert float(R.exact_intersection(A, B)) == pytest.approx(32.0 * (np.sqrt(2.0) - 1.0), abs=R.area_bound(52.9))


RATIONAL = [
    # (A, B, exact area written out by hand)
    ([(0, 0), (4, 0), (4, 3), (0, 3)], [(1.5, 1), (6, 1), (6, 5.25), (1.5, 5.25)], Fraction(5)),            # 2.5 x 2
    ([(0, 0), (4, 0), (4, 3), (0, 3)], [(4, 0), (7, 0), (7, 3), (4, 3)], Fraction(0)),                      # shared edge
    ([(0, 0), (4, 0), (4, 3), (0, 3)], [(4, 3), (7, 3), (7, 5), (4, 5)], Fraction(0)),                      # shared corner
    ([(0, 0), (4, 0), (4, 3), (0, 3)], [(0, 0), (4, 0), (4, 3), (0, 3)], Fraction(12)),                     # identical
    ([(0, 0), (4, 0), (4, 3), (0, 3)], [(0.5, 0), (2.75, 0), (2.75, 3), (0.5, 3)], Fraction(27, 4)),        # two shared lines
    ([(0, 0), (8, 0), (8, 2), (0, 2)], [(3, -3), (5, -3), (5, 5), (3, 5)], Fraction(4)),                    # cross
    ([(0, 0), (4, 0), (4, 4), (0, 4)], [(2, -1), (5, 2), (2, 5), (-1, 2)], Fraction(14)),                   # 16 - 4 * 1/2
    ([(0.125, 0.25), (3.125, 0.25), (3.125, 1.75), (0.125, 1.75)], [(1, 1), (2, 1), (2, 9), (1, 9)], Fraction(3, 4)),
    ([(0, 0), (3, 0), (3, 3), (0, 3)], [(1, 1), (2, 1), (2, 1), (1, 1)], Fraction(0)),                      # zero-area quad
]


@pytest.mark.parametrize("k", range(len(RATIONAL)))
def test_reference_on_rational_corners(k):
    A, B, expect = RATIONAL[k]
    A, B = np.array(A, float), np.array(B, float)
    for P, Q in ((A, B), (B, A), (A[::-1], B), (np.roll(A, 1, axis=0), B[::-1])):
        assert R.exact_intersection(P + 100.0, Q + 100.0) == expect
        assert R.exact_intersection(P, Q) == expect


def test_reference_through_corners_at_axis_angles():
    # angle pi/2: the long side runs along the rows, corners are whole numbers: 8 x 4 shifted by 2 rows -> 6 x 4
    assert R.exact_intersection(R.corners([50, 50, 6.0, 0.5, np.pi / 2]), R.corners([52, 50, 6.0, 0.5, np.pi / 2])) == 24
    # angle 0: the long side runs along the columns; 8 x 4 against 4 x 2 whose corner sits on the first's corner
    assert R.exact_intersection(R.corners([50, 50, 6.0, 0.5, 0.0]), R.corners([51, 52, 3.0, 0.5, 0.0])) == 8
    assert R.exact_intersection(R.corners([50, 50, 6.0, 0.5, 0.0]), R.corners([53, 56, 3.0, 0.5, 0.0])) == 0
    assert R.align([0, 0, 1, 1, 0.25], [0, 0, 1, 1, 0.25 + np.pi / 2], 0.0) == pytest.approx(1.0, abs=1e-15)
    assert R.align([0, 0, 1, 1, 0.25], [0, 0, 1, 1, 0.25], 1.0) == -1.0


# ---- every CPU clipper against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_oracle_overlap_within_bound(name):
    worst = 0.0
    for f in facts(name):
        e, tol = R.overlap(f["r1"], f["r2"]), R.overlap_tol(f["r1"], f["r2"])
        for got in (oracle.overlap(f["r1"], f["r2"]), oracle.overlap(f["r2"], f["r1"])):
            worst = max(worst, abs(got - e) / tol)
            assert abs(got - e) <= tol, (name, f["r1"], f["r2"], got, e, tol)
    print(f"oracle.overlap, {name}: {len(facts(name))} pairs, largest |oracle - exact| / bound = {worst:.3g}")


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_shim_within_bound(name):
    """``Polygon.intersection(...).area`` of tests/golden/_shim/shapely: the code that recorded the tapes"""
    g = shim_geometry()
    worst = 0.0
    for f in facts(name):
        A, B, b = f["A"], f["B"], R.area_bound(f["M"])
        got = g.Polygon(A).intersection(g.Polygon(B)).area
        if min(float(R.exact_area(A)), float(R.exact_area(B))) < 1e-12:
            assert got == 0.0
            continue
        worst = max(worst, abs(got - f["inter"]) / b)
        assert abs(got - f["inter"]) <= b, (name, f["r1"], f["r2"], got, f["inter"])
    print(f"shim, {name}: largest |shim - exact| / bound = {worst:.3g}")


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_triangle_fan_within_bound(name):
    """``oracle.voc_eval.iou_poly`` (polyiou.cpp's triangle fan) against exact inter / (A + B - inter).

    IoU = I / U with U = A + B - I and every area within b = area_bound: |d IoU| <= (dI + IoU dU) / U <= 4 b / U.

    The devkit's absolute sign tolerance of 1e-8 failed this on "near touch" (14 of 490 pairs, up to 62 x the tolerance:
    touching poses displaced by 1e-9 px were snapped onto the line); oracle/voc_eval.py now decides on the sign of the
    double itself and passes every family at <= 0.03 of the tolerance."""
    worst = 0.0
    misses = []
    for f in facts(name):
        A, B, b = f["A"], f["B"], R.area_bound(f["M"])
        union = float(R.exact_area(A)) + float(R.exact_area(B)) - f["inter"]
        if not union > 0.0:
            continue
        got = voc_eval.iou_poly(A.reshape(-1), B.reshape(-1))
        tol = 4.0 * b / union
        worst = max(worst, abs(got - f["inter"] / union) / tol)
        if abs(got - f["inter"] / union) > tol:
            misses.append((f["r1"].tolist(), f["r2"].tolist(), got, f["inter"] / union, tol))
    print(f"triangle fan, {name}: largest |IoU - exact| / tolerance = {worst:.3g}, {len(misses)} misses")
    assert not misses, (name, len(misses), misses[:3])


# ---- discrimination: a restatement of the float64 clipper passes, three wrong ones do not ----------------------------------
def clipper(S, C, cap=8, clockwise=False, wrong_t=False):
    """clip_area() of csrc/mpp_device.hpp in Python floats (IEEE double, no FMA)"""
    if clockwise:
        C = C[::-1]
    ax, ay = [float(p[0]) for p in S], [float(p[1]) for p in S]
    for e in range(4):
        if not ax:
            break
        x0, y0, x1, y1 = float(C[e][0]), float(C[e][1]), float(C[(e + 1) & 3][0]), float(C[(e + 1) & 3][1])
        ex, ey = x1 - x0, y1 - y0
        bx, by = [], []
        px, py = ax[-1], ay[-1]
        sp = ex * (py - y0) - ey * (px - x0)
        for qx, qy in zip(ax, ay):
            sq = ex * (qy - y0) - ey * (qx - x0)
            if sq >= 0:
                if sp < 0 and len(bx) < cap:
                    t = sq / (sq - sp) if wrong_t else sp / (sp - sq)
                    bx.append(px + t * (qx - px)); by.append(py + t * (qy - py))
                if len(bx) < cap:
                    bx.append(qx); by.append(qy)
            elif sp >= 0 and len(bx) < cap:
                t = sq / (sq - sp) if wrong_t else sp / (sp - sq)
                bx.append(px + t * (qx - px)); by.append(py + t * (qy - py))
            px, py, sp = qx, qy, sq
        ax, ay = bx, by
    if len(ax) < 3:
        return 0.0
    s = 0.0
    for i in range(len(ax)):
        j = (i + 1) % len(ax)
        s += ax[i] * ay[j] - ax[j] * ay[i]
    return 0.5 * abs(s)


def clipper_failures(name, **mutation):
    bad = 0
    for f in facts(name):
        if min(float(R.exact_area(f["A"])), float(R.exact_area(f["B"]))) < 1e-12:
            continue
        bad += abs(clipper(f["A"], f["B"], **mutation) - f["inter"]) > R.area_bound(f["M"])
    return bad


def test_restated_clipper_passes_and_mutants_fail():
    assert {n: clipper_failures(n) for n in FAMILY_NAMES} == {n: 0 for n in FAMILY_NAMES}
    table = {}
    for label, mutation in (("vertex cap 7", dict(cap=7)), ("clipper wound clockwise", dict(clockwise=True)),
                            ("t = sq / (sq - sp)", dict(wrong_t=True))):
        table[label] = {n: clipper_failures(n, **mutation) for n in FAMILY_NAMES}
        print(f"mutant '{label}': failing pairs per family {table[label]}")
        assert sum(table[label].values()) > 0, label
    assert table["vertex cap 7"]["eight vertices"] > 0


# ---- the families keep what they were built for -----------------------------------------------------------------------
def test_family_conditions():
    allf = [f for n in FAMILY_NAMES for f in facts(n)]
    nonzero = sum(f["inter"] > 0.0 for f in allf)
    parallel = sum(f["par"] for f in allf)
    eight = sum(f["nv"] == 8 for f in allf)
    print(f"{len(allf)} pairs: {nonzero} with a non-zero exact area, {parallel} with exactly parallel edges, "
          f"{eight} with 8-vertex intersections; per family "
          f"{ {n: len(facts(n)) for n in FAMILY_NAMES} }")
    assert nonzero >= 0.4 * len(allf)
    assert parallel >= 200
    assert eight >= 30
    assert len(facts("generic")) == 300
    assert sum(f["nv"] == 8 for f in facts("eight vertices")) >= 30
    for n in FAMILY_NAMES:
        if n != "slivers and tiny":
            assert all(min(float(R.exact_area(f["A"])), float(R.exact_area(f["B"]))) >= 1.0 for f in facts(n)), n
        assert all(40 <= f["r1"][0] <= 480 and 40 <= f["r1"][1] <= 480 for f in facts(n)), n
    for crowd in OC.crowds():
        assert len(crowd) >= 10                       # the last one meets >= 9 others: more clips than CLIP_SLOTS = 4
        assert sum(R.overlap(crowd[-1], q) > 0 for q in crowd[:-1]) >= 9


def test_parking_lot_reaches_the_degenerate_clips():
    """the deep-round case of tests/test_gpu_overlap_exact.py, with the oracle's own run at the same seed: enough steps
    clip exactly parallel edges and identical rectangles, enough accepted steps change the population"""
    det, maps, model, kd, xy, m = OC.lot_case()
    o = oracle.Oracle((OC.LOT_TILE, OC.LOT_TILE), det, maps, model, kd)
    o.set_points(xy, m)
    o.set_temperature(OC.LOT_T0, OC.LOT_ALPHA, 0.0)
    out, props = o.run(OC.LOT_STEPS, OC.LOT_SEED, chain=0, trace=True)
    o.set_points(xy, m)
    n_par = n_same = n_pop = 0
    n = len(xy)
    worst = 0.0
    for i, (before, after) in enumerate(OC.lot_walk(o, props, out["accepted"])):
        dE, tol, pairs = R.step_delta(before, after, model)
        par, same = OC.lot_census(pairs)
        n_par, n_same = n_par + par, n_same + same
        n_pop += bool(out["accepted"][i]) and out["n_after"][i] != n
        n = out["n_after"][i]
        worst = max(worst, abs(out["dE"][i] - dE) / tol)
        assert abs(out["dE"][i] - dE) <= tol, (i, props[i], out["dE"][i], dE, tol)
    print(f"parking lot, oracle's run: {n_par} steps clip parallel edges, {n_same} identical rectangles, {n_pop} accepted "
          f"steps change the population, {int(out['accepted'].sum())} accepted; largest |dE - exact| / tolerance = "
          f"{worst:.3g}; {R.exact_pairs_done()} exact pairs so far")
    assert n_par >= 200 and n_same >= 50 and n_pop >= 20
