"""The classic image energies on the GPU (csrc/mpp_classics.hpp) where the rasteriser's grid outgrows one 64-bit word or
64 lanes, and where it hangs over the borders of a picture that is not square: the rectangles of tests/classics_cases.py
under every mask recipe ``mpp_set_model`` admits, against the CPU oracle on the same float32 picture (the oracle goes pixel
by pixel, has no grid, and is pinned to the reference at these rectangles by tests/test_classics_edges_host.py).

(a) the one-thread form (``classic_contrast``, ``classic_gradient``) through ``classic_values``;
(b) the wave form (``classic_contrast_wave``) in the chain kernel and in the HBM-state kernel, one chosen rectangle at a
    time: a replayed tape of births on an empty configuration, bit for bit against (a);
(c) the wave form in the deep-round kernel: a chain steered to large thin rectangles, lockstep with the oracle;
(d) the admission check of ``mpp_set_model``: the largest rectangle of a 36-px size mapping fits the 96 x 128 window.

Tolerance: device vs oracle 1e-12 relative of max(1, |v|), the bar of tests/test_gpu_classics.py (the same float64
expressions; another order of summation and libm vs device sqrt / log in the last place)."""
import numpy as np
import pytest

import classics_cases as CC
import oracle
from helpers import lockstep_vs_oracle
from mpp_cnn_rs_object_detection_amd import energies as E
from mpp_cnn_rs_object_detection_amd import hip_api, kernels
from mpp_cnn_rs_object_detection_amd.custom_types import ImageWMaps
from mpp_cnn_rs_object_detection_amd.shapes import Rectangle

pytestmark = pytest.mark.gpu

TOL = 1e-12
N32 = len(CC.CASES)
EMPTY_XY, EMPTY_MARKS = np.zeros((0, 2), np.int32), np.zeros((0, 3), np.float64)


class _Desc:
    unit, pair, combinator, gate_term, gate_thr, lin0 = [(E.U_CONST, 0, 1.0, [0.0])], [], 0, -1, 0.0, 0.0


def rel(a, b):
    with np.errstate(invalid="ignore"):
        return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def rects(cases):
    return [Rectangle(x, y, size=s, ratio=r, angle=a) for x, y, s, r, a in cases]


def contrast_term(t, recipe, rgb):
    dil, gap, ero = recipe
    image = CC.picture() if rgb else CC.grey_picture()[..., None]
    return E.contrast_term("c", image, dilation=dil, gap=gap, erode=ero, contrast_measure_type=t, rgb=rgb, thresh=0.25)


def gradient_term(rgb):
    return E.gradient_term("g", CC.picture() if rgb else CC.grey_picture()[..., None], dilation=1, rgb=rgb, thresh=0.1)


_oracle, _cache = [], {}


def the_oracle():
    if not _oracle:
        _oracle.append(oracle.Oracle((CC.H, CC.W), np.zeros((CC.H, CC.W), np.float32), None, _Desc()))
    return _oracle[0]


def values(key):
    """(device one-thread values, oracle values, fill mask is empty) over CASES + CASES36, computed once per term.
    key = ("c", measure, recipe, rgb) or ("g", rgb).  CASES go through the default mappings, CASES36 through a 0..36 px size
    mapping, as a model holding them would."""
    if key not in _cache:
        term = contrast_term(*key[1:]) if key[0] == "c" else gradient_term(key[1])
        got = np.concatenate([E.classic_values(term, rects(CC.CASES), mappings=CC.mappings32()),
                              E.classic_values(term, rects(CC.CASES36), mappings=CC.mappings36())])
        o = the_oracle()
        o.set_image(term.image)
        want = np.array([o.unit_value((term.kind, 0, 1.0, term.params), r) for r in CC.ALL_CASES])
        empty = np.zeros(len(want), bool)
        if key[0] == "c":
            empty = np.array([len(o.contrast_masks(r, *key[2])[0]) == 0 for r in CC.ALL_CASES])
        _cache[key] = (got, want, empty)
    return _cache[key]


def check_against_oracle(got, want, empty, default, what):
    """-> worst rel.  Finite where the oracle is finite and within TOL of it, non-finite where it is not, exactly the
    default value where the fill is empty or eroded away."""
    fin = np.isfinite(want)
    assert not np.any(np.isnan(got[fin])), (what, np.nonzero(np.isnan(got) & fin)[0])      # (the grid-too-large exit answers NaN)
    assert np.all(np.isfinite(got[fin])) and not np.any(np.isfinite(got[~fin])), what
    worst = float(np.max(rel(got[fin], want[fin])))
    assert worst < TOL, (what, worst, int(np.argmax(np.where(fin, rel(got, want), 0))))
    if default is not None:
        assert np.all(got[empty] == default) and np.all(want[empty] == default), what
    return worst


# ---- (a) the one-thread form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgb", [True, False])
@pytest.mark.parametrize("t", CC.MEASURES)
def test_contrast_values_one_thread(t, rgb):
    worst = 0.0
    for recipe in CC.RECIPES:
        got, want, empty = values(("c", t, recipe, rgb))
        assert np.isfinite(want).sum() > 0.9 * len(want) and (empty.any() or recipe[2] == 0)
        worst = max(worst, check_against_oracle(got, want, empty, E.CONTRAST_MEASURES[t][2], (t, recipe, rgb)))
    print(t, "rgb" if rgb else "grey", "one-thread form, worst rel err vs oracle", worst)


@pytest.mark.parametrize("rgb", [True, False])
def test_gradient_values(rgb):
    got, want, empty = values(("g", rgb))
    assert np.all(np.isfinite(want))
    worst = check_against_oracle(got, want, empty, None, ("gradient", rgb))
    print("gradient", "rgb" if rgb else "grey", "worst rel err vs oracle", worst)


# ---- (b) the wave form, one chosen rectangle at a time ----------------------------------------------------------------
def birth_tape(cases, with_death):
    tape = np.zeros(len(cases) * (2 if with_death else 1), hip_api.PROPOSAL_DTYPE)
    births = tape[::2] if with_death else tape
    births["kernel"], births["target"] = 0, -1
    for p, (x, y, s, r, a) in zip(births, cases):
        p["ax"], p["ay"], p["as"], p["ar"], p["aa"] = x, y, s, r, a
    if with_death:
        tape[1::2]["kernel"], tape[1::2]["target"] = 1, 0
    tape["u_accept"] = 1e-300
    return tape


WAVE_RECIPES = [(2, 1, 1), (4, 2, 2), (4, 2, 0), (2, 0, 0)]


@pytest.mark.parametrize("spec,chain_state", [(1, 0), (8, 0), (8, 2)])
def test_wave_form_equals_the_one_thread_form_bit_for_bit(spec, chain_state):
    """The model's only term is the contrast term (plain sum: coefficient 1, not gated, lin0 = 0; a model needs nothing
    else to be replayed), the configuration is empty, and the tape alternates the birth of case i (uniform birth kernel)
    with its death at a temperature of 1e12 and an accept uniform of 1e-300: every birth lands on an empty configuration
    and its dE is the combined energy of the new point alone,

        dE = lin0 + coef * 1.0 * v = 0.0 + 1.0 * 1.0 * v      (unit_part_mv, csrc/mpp_device.hpp)

    with v the wave's value of the term.  Multiplying by 1.0 and adding to 0.0 change no bit of a finite or infinite v (v
    is never -0.0 here: a difference with a non-zero threshold, or a default value): so dE must be the one-thread value of
    (a) bit for bit -- what ``cl_sums`` promises -- and within 1e-12 of the oracle.  Rectangles whose value is not finite
    (a one-pixel fill under the craciun measure) are born alone on a configuration emptied by ``set_points``, since
    their death may be refused; their dE must be the same non-finite value."""
    worst, n_births, n_large = 0.0, 0, 0
    for rgb in (True, False):
        image = (CC.picture() if rgb else CC.grey_picture()[..., None])
        ctx = hip_api.MppContext(0, point_capacity=256, spec_waves=spec, chain_state=chain_state)
        ctx.set_maps(np.full((CC.H, CC.W), 0.5, np.float32), [np.full((CC.H, CC.W, 32), 1.0 / 32, np.float32)] * 3)
        ctx.set_image(image)
        kd = kernels.make_kernels(CC.mappings36(), 1.0)
        for recipe in WAVE_RECIPES:
            large = sum(max(g["nr"], g["nc"]) > 64 for g in (CC.grid(r, recipe) for r in CC.ALL_CASES))
            for t in CC.MEASURES:
                one, want, empty = values(("c", t, recipe, rgb))
                term = contrast_term(t, recipe, rgb)
                ctx.set_model(E.build_model_desc([term], [], None), CC.mappings36())
                ctx.set_kernels(kd)
                ctx.set_schedule(1e12, 1.0, 0.0)
                fin = np.isfinite(want)
                idx = np.nonzero(fin)[0]
                ctx.set_points(0, EMPTY_XY, EMPTY_MARKS)
                out = ctx.replay(0, birth_tape([CC.ALL_CASES[i] for i in idx], True))
                assert np.all(out["accepted"] == 1) and np.all(out["n_after"][::2] == 1) and np.all(out["n_after"][1::2] == 0)
                dE = np.zeros(len(want))
                dE[idx] = out["dE"][::2]
                for i in np.nonzero(~fin)[0]:
                    ctx.set_points(0, EMPTY_XY, EMPTY_MARKS)
                    dE[i] = ctx.replay(0, birth_tape([CC.ALL_CASES[i]], False))["dE"][0]
                what = (t, recipe, rgb, spec, chain_state)
                same = (dE.view(np.uint64) == (0.0 + 1.0 * 1.0 * one).view(np.uint64)) | (np.isnan(dE) & np.isnan(one))
                assert np.all(same), (what, np.nonzero(~same)[0], dE[~same], one[~same])
                worst = max(worst, check_against_oracle(dE, want, empty, E.CONTRAST_MEASURES[t][2], what))
                n_births += len(want); n_large += large
        assert ctx.get_option("hbm_chains") == (1 if chain_state == 2 else 0)
        ctx.close()
    print(f"wave form, spec_waves {spec} chain_state {chain_state}: {n_births} births ({n_large} on a grid of more than 64 rows "
          f"or columns) equal the one-thread form bit for bit; worst rel err vs oracle {worst}")


# ---- (c) the wave form in the deep-round kernel -----------------------------------------------------------------------
TILE = (128, 160)
DEEP_RECIPE = (2, 1, 1)          # the contrast setup's masks for the craciun2 measure


def peaked(classes, weights, rng):
    p = np.full(32, 0.002)
    p[list(classes)] += weights
    m = np.tile((p / p.sum()).astype(np.float32), TILE + (1,)) * rng.uniform(0.8, 1.2, size=TILE + (32,)).astype(np.float32)
    return (m / m.sum(-1, keepdims=True)).astype(np.float32)


def steered_setup():
    """the contrast setup on a 128 x 160 tile of the noise picture with mark maps that propose large thin rectangles: size
    classes 29..31, ratio classes 3..5 (0.09 to 0.16), angles around 0 and pi / 2; a threshold that rewards every
    rectangle, so that the chain holds a few dozen of them and moves them about"""
    setup = E.ContrastMeasureEnergySetup(contrast_type="craciun2", manual_threshold=0.02)
    setup.energy_cal = {"detection_thresh": 0.02, "min_area": 20.0, "max_area": 400.0}
    rng = np.random.default_rng(3)
    det = np.clip(0.3 + rng.normal(0, 0.1, TILE), 0.01, 1).astype(np.float32)
    marks = [peaked((31, 30, 29), (0.5, 0.3, 0.1), rng), peaked((3, 4, 5), (0.5, 0.3, 0.1), rng), peaked((0, 16, 8), (0.4, 0.4, 0.1), rng)]
    data = ImageWMaps(name="0", shape=TILE, image=np.ascontiguousarray(CC.picture()[:TILE[0], :TILE[1]]), detection_map=det,
                      param_dist_maps=marks, mappings=CC.mappings32(), param_names=["size", "ratio", "angle"], labels=None,
                      gt_config=[])
    return setup, data


def steered_ctx(data, unit, model, kd, spec, T0, alpha):
    ctx = hip_api.MppContext(0, point_capacity=256, spec_waves=spec)
    ctx.set_maps(data.detection_map, data.param_dist_maps)
    ctx.set_image(E.classic_image(unit))
    ctx.set_model(model, data.mappings)
    ctx.set_points(0, EMPTY_XY, EMPTY_MARKS)
    ctx.set_kernels(kd)
    ctx.set_schedule(T0, alpha, 0.0)
    return ctx


@pytest.mark.parametrize("spec", [8, 1])
def test_deep_rounds_with_large_thin_rectangles_against_the_oracle(spec):
    """3 000 steps in deep rounds (the default ``deep``; a call of fewer than 4 096 steps starts in them), lockstep with
    the oracle: proposals, dE to 1e-9, decisions, final configuration; then the untraced production launch, array for
    array.  Counted from the traced proposals with ``classics_cases.grid``: at least 50 evaluated additions (births, and
    moves of an existing point) whose grid has more than 64 rows, and 50 with more than 64 columns -- the maps, the
    seed and the length were chosen with ``oracle.run(..., trace=True)`` alone (134 and 104)."""
    n_steps, seed, T0, alpha = 3000, 7, 0.05, 0.999
    setup, data = steered_setup()
    np.random.seed(5)
    unit, pair = setup.make_energies(data)
    comb = E.ManualHierarchicalEnergyCombinator(dict(zip(setup.NAMES, [1.0, 2.0, 0.5, 0.25, 0.75])), "ContrastEnergy", 0.0)
    model = E.build_model_desc(unit, pair, comb)
    kd = kernels.make_kernels(data.mappings, 12.0)
    o = oracle.Oracle(data.shape, data.detection_map, data.param_dist_maps, model, kd)
    o.set_image(E.classic_image(unit))
    o.set_points(EMPTY_XY, EMPTY_MARKS)
    o.set_temperature(T0, alpha, 0.0)
    ctx = steered_ctx(data, unit, model, kd, spec, T0, alpha)
    traced, run = [], ctx.run

    def spy(*a, **k):
        res = run(*a, **k)
        traced.append(res[1])
        assert ctx.deep_stats()["committed"] == len(res[1]) and ctx.deep_stats()["rounds"] > 0      # all of it in deep rounds
        return res
    ctx.run = spy
    ties = lockstep_vs_oracle(ctx, o, n_steps, seed=seed, chain=0, alpha=alpha, chunk=1000)
    props = np.concatenate(traced)
    assert len(props) == n_steps
    rows = cols = 0
    for p in props[~np.isin(props["kernel"], (1, 3)) & ((props["kernel"] < 4) | (props["target"] >= 0))]:
        g = CC.grid((p["ax"], p["ay"], p["as"], p["ar"], p["aa"]), DEEP_RECIPE, TILE)
        rows, cols = rows + (g is not None and g["nr"] > 64), cols + (g is not None and g["nc"] > 64)
    print(f"deep rounds, spec_waves {spec}: {rows} evaluated additions with more than 64 grid rows, {cols} with more than 64 "
          f"columns, {ties} ties, {len(o)} points at the end")
    assert rows >= 50 and cols >= 50
    gxy, gm = ctx.get_points(0)
    oxy, om = o.get_points()
    assert len(gxy) >= 10
    np.testing.assert_array_equal(gxy, oxy)
    np.testing.assert_allclose(gm, om, rtol=1e-9, atol=1e-9)
    assert ties <= 3
    ctx2 = steered_ctx(data, unit, model, kd, spec, T0, alpha)
    ctx2.run(n_steps, seed=seed, chain0=0)
    st = ctx2.deep_stats()
    assert st["rounds"] > 0 and st["committed"] == n_steps, st
    pxy, pm = ctx2.get_points(0)
    np.testing.assert_array_equal(pxy, gxy)
    np.testing.assert_array_equal(pm, gm)
    ctx.close(); ctx2.close()


# ---- (d) the admission check ------------------------------------------------------------------------------------------
def test_the_largest_admitted_rectangle_fits_the_window():
    """"the largest rectangle (size = vmax, ratio -> 0) must fit with its margins" (mpp_set_model): with a 0..36 px size
    mapping and the recipe of the widest margin, (4, 2, 0), every value of CASES36 -- up to 71.9 px long, a grid of up to
    87 rows or columns -- is finite and the oracle's; a mapping that goes a hair beyond 36 px is refused."""
    worst = 0.0
    for rgb in (True, False):
        for t in CC.MEASURES:
            got, want, empty = values(("c", t, (4, 2, 0), rgb))
            got, want = got[N32:], want[N32:]
            assert np.all(np.isfinite(want)) and np.all(np.isfinite(got)), (t, rgb)
            assert np.all(rel(got, want) < TOL), (t, rgb, np.max(rel(got, want)))
            worst = max(worst, float(np.max(rel(got, want))))
    grids = [CC.grid(r, (4, 2, 0)) for r in CC.CASES36]
    assert max(g["nr"] for g in grids) > 80 and max(g["nc"] for g in grids) > 80
    print("36-px size mapping, recipe (4, 2, 0): worst rel err vs oracle", worst)
    term = contrast_term("craciun2", (4, 2, 0), True)
    ctx = hip_api.MppContext(0, point_capacity=256)
    ctx.set_maps(np.zeros((CC.H, CC.W), np.float32), [np.zeros((CC.H, CC.W, 32), np.float32)] * 3)
    ctx.set_image(term.image)
    ctx.set_model(E.build_model_desc([term], [], None), CC.mappings36())
    for model_term in (term, gradient_term(True)):
        with pytest.raises(hip_api.MppError, match="the classic image energies need size marks <= 36 px"):
            ctx.set_model(E.build_model_desc([model_term], [], None), CC.mappings36(float(np.nextafter(36.0, 37.0))))
    ctx.close()
