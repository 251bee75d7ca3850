"""The device-side merge (``mpp_merge_score``: ``k_papangelou_tiles``, ``k_has_neighbour``, ``k_dedupe_tiles`` and the second
``k_papangelou_tiles``) against the plain walk of tests/merge_ref.py and the float64 oracle, at the configurations of
tests/merge_cases.py.  Every case asserts (``check_merge``):

(a) first scoring, bit for bit: the reference walk over ``exp(-dE)`` of ``ctx.papangelou(tile)``, read before the merge,
    gives exactly the device's removed count, survivors, survivor ORDER and marks;
(b) first scoring against float64: that ``dE`` equals the oracle's ``papangelou()`` to ``rtol=1e-9, atol=1e-8`` (the
    tolerance tests/test_gpu_kat.py uses for this quantity), and the walk over the ORACLE's scores removes the same points
    (tests/test_merge_ref_host.py proves that no decision of these inputs is closer than 1e-6 relative, constructed
    duplicates apart, which agree to 1e-12);
(c) second scoring: the returned ``dE`` of the survivors equals bit for bit ``papangelou()`` of a fresh context loaded with
    the survivors, and the oracle's values to the same tolerance;
(d) state: afterwards ``ctx.count(t)`` / ``ctx.get_points(t)`` are the returned configuration and
    ``removed[t] == n_before - n_after``.

``MppContext.merge_score`` allocates its own output arrays, so the tests cannot hand sentinels to the device; what they
can see is that every returned row was written (it equals an independent computation).
Measured figures (reached branches, error / tolerance) are in profiles/merge_tests.md."""
import numpy as np
import pytest

import merge_cases as MC
import merge_ref as R
import oracle
from helpers import hrc_model, log_model
from mpp_cnn_rs_object_detection_amd import hip_api, mappings
from mpp_cnn_rs_object_detection_amd.custom_types import ImageWMaps
from mpp_cnn_rs_object_detection_amd.shapes import Rectangle

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-8
WORST = {}                  # case -> largest |device - oracle| / tolerance seen (printed; pytest -s shows it)


def context(case, tiles=None, which=None, capacity=None):
    """a context with the case's maps and model and the given tiles' points (``which``: a subset of the case's tiles)"""
    which = list(range(len(case.tiles))) if which is None else which
    tiles = [case.tiles[t] for t in which] if tiles is None else tiles
    ctx = hip_api.MppContext(0, point_capacity=case.capacity if capacity is None else capacity)
    ctx.set_maps(np.stack([case.maps[t][0] for t in which]), [np.stack([case.maps[t][1][k] for t in which]) for k in range(3)])
    if case.image is not None:
        ctx.set_image(np.stack([case.image] * len(which)))
    ctx.set_model(case.model or MC.model_desc(case.setup_name), mappings.default_mappings())
    for k, (xy, mk) in enumerate(tiles):
        ctx.set_points(k, xy, mk)
    return ctx


def close_to_oracle(label, got, want):
    """(b) / (c): finite entries to the tolerance, the pattern of the non-finite ones exactly"""
    got, want = np.asarray(got), np.asarray(want)
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=label)
    np.testing.assert_array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)], err_msg=label)
    if fin.any():
        ratio = float(np.max(np.abs(got[fin] - want[fin]) / (ATOL + RTOL * np.abs(want[fin]))))
        WORST[label] = max(WORST.get(label, 0.0), ratio)
        print(f"{label}: max |device - oracle| / tolerance = {ratio:.3g}")
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=ATOL, err_msg=label)


def check_merge(case, distance, which=None, against_oracle=True, oracle_walk=True, oracle_after=True):
    """(a) - (d) for every tile of the case at one distance -> [(first dE, (xy, marks, dE) of the survivors)] per tile"""
    which = list(range(len(case.tiles))) if which is None else which
    ctx = context(case, which=which)
    first = [ctx.papangelou(k).copy() for k in range(len(which))]
    res, removed = ctx.merge_score(distance)
    assert len(res) == len(which) and len(removed) == len(which)
    for k, t in enumerate(which):
        xy, mk = case.tiles[t]
        label = f"{case.name}/{case.setup_name}/tile{t}/d={distance:.3f}"
        gxy, gmk, gdE = res[k]
        assert len(first[k]) == len(xy)
        # (a)
        rm = R.walk(xy, MC.scores_of(first[k]), distance)
        sxy, smk, _ = R.compact(xy, mk, rm)
        assert int(removed[k]) == int(rm.sum()), label
        np.testing.assert_array_equal(gxy, sxy, err_msg=label)
        np.testing.assert_array_equal(gmk, smk, err_msg=label)
        # (b)
        if against_oracle:
            want = MC.oracle_dE(case, t)
            close_to_oracle(label + " first", first[k], want)
            if oracle_walk:
                np.testing.assert_array_equal(R.walk(xy, MC.scores_of(want), distance), rm, err_msg=label)
        # (d)
        assert ctx.count(k) == len(gxy) and int(removed[k]) == len(xy) - len(gxy), label
        pxy, pmk = ctx.get_points(k)
        np.testing.assert_array_equal(pxy, gxy, err_msg=label)
        np.testing.assert_array_equal(pmk, gmk, err_msg=label)
    ctx.close()
    # (c)
    fresh = context(case, tiles=[(r[0], r[1]) for r in res], which=which)
    for k, t in enumerate(which):
        gxy, gmk, gdE = res[k]
        assert len(gdE) == len(gxy)
        np.testing.assert_array_equal(fresh.papangelou(k), gdE, err_msg=f"{case.name} tile {t} second scoring")
        if against_oracle and oracle_after and len(gxy):
            close_to_oracle(f"{case.name}/{case.setup_name}/tile{t}/d={distance:.3f} second", gdE, MC._dE(case, t, gxy, gmk))
    fresh.close()
    return [(first[k], res[k]) for k in range(len(which))], removed


# ---- 1. the mixed batch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setup_name", ["legacy", "no-calibration"])
def test_mixed_batch(setup_name):
    """Tiles of 0, 37 and 700 points on different maps in a context of capacity 777; the 700-point tile carries the planted
    structures of ``merge_cases.mixed`` (duplicates, pairs at exactly 3 and just outside, A-B-C chains in all six score
    orders, clumps, the last index as a winner, the corners), the 37-point one ends with a loser.  ``merge_score`` switches
    the candidate grids on by ``max_n >= 64`` for the WHOLE batch (the option ``scratch_grid_min_points`` plays no part on
    this path: the case runs with it at 0 too), so the 37-point tile is scored with a grid here and without one when it
    runs alone in a context of its own: the results must be the same bit for bit.
    Under the log model ("no-calibration") the scores of points off the objects agree to five digits (a saturated
    sigmoid), so its decisions do hang on small differences: for it the walk over the ORACLE's scores is not asserted;
    (a), the dE half of (b), (c) and (d) are."""
    case = MC.mixed(setup_name)
    assert [len(t[0]) for t in case.tiles] == [0, 37, 700] and case.capacity == 777
    got, removed = check_merge(case, 3.0, oracle_walk=setup_name == "legacy")
    assert removed[0] == 0 and removed[1] >= 1 and removed[2] >= 59
    alone, removed_alone = check_merge(case, 3.0, which=[1], oracle_walk=setup_name == "legacy")
    np.testing.assert_array_equal(alone[0][0], got[1][0])              # (papangelou() before the merge: the same launch both times)
    for a, b in zip(alone[0][1], got[1][1]):
        np.testing.assert_array_equal(a, b)
    assert removed_alone[0] == removed[1]
    ctx = context(case)
    ctx.set_option("scratch_grid_min_points", 0)
    res, rem = ctx.merge_score(3.0)
    ctx.close()
    np.testing.assert_array_equal(rem, removed)
    for k in range(3):
        for a, b in zip(res[k], got[k][1]):
            np.testing.assert_array_equal(a, b)


# ---- 2. a crowd beyond the list ----------------------------------------------------------------------------------------
def test_crowd_beyond_the_list():
    """More than 300 points within the model's reach of a common point: ``k_papangelou_tiles`` lists 303 > 256 neighbours
    for each of them and falls back to its plain loop, while the 25 far points of the same tile keep the list.  Both must
    give ``papangelou()``'s values bit for bit -- (a) and (c) compare them through the walk and directly -- and the
    oracle's.  Merged with distance 3 and with distance 0 (only the exact duplicates go; the oracle's pass over the 324
    survivors would take 15 s on the CPU, so (c) is checked against the fresh context there and not against the oracle)."""
    case = MC.crowd()
    xy = case.tiles[0][0].astype(np.int64)
    reach = MC.max_inter(case.setup_name)
    assert reach == max(p[4] for p in MC.model_desc(case.setup_name).pair)
    centre = np.array(MC.CROWD_CENTRE)
    assert int((np.sqrt(((xy - centre) ** 2).sum(-1)) <= reach).sum()) >= 300
    within = (np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1).astype(float)) <= reach).sum(axis=1)
    assert int((within > 256).sum()) >= 300 and int((within <= 256).sum()) >= 20          # both paths are taken
    print(f"crowd: {int((within > 256).sum())} points take the plain loop, {int((within <= 256).sum())} the list")
    _, removed3 = check_merge(case, 3.0)
    _, removed0 = check_merge(case, 0.0, oracle_after=False)
    assert removed0[0] == 4 and removed3[0] > 100


# ---- 3. non-finite scores ------------------------------------------------------------------------------------------------
def test_non_finite_scores_from_a_linear_model():
    """+inf and 0 scores from the legacy model with its unit weights times 1e4 (``exp(-dE)`` overflows on the objects and
    underflows off them): neighbourhoods of two infinities (the first wins), of zeros only (the first wins: a finite tie)
    and of an infinity with a zero.  dE itself stays finite and is compared as usual; the walks over the device's and over
    the oracle's scores must remove the same points."""
    case = MC.nonfinite_linear()
    got, _ = check_merge(case, 3.0)
    s = MC.scores_of(got[0][0])
    assert np.isinf(s).sum() >= 10 and (s == 0).sum() >= 10
    print(f"nonfinite_linear: {int(np.isinf(s).sum())} +inf, {int((s == 0).sum())} zero scores of {len(s)}")
    kinds = {(int(np.isinf(s[near]).sum()), int((s[near] == 0).sum())) for _, near, _ in R._decisions(case.tiles[0][0], s, 3.0)[1]}
    assert {(2, 0), (0, 3), (1, 1)} <= kinds


def test_nan_scores_from_the_craciun_contrast_measure():
    """NaN through a real model (``merge_cases.nonfinite_contrast``): the oracle gives NaN at the same indices as the device
    (asserted by ``close_to_oracle``), the one-pixel rectangle scores +inf, and the neighbourhoods hold a NaN after a
    larger finite score (the NaN is kept), an infinity with a NaN (the NaN is kept), two NaN (the first), two finite."""
    case = MC.nonfinite_contrast()
    got, removed = check_merge(case, 3.0)
    dE = got[0][0]
    s = MC.scores_of(dE)
    np.testing.assert_array_equal(np.isnan(dE), np.isnan(MC.oracle_dE(case, 0)))
    print(f"nonfinite_contrast: {int(np.isnan(s).sum())} NaN, {int(np.isinf(s).sum())} +inf scores of {len(s)}")
    assert np.isinf(s[2]) and np.isnan(s[[1, 3, 4, 5, 9, 12]]).all() and np.isfinite(s[[0, 6, 7, 8, 10, 11]]).all()
    assert removed[0] == 4
    finite_loser = 6 if s[6] < s[7] else 7
    np.testing.assert_array_equal(R.walk(case.tiles[0][0], s, 3.0), np.isin(np.arange(13), [0, 2, 5, finite_loser]))


def test_beyond_the_models_reach_a_score_stays_finite():
    """DESIGN.md 2, deviation 9, pinned (``merge_cases.beyond_reach``): Q lies 40 px from the one-pixel rectangle P, beyond
    the model's reach of 32 but inside P's 3 x 3 cells.  The oracle (the reference's two neighbourhood sums) gives Q NaN;
    the scratch kernels sum over the points within reach and give Q the dE it has without P, before and after the merge."""
    case = MC.beyond_reach()
    xy, mk = case.tiles[0]
    want = MC.oracle_dE(case, 0)
    assert want[0] == -np.inf and np.isnan(want[1]) and np.isfinite(want[2])
    without_p = MC._dE(case, 0, xy[1:], mk[1:])
    ctx = context(case)
    first = ctx.papangelou(0).copy()
    res, removed = ctx.merge_score(3.0)
    ctx.close()
    assert first[0] == -np.inf and removed[0] == 0
    np.testing.assert_allclose(first[1:], without_p, rtol=RTOL, atol=ATOL)
    np.testing.assert_array_equal(res[0][0], xy)
    np.testing.assert_array_equal(res[0][2], first)


def test_the_tie_rule_on_scores_that_differ():
    """``merge_cases.near_tie``: the later of two neighbours scores HIGHER by one float32 ulp of the detection map, 2.3e-10
    relative.  That is a tie (1e-9): the first is kept.  Asserted on the device's own scores (0 < gap < 1e-9, the later one
    larger), then through (a) - (d)."""
    case = MC.near_tie()
    got, removed = check_merge(case, 3.0)
    s = MC.scores_of(got[0][0])
    assert s[1] > s[0] and 0 < (s[1] - s[0]) / s[1] < 1e-9 and s[3] > s[4] and 0 < (s[3] - s[4]) / s[3] < 1e-9
    assert removed[0] == 4
    survivors = {tuple(p) for p in got[0][1][0].tolist()}
    assert survivors == {(10, 10), (20, 30), (28, 5)}


# ---- 4. distances ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distance", MC.DISTANCES, ids=lambda d: f"{d:.4f}")
def test_distances(distance):
    """``dist2 = floor(d * d + 1e-9)`` against the float comparison ``sqrt(dx^2 + dy^2) <= d`` of the reference walk, on a
    configuration that holds a pair for every integer offset up to length 5."""
    case = MC.distances()
    _, removed = check_merge(case, distance)
    xy = case.tiles[0][0].astype(np.int64)
    pairs_within = sum(1 for a, b in case.roles["pairs"] if np.sqrt(float(((xy[a] - xy[b]) ** 2).sum())) <= distance)
    assert int(removed[0]) >= pairs_within and (distance > 0 or removed[0] == 0)


# ---- 5. the largest tile the walk accepts ------------------------------------------------------------------------------------
def test_largest_accepted_tile():
    """n = 8192 in a context of capacity 9600 on a 512 x 512 support: (a), (c), (d) (the oracle's O(n^2) pass is left out);
    one point more is declined with code -4, which the callers turn into the host merge."""
    case = MC.largest()
    assert len(case.tiles[0][0]) == 8192 and case.capacity == 9600
    _, removed = check_merge(case, 3.0, against_oracle=False)
    assert removed[0] > 1000
    xy, mk = case.tiles[0]
    free = np.setdiff1d(np.arange(512 * 512), xy[:, 0].astype(np.int64) * 512 + xy[:, 1])[:1]
    ctx = context(case, tiles=[(np.concatenate([xy, [[free[0] // 512, free[0] % 512]]]).astype(np.int32), np.concatenate([mk, mk[:1]]))])
    assert ctx.count(0) == 8193
    with pytest.raises(hip_api.MppError) as ei:
        ctx.merge_score(3.0)
    assert ei.value.code == -4 and "8193" in str(ei.value) and "host" in str(ei.value)
    assert ctx.count(0) == 8193                                           # (declined before anything was touched)
    ctx.close()


# ---- 6. through the user-facing call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["hrc", "log"])
def test_merge_score_images_equals_merge_patches(tag):
    """``data_loaders.merge_score_images`` on two images of one shape with 37 and 700 detections (the mixed batch's tiles)
    against ``merge_patches`` + ``papangelou_all`` image by image: survivors, order and scores are equal."""
    from mpp_cnn_rs_object_detection_amd.data_loaders import merge_patches, merge_score_images
    setup, comb = hrc_model() if tag == "hrc" else log_model()
    case = MC.mixed("legacy")
    images = [ImageWMaps(name=str(t), shape=case.shape, image=None, detection_map=case.maps[t][0], param_dist_maps=case.maps[t][1],
                         mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS, labels=None, gt_config=[],
                         crop_data={"tl_anchor": np.array([0, 0])}) for t in (1, 2)]
    agg = [case.tiles[t] for t in (1, 2)]
    res = merge_score_images(images, agg, comb, setup, 3)
    for image, (xy, mk), (det, scores) in zip(images, agg, res):
        rects = [Rectangle(int(x), int(y), size=float(s), ratio=float(r), angle=float(a)) for (x, y), (s, r, a) in zip(xy, mk)]
        merged = merge_patches(patches=[image], results=[rects], original_image=image, energy_model=comb, method="distance",
                               energy_setup=setup, distance=3)
        host_rows = np.array([p.as_row() for p in merged])
        assert 0 < len(host_rows) < len(xy)
        np.testing.assert_array_equal(np.array([p.as_row() for p in det]), host_rows)
        np.testing.assert_array_equal(scores, merged.papangelou_all(energy_combinator=comb))


# ---- 7. wide supports ------------------------------------------------------------------------------------------------------
def test_wide_support():
    """Points 46350 columns apart: 46350^2 does not fit an int32, and a squared distance that wraps to a negative number
    would make them neighbours.  Only the exact duplicate may be removed."""
    case = MC.wide()
    got, removed = check_merge(case, 3.0)
    assert removed[0] == 1
    np.testing.assert_array_equal(got[0][1][0], case.tiles[0][0][[0, 1, 2, 4]])


def test_the_widest_support_a_context_takes():
    """Positions travel through the walk packed as two 16-bit halves.  ``set_maps`` is the guard: it takes no side above
    65535, so no coordinate exceeds 65534.  At that width the extreme coordinates come back unchanged and the points at the
    two ends, whose squared distance exceeds 2^32, are no neighbours."""
    from mpp_cnn_rs_object_detection_amd import synth
    W = 65535
    xy = np.array([[0, 0], [0, W - 1], [0, 40000], [0, W - 1], [0, 32768]], dtype=np.int32)
    mk = MC.rand_marks(np.random.default_rng(5), 5)
    mk[3] = mk[1]
    det, marks = synth.render_maps((1, W), xy[[0, 2]], mk[[0, 2]], noise=0.2, noise_seed=4)
    case = MC.Case("widest", "legacy", (1, W), [(det, marks)], [(xy, mk)], 64)
    got, removed = check_merge(case, 3.0)
    assert removed[0] == 1
    np.testing.assert_array_equal(got[0][1][0], xy[[0, 1, 2, 4]])
    ctx = hip_api.MppContext(0, point_capacity=64)
    with pytest.raises(hip_api.MppError) as ei:
        ctx.set_maps(np.zeros((1, W + 1), np.float32), [np.zeros((1, W + 1, 32), np.float32)] * 3)
    assert ei.value.code == -1 and "geometry" in str(ei.value)
    ctx.close()
