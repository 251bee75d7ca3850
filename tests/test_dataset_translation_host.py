"""Dataset translation, host half (no GPU): annotations against the reference's own pickles for five images of its sample
dataset, ``polygon_to_abw``, the tap tables of the rescale against the scipy restatement of skimage 0.18.1
(``rescale_ref.py``), selection and meta parsing on a fabricated tree."""
import os
import warnings

import numpy as np
import pytest

from mpp_cnn_rs_object_detection_amd import dataset_translation as dt
from mpp_cnn_rs_object_detection_amd.shapes import polygon_to_abw, rect_to_poly
from rescale_ref import output_shape, rescale_ref
from translation_cases import KERNEL_CASES, Golden, assert_annotations_equal, build_dota_tree, make_image, meta_text


@pytest.fixture(scope="module")
def gold():
    return Golden()


# ---- annotations -----------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_five_images(gold):
    assert gold.ids == [2800, 2804, 2781, 2789, 2794]
    assert sum(len(gold.get("centers", i)) for i in gold.ids) == 1104


@pytest.mark.parametrize("i", [2800, 2804, 2781, 2789, 2794])
def test_annotations_equal_the_reference_pickles(gold, i):
    """|parameters - reference| <= 1e-12: a few ulps of values up to about 100 (measured: 7.2e-15)"""
    gsd = gold.get("original_gsd", i)
    scale = gsd / gold.target_gsd
    assert scale == gold.get("scale", i)
    lab = dt.dota_annotations(gold.get("text", i), gold.categories, scale)
    assert_annotations_equal(lab, gold, i, tol=1e-12)
    assert sum(dt.count_objects(gold.get("text", i), gold.categories).values()) == gold.get("n_objects", i) == len(lab["centers"])


def test_annotations_without_objects_are_empty_arrays(gold):
    lab = dt.dota_annotations(gold.get("text", 2800), ["helipad"], 0.5)
    assert set(lab) == {"centers", "parameters", "categories", "difficult"}
    assert all(isinstance(v, np.ndarray) and v.shape == (0,) for v in lab.values())


def test_scale_within_a_hundredth_of_one_leaves_polygons_unscaled():
    text = "10.0 20.0 30.0 20.0 30.0 28.0 10.0 28.0 small-vehicle 1\n5 5 9 5 9 7 5 7 plane 0\n"
    a = dt.dota_annotations(text, ["small-vehicle"], 0.995)
    b = dt.dota_annotations(text, ["small-vehicle"], 1.0)
    assert np.array_equal(a["centers"], [[24, 20]]) and np.array_equal(a["parameters"], b["parameters"])
    # corners are (y, x): the long edges run along x, the axis joins their midpoints, (28, 20) -> (20, 20): atan2(0, -8) % pi
    assert np.allclose(a["parameters"], [[8.0, 20.0, 0.0]], atol=1e-15) and list(a["difficult"]) == [1]
    c = dt.dota_annotations(text, ["small-vehicle"], 0.5)
    assert np.array_equal(c["centers"], [[12, 10]]) and np.allclose(c["parameters"], [[4.0, 10.0, 0.0]], atol=1e-15)


def test_polygon_to_abw_both_branches():
    # first edge short (n1 < n2) and first edge long: a rectangle and the same one with its corners shifted by one
    for angle in (0.0, 0.3, 1.2, np.pi / 2, 2.0, 3.0):
        poly = rect_to_poly((50.0, 60.0), short=6.0, long=15.0, angle=angle)
        for shift in range(4):
            a, b, w = polygon_to_abw(np.roll(poly, shift, axis=0))
            assert abs(a - 6.0) < 1e-12 and abs(b - 15.0) < 1e-12 and 0 <= w < np.pi
    one = np.array([[0.0, 0.0], [0.0, 4.0], [10.0, 4.0], [10.0, 0.0]])          # |p0 p1| = 4 < |p1 p2| = 10: first branch
    assert np.allclose(polygon_to_abw(one), [4.0, 10.0, np.pi / 2])             # axis (5, 0) -> (5, 4): atan2(4, 0)
    two = np.roll(one, 1, axis=0)                                               # |p0 p1| = 10: second branch
    assert np.allclose(polygon_to_abw(two), [4.0, 10.0, np.pi / 2])             # axis (0, -4): atan2(-4, 0) % pi
    both = polygon_to_abw(np.stack([one, two, one * 2.0]))
    assert both.shape == (3, 3) and np.allclose(both[2], [8.0, 20.0, np.pi / 2])
    tilted = np.array([[0.0, 0.0], [3.0, -3.0], [13.0, 7.0], [10.0, 10.0]])
    a, b, w = polygon_to_abw(tilted)
    assert np.allclose([a, b, w], [np.hypot(3, 3), np.hypot(10, 10), 3 * np.pi / 4])     # axis (5, 5) -> (8, 2): atan2(-3, 3) % pi


# ---- the tap tables of the rescale -----------------------------------------------------------------------------------------
def dense(idx, w, n_in):
    m = np.zeros((len(idx), n_in))
    np.add.at(m, (np.repeat(np.arange(len(idx)), idx.shape[1]), idx.ravel()), w.ravel())
    return m


@pytest.mark.parametrize("H,W,scale", KERNEL_CASES)
def test_tables_reproduce_the_scipy_restatement(H, W, scale):
    """R @ img @ C^T against gaussian_filter(mode='mirror') + bilinear: at most (2 * 18 + 2)^2 ~ 1.4 k terms of size <= 1 at
    eps 1.1e-16 bound the difference of the two orders by 1.6e-13 (measured: 6.7e-16); tolerance 1e-12."""
    img = make_image(H, W)
    (oh, ow), (ri, rw, ci, cw) = dt.rescale_image_tables(H, W, scale)
    assert (oh, ow) == output_shape(H, W, scale)
    assert ri.dtype == np.int32 and ci.dtype == np.int32 and rw.dtype == np.float64 and ri.shape == rw.shape == (oh, ri.shape[1])
    sigma = max(0.0, (H / oh - 1) / 2)
    assert ri.shape[1] == 2 * int(4 * sigma + 0.5) + 2
    R, C = dense(ri, rw, H), dense(ci, cw, W)
    x = img / 255
    out = np.stack([R @ x[:, :, c] @ C.T for c in range(3)], axis=-1)
    err = float(np.abs(out - rescale_ref(img, scale)).max())
    print(f"{H} x {W} @ {scale}: -> {oh} x {ow}, T = {ri.shape[1]} / {ci.shape[1]}, max |tables - restatement| = {err:.3g}")
    assert err <= 1e-12
    for idx, w, n in ((ri, rw, H), (ci, cw, W)):
        assert np.abs(w.sum(axis=1) - 1).max() <= 1e-15
        assert idx.min() >= 0 and idx.max() < n


def test_output_shapes():
    assert dt.rescale_output_shape(2213, 3553, 0.21193735055) == (469, 753)        # the reference's metadata shape of 2781
    assert dt.rescale_output_shape(5, 25, 0.5) == (2, 12)                          # 2.5 and 12.5: half to even
    assert dt.rescale_output_shape(7, 3, 0.5) == (4, 2)                            # 3.5 -> 4, 1.5 -> 2


def test_tables_fold_at_the_mirror_boundary():
    idx, w = dt.rescale_tables(10, 2)                  # f = 5: sigma 2, radius 8, 18 taps around 2 and 7 fold at both ends
    assert idx.shape == (2, 18) and idx.min() == 0 and idx.max() == 9
    assert list(idx[0][:7]) == [6, 5, 4, 3, 2, 1, 0]   # positions -6 .. 0 without repeating the edge
    with pytest.raises(ValueError):
        dt.rescale_tables(10, 11)


# ---- selection and meta parsing --------------------------------------------------------------------------------------------
def test_meta_parsing():
    assert dt.parse_meta_text(meta_text("2015-07-15", "GoogleEarth", 0.118071506532)) == ("2015-07-15 00:00:00", "GoogleEarth",
                                                                                       0.118071506532)
    assert dt.parse_meta_text("acquisition date:\nimagesource:None\ngsd:null\n") == ("NaT", None, None)
    assert dt.parse_meta_text(meta_text("soon", "GF", "None")) == ("NaT", "GF", None)
    with pytest.raises(ValueError):
        dt.parse_meta_text("gsd:0.1\n")


def test_selection_on_a_fabricated_tree(tmp_path, gold):
    build_dota_tree(tmp_path, gold, with_images=False)
    rows = dt.fetch_dota_paths(str(tmp_path), "val")
    assert [r["id"] for r in rows] == [2781, 2789, 2794, 9001, 9002]
    with open(tmp_path / "val" / "meta" / "P9003.txt", "w") as f:          # no image, no labels: not paired
        f.write(meta_text("", "GoogleEarth", 0.1))
    for i, gsd in ((9004, "unknown"), (9005, 0.25)):                         # an unparsable gsd; an image without objects
        for d, text in (("images", ""), ("DOTA-v2.0_val", "1 1 5 1 5 3 1 3 plane 0\n"), ("meta", meta_text("", "JL", gsd))):
            with open(tmp_path / "val" / d / f"P{i}.{'png' if d == 'images' else 'txt'}", "w") as f:
                f.write(text)
    rows = dt.fetch_dota_paths(str(tmp_path), "val")
    assert [r["id"] for r in rows] == [2781, 2789, 2794, 9001, 9002, 9004, 9005]
    for r in rows:
        with open(r["path_label"]) as f:
            r["counts"] = dt.count_objects(f.read(), gold.categories)

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        kept = dt.select_dota(rows, gold.categories, 0.5, prune_empty=True, banned_sources=["Aerial"])
    assert [r["id"] for r in kept] == [2781, 2789, 2794]
    assert [r["n_objects"] for r in kept] == [gold.get("n_objects", i) for i in (2781, 2789, 2794)]
    assert [r["scale"] for r in kept] == [gold.get("scale", i) for i in (2781, 2789, 2794)]
    assert abs(sum(r["sample_density"] for r in kept) - 1) < 1e-12
    with pytest.warns(UserWarning, match="WorldView"):
        kept = dt.select_dota(rows, gold.categories, 0.5, prune_empty=False, banned_sources=["WorldView"])
    assert [r["id"] for r in kept] == [2781, 2789, 2794, 9002, 9005]       # 9001: gsd 0.8, 9004: no gsd; the empty one stays
    kept = dt.select_dota(rows, gold.categories, 1.0, prune_empty=True, banned_sources=None)
    assert [r["id"] for r in kept] == [2781, 2789, 2794, 9001, 9002] and kept[3]["scale"] == 0.8


def test_drop_rate_reproduces_the_reference_draw():
    rows = [{"id": 100 - i, "source": "GoogleEarth", "gsd": 0.25, "counts": {"small-vehicle": 1}} for i in range(37)]
    kept = dt.select_dota(rows, ["small-vehicle"], 0.5, prune_empty=True, drop_rate=0.3, banned_sources=[])
    by_id = sorted(r["id"] for r in rows)
    want = np.sort(np.random.default_rng(0).choice(range(37), size=int(37 * (1 - 0.3)), replace=False))
    assert [r["id"] for r in kept] == [by_id[k] for k in want] and len(kept) == 25
    assert len(dt.select_dota(rows, ["small-vehicle"], 0.5, prune_empty=True, drop_rate=0.0)) == 37


def test_cowc_annotations():
    ann = np.zeros((20, 30, 4), dtype=np.uint8)
    ann[3, 7] = (255, 0, 0, 255)
    ann[19, 29] = (255, 0, 0, 255)
    lab = dt.cowc_annotations(ann, 0.15 / 0.5)
    assert np.array_equal(lab["centers"], [[0, 2], [5, 8]])                # int(3 * 0.3), int(7 * 0.3); int(5.7), int(8.7)
    assert np.array_equal(lab["parameters"], [[4.0, 4.0, 0.0]] * 2) and list(lab["categories"]) == ["vehicle", "vehicle"]
    assert np.array_equal(lab["difficult"], [0, 0])
    assert all(len(v) == 0 for v in dt.cowc_annotations(np.zeros((4, 4, 4), np.uint8), 0.3).values())
