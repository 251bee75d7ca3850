"""The rules of the result pictures and of ``-p detect`` that need no GPU: the line rule of the NumPy restatement against
hand-written pixel lists, its 8-bit rule against ``plt.imsave`` itself, the colour of a score, the map from the pixels the
model saw back to those of the source file, and the command line."""
import os
import sys

import numpy as np
import pytest

import figures_ref as R
from helpers import REPO
from mpp_cnn_rs_object_detection_amd import detect, figures
from mpp_cnn_rs_object_detection_amd.dataset_translation import rescale_tables
from mpp_cnn_rs_object_detection_amd.shapes import rect_to_poly

# (row, col) pixel lists written by hand from the rule: err = dx + dy, e2 = 2 err, e2 >= dy steps x, e2 <= dx steps y
LINES = {
    "horizontal": ((2, 1), (2, 5), [(2, 1), (2, 2), (2, 3), (2, 4), (2, 5)]),
    "vertical": ((1, 3), (4, 3), [(1, 3), (2, 3), (3, 3), (4, 3)]),
    "diagonal": ((0, 0), (3, 3), [(0, 0), (1, 1), (2, 2), (3, 3)]),
    "anti-diagonal": ((0, 3), (3, 0), [(0, 3), (1, 2), (2, 1), (3, 0)]),
    # dx = 2, dy = -5: err 3 ... the walk steps a row every time and a column twice
    "steep": ((0, 0), (5, 2), [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)]),
    # dx = 5, dy = -2
    "shallow": ((0, 0), (2, 5), [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5)]),
}


@pytest.mark.parametrize("name", sorted(LINES))
def test_line_rule_forward(name):
    p0, p1, want = LINES[name]
    assert R.line_pixels(p0, p1) == want


# backward walks: the rule is not symmetric under reversal when a tie (e2 == dy or e2 == dx) occurs, so these are lists of
# their own, again by hand
BACKWARD = {
    "horizontal": [(2, 5), (2, 4), (2, 3), (2, 2), (2, 1)],
    "vertical": [(4, 3), (3, 3), (2, 3), (1, 3)],
    "diagonal": [(3, 3), (2, 2), (1, 1), (0, 0)],
    "anti-diagonal": [(3, 0), (2, 1), (1, 2), (0, 3)],
    "steep": [(5, 2), (4, 2), (3, 1), (2, 1), (1, 0), (0, 0)],
    "shallow": [(2, 5), (2, 4), (1, 3), (1, 2), (0, 1), (0, 0)],
}


@pytest.mark.parametrize("name", sorted(LINES))
def test_line_rule_backward(name):
    p0, p1, _ = LINES[name]
    assert R.line_pixels(p1, p0) == BACKWARD[name]


def test_steep_line_by_hand_trace():
    """the steep line of LINES, traced state by state: (row, col, err) before each step"""
    # dx = 2, dy = -5, err = -3: e2 = -6 < dy, no x step; e2 <= dx, y step, err = -1
    # (1, 0), err -1: e2 = -2 >= -5 -> x step, err = -6; e2 <= 2 -> y step, err = -4           -> (2, 1)
    # (2, 1), err -4: e2 = -8 < -5; y step, err = -2                                            -> (3, 1)
    # (3, 1), err -2: e2 = -4 >= -5 -> x step, err = -7; y step, err = -5                       -> (4, 2)
    # (4, 2), err -5: e2 = -10 < -5; y step                                                     -> (5, 2)
    assert R.line_pixels((0, 0), (5, 2)) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)]


def test_closed_outline_of_four_edges():
    corners = np.array([[1, 1], [1, 4], [3, 4], [3, 1]], dtype=np.int32)
    px = R.outline_pixels(corners)
    want = {(1, 1), (1, 2), (1, 3), (1, 4), (2, 4), (3, 4), (3, 3), (3, 2), (3, 1), (2, 1)}
    assert set(px) == want
    assert px[0] == (1, 1) and px[-1] == (1, 1)                    # edge 3 ends where edge 0 began: the outline is closed
    img = R.draw(np.zeros((5, 6, 3), np.float32), [corners], [(0, 1, 0)])
    on = {(int(r), int(c)) for r, c in zip(*np.nonzero(img[:, :, 1]))}
    assert on == want and img[2, 2].tolist() == [0, 0, 0]          # the inside stays the picture's


def test_later_rectangles_overwrite_earlier_ones_and_outside_pixels_are_skipped():
    a = np.array([[0, 0], [0, 3], [2, 3], [2, 0]], dtype=np.int32)
    b = np.array([[2, -2], [2, 2], [5, 2], [5, -2]], dtype=np.int32)        # shares row 2 with a, leaves the picture
    img = R.draw(np.zeros((4, 4, 3), np.float32), [a, b], [(1, 0, 0), (0, 0, 1)])
    assert img[2, 0].tolist() == [0, 0, 1] and img[2, 2].tolist() == [0, 0, 1] and img[2, 3].tolist() == [1, 0, 0]
    img2 = R.draw(np.zeros((4, 4, 3), np.float32), [b, a], [(0, 0, 1), (1, 0, 0)])
    assert img2[2, 0].tolist() == [1, 0, 0] and img2[3, 2].tolist() == [0, 0, 1]


def test_corners_truncate_toward_zero():
    poly = np.array([[[-0.9, -1.2], [-0.2, 3.9], [2.7, 3.2], [2.99, -2.5]]])
    want = [[0, -1], [0, 3], [2, 3], [2, -2]]
    assert R.corners_of(poly)[0].tolist() == want
    centers, params = [(10.5, -3.25)], [(4.0, 9.0, 0.3)]
    np.testing.assert_array_equal(figures.rect_corners(centers, params),
                                  R.corners_of([rect_to_poly(centers[0], short=4.0, long=9.0, angle=0.3)]))
    assert figures.rect_corners([(0.0, 0.0)], [(1.5, 1.5, 0.0)])[0].tolist() == [[0, 0], [0, 0], [0, 0], [0, 0]]


def test_eight_bit_rule_is_that_of_imsave(tmp_path):
    from matplotlib import pyplot as plt
    k = np.arange(1, 255, dtype=np.float64)
    vals = np.concatenate([[0.0, 1.0, 0.5], k / 255, k / 255 + 1e-7, k / 255 - 1e-7]).astype(np.float32)
    n = -(-len(vals) // 3) * 3
    img = np.resize(vals, n).reshape(1, -1, 3)
    img = np.concatenate([img, img[:, ::-1]], axis=0)                       # 2 rows
    plt.imsave(tmp_path / "a.png", img)
    from PIL import Image
    back = np.array(Image.open(tmp_path / "a.png"))[:, :, :3]
    got = R.to_bytes(img)
    np.testing.assert_array_equal(got, back)
    assert got.dtype == np.uint8 and got[0, 0].tolist() == [0, 255, 127]
    # the rule truncates: it is not round-to-nearest
    assert R.to_bytes(np.full((1, 1, 3), 0.999, np.float32))[0, 0, 0] == 254


def test_colour_of_a_score():
    from matplotlib import pyplot as plt
    scores = [0.5, 2.0, 4.0, 1.0]
    cm = plt.get_cmap("plasma")
    want = np.array([cm(np.clip(s / 4.0, 0, 4.0))[:3] for s in scores], dtype=np.float32)
    np.testing.assert_array_equal(figures.score_colors(scores), want)
    np.testing.assert_array_equal(R.score_colors(scores), want)
    np.testing.assert_array_equal(figures.score_colors(scores)[2], np.asarray(cm(1.0)[:3], np.float32))   # the best: the top
    # the reference's quirk: the upper clip bound is max_score, not 1 -- with max_score = 0.2 every ratio above 0.2 (the
    # best score's 1.0 and the other's 0.5) is clipped to 0.2
    np.testing.assert_array_equal(figures.score_colors([0.2, 0.1]), np.asarray([cm(0.2)[:3]] * 2, np.float32))
    assert figures.score_colors([]).shape == (0, 3)
    np.testing.assert_array_equal(figures.cmap_table("plasma")[[0, 255]], np.asarray(cm([0, 255])[:, :3], np.float32))


def test_source_coordinate_map():
    # the identity when nothing was rescaled
    p = np.array([0.0, 3.0, 17.5])
    np.testing.assert_array_equal(detect.to_source(p, 40, 40), p)
    # per axis: a 600 x 840 source seen as 300 x 420, and one whose axes differ in factor
    np.testing.assert_allclose(detect.to_source([0, 10, 299], 600, 300), [0.5, 20.5, 598.5], rtol=0, atol=1e-12)
    np.testing.assert_allclose(detect.to_source([0, 419], 837, 420), [0.5 * 837 / 420 - 0.5, 419.5 * 837 / 420 - 0.5], rtol=0, atol=1e-12)
    # round trip with the rescale's tap centres: output pixel i samples the source at the weighted mean of its taps
    for n_in, n_out in ((600, 300), (837, 420), (101, 37)):
        idx, w = rescale_tables(n_in, n_out)
        inner = slice(8, n_out - 8)                                # (away from the mirrored border, where taps fold back)
        centre = (idx * w).sum(axis=1)
        np.testing.assert_allclose(detect.to_source(np.arange(n_out), n_in, n_out)[inner], centre[inner], rtol=0, atol=1e-9)


def test_rows_map_centre_and_corners_per_axis():
    from mpp_cnn_rs_object_detection_amd.shapes import Rectangle, sra_to_wla
    pts = [Rectangle(10, 20, size=8.0, ratio=0.5, angle=0.3), Rectangle(0, 419, size=6.0, ratio=0.4, angle=2.0)]
    res = detect.DetectResult(detections=pts, scores=np.array([1.5, 0.25]), image=np.zeros((300, 420, 3), np.float32), scale=0.5,
                              source_shape=(603, 840))
    rows = res.rows()
    assert rows.shape == (2, 14) and detect.CSV_COLUMNS[:3] == ["row", "col", "score"] and len(detect.CSV_COLUMNS) == 14
    for r, p in zip(rows, pts):
        poly = rect_to_poly((p.x, p.y), *sra_to_wla(p.size, p.ratio, p.angle))
        assert r[0] == pytest.approx((p.x + 0.5) * 603 / 300 - 0.5, abs=1e-12)
        assert r[1] == pytest.approx((p.y + 0.5) * 840 / 420 - 0.5, abs=1e-12)
        np.testing.assert_allclose(r[3:11:2], (poly[:, 0] + 0.5) * 603 / 300 - 0.5, rtol=0, atol=1e-9)
        np.testing.assert_allclose(r[4:11:2], (poly[:, 1] + 0.5) * 840 / 420 - 0.5, rtol=0, atol=1e-9)
        assert r[11:].tolist() == [p.size, p.ratio, p.angle]
    assert rows[:, 2].tolist() == [1.5, 0.25]


def test_a_coarser_picture_is_refused_and_the_flag_named():
    assert detect.resolve_scale(None) == 1.0 and detect.resolve_scale(0.5, 0.5) == 1.0 and detect.resolve_scale(0.25, 0.5) == 0.5
    with pytest.raises(ValueError, match="--gsd"):
        detect.resolve_scale(1.0, 0.5)
    with pytest.raises(ValueError, match="--gsd"):
        detect.detect_files(None, [], "unused", gsd=0.6, model_gsd=0.5)


def test_image_list_takes_directories_in_sorted_order(tmp_path):
    for name in ("b.png", "a.PNG", "notes.txt", "c.jpg"):
        (tmp_path / name).write_bytes(b"")
    (tmp_path / "single.png").write_bytes(b"")
    sub = tmp_path / "more"
    sub.mkdir()
    (sub / "z.png").write_bytes(b"")
    got = detect.list_images([str(sub), str(tmp_path / "single.png")])
    assert [os.path.basename(f) for f in got] == ["z.png", "single.png"]
    assert [os.path.basename(f) for f in detect.list_images([str(tmp_path)])] == ["a.PNG", "b.png", "c.jpg", "single.png"]
    with pytest.raises(FileNotFoundError):
        detect.list_images([str(tmp_path / "missing.png")])


def test_parser_takes_the_detect_command_line():
    sys.path.insert(0, REPO)
    import main
    a = main.build_parser().parse_args("-p detect -m mpp -c mpp_hrcM --images a b --out d".split())
    assert a.procedure == "detect" and a.images == ["a", "b"] and a.out == "d"
    assert a.gsd is None and a.model_gsd == 0.5 and a.min_score is None and a.figures is False
    b = main.build_parser().parse_args("-p detect -m mpp -c x --images a --out d --gsd 0.25 --model-gsd 0.5 --min-score 0.3 "
                                       "--figures --restarts 2 --unet-max-pixels 1000".split())
    assert (b.gsd, b.model_gsd, b.min_score, b.figures, b.restarts, b.unet_max_pixels) == (0.25, 0.5, 0.3, True, 2, 1000)
    assert main.build_parser().parse_args("-p infer -m mpp -c x".split()).figures is False


def test_save_png_round_trip(tmp_path):
    from PIL import Image
    a = np.random.default_rng(0).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    figures.save_png(str(tmp_path / "x.png"), a)
    np.testing.assert_array_equal(np.array(Image.open(tmp_path / "x.png"))[:, :, :3], a)
    with pytest.raises(ValueError):
        figures.save_png(str(tmp_path / "y.png"), a.astype(np.float32))
