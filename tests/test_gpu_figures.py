"""The outline scatter and compose kernels (``csrc/mpp_figures.hip``) against the NumPy restatement of ``figures_ref.py``,
byte for byte: all octants, corners beyond every border, a rectangle wholly outside, one collapsed into a pixel, overlapping
outlines in both index orders, many rectangles over several blocks, and the scalar base."""
import numpy as np
import pytest

import figures_ref as R
from mpp_cnn_rs_object_detection_amd import figures
from mpp_cnn_rs_object_detection_amd.shapes import Rectangle, rect_to_poly, sra_to_wla

pytestmark = pytest.mark.gpu

H, W = 37, 53


@pytest.fixture(scope="module")
def ctx():
    from mpp_cnn_rs_object_detection_amd.hip_api import MppContext
    c = MppContext(0)
    yield c
    c.close()


def base_picture(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.random((h, w, 3)).astype(np.float32)
    img[0, 0], img[0, 1], img[1, 0] = 0.0, 1.0, 0.5
    img[2, :w // 2] = (rng.integers(0, 256, (w // 2, 3)) / 255).astype(np.float32)          # k / 255: the edges of the 8-bit rule
    return img


def forty_rectangles():
    """(centers, params = (a, b, angle)) of the 37 x 53 case; the last four are two overlapping pairs"""
    centers, params = [], []
    for k in range(16):                                            # 16 angles: every octant, both directions of each edge
        centers.append((6.0 + 8 * (k // 4) + 0.37 * k, 7.0 + 11 * (k % 4) + 0.61 * k))
        params.append((5.0 + 0.3 * k, 11.0 + 0.2 * k, k * 2 * np.pi / 16 + 0.05))
    for c in ((-2.0, 20.0), (38.5, 30.0), (15.0, -3.0), (20.0, 54.0),      # corners beyond the top, bottom, left, right border
              (0.0, 0.0), (36.0, 52.0), (-4.0, -4.0), (40.0, 56.0)):       # ... and beyond two at once, at each corner
        centers.append(c)
        params.append((7.0, 13.0, 0.4 + 0.3 * len(centers)))
    centers.append((-30.0, 80.0)); params.append((6.0, 12.0, 0.7))         # wholly outside
    centers.append((100.0, 10.0)); params.append((6.0, 12.0, 2.1))         # wholly outside, its bounding box too
    centers.append((12.3, 17.8)); params.append((0.0, 0.0, 1.0))           # size 0: all four corners in one pixel
    centers.append((-0.4, -0.7)); params.append((0.5, 0.5, 0.0))           # ... truncated toward zero from the negative side
    rng = np.random.default_rng(3)
    while len(centers) < 36:
        centers.append((float(rng.uniform(0, H)), float(rng.uniform(0, W))))
        params.append((float(rng.uniform(2, 9)), float(rng.uniform(4, 20)), float(rng.uniform(0, np.pi))))
    centers += [(18.0, 25.0), (20.0, 28.0), (9.0, 40.0), (9.0, 43.0)]      # two pairs whose outlines cross
    params += [(9.0, 15.0, 0.3), (9.0, 15.0, 1.2), (6.0, 10.0, 0.0), (6.0, 10.0, 0.0)]
    assert len(centers) == 40
    return centers, params


def colors_for(n, seed=1):
    rng = np.random.default_rng(seed)
    c = rng.random((n, 3)).astype(np.float32)
    if n:
        c[0] = (0.0, 1.0, 0.0)
    return c


def on_device(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(f"cuda:{ctx.device}")


def run(ctx, base, corners, colors):
    import torch
    t = on_device(ctx, base)
    torch.cuda.synchronize()
    return ctx.draw_outlines(t, corners, colors).cpu().numpy()


@pytest.mark.parametrize("n", [0, 1, 40])
def test_small_picture_equals_the_restatement(ctx, n):
    centers, params = forty_rectangles()
    corners = figures.rect_corners(centers[:n], params[:n])
    np.testing.assert_array_equal(corners, R.corners_of([rect_to_poly(c, short=p[0], long=p[1], angle=p[2])
                                                         for c, p in zip(centers[:n], params[:n])]))
    base, colors = base_picture(H, W, 0), colors_for(n)
    got = run(ctx, base, corners, colors)
    want = R.picture(base, corners, colors)
    assert got.shape == (H, W, 3) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, want)
    if n == 0:
        np.testing.assert_array_equal(got, R.to_bytes(base))       # no rectangle: the base picture
    if n == 40:
        assert np.any(corners < 0) and np.any(corners[:, :, 0] >= H) and np.any(corners[:, :, 1] >= W)
        assert len({tuple(q) for q in corners[26]}) == 1 and corners[27].tolist() == [[0, 0]] * 4      # the collapsed ones


def test_overlapping_outlines_follow_the_index(ctx):
    centers, params = forty_rectangles()
    base, colors = base_picture(H, W, 0), colors_for(40)
    corners = figures.rect_corners(centers, params)
    swap = np.arange(40)
    swap[[36, 37, 38, 39]] = [37, 36, 39, 38]                      # the same rectangles and colours, the pairs in the other order
    a = run(ctx, base, corners, colors)
    b = run(ctx, base, corners[swap], colors[swap])
    np.testing.assert_array_equal(a, R.picture(base, corners, colors))
    np.testing.assert_array_equal(b, R.picture(base, corners[swap], colors[swap]))
    # the pictures differ exactly where the outlines of a pair cross, and there the higher index wins
    diff = np.any(a != b, axis=2)
    assert diff.any()
    for i, j in ((36, 37), (38, 39)):
        shared = set(R.outline_pixels(corners[i])) & set(R.outline_pixels(corners[j]))
        shared = {(r, c) for r, c in shared if 0 <= r < H and 0 <= c < W}
        later = [set(R.outline_pixels(corners[k])) for k in range(j + 1, 40)]
        shared = {p for p in shared if not any(p in s for s in later)}
        assert shared
        for (r, c) in shared:
            assert a[r, c].tolist() == R.to_bytes(colors[j][None, None])[0, 0].tolist()
            assert b[r, c].tolist() == R.to_bytes(colors[i][None, None])[0, 0].tolist()


def test_five_hundred_rectangles_over_several_blocks(ctx):
    h, w, n = 300, 420, 500
    rng = np.random.default_rng(7)
    centers = np.stack([rng.uniform(-10, h + 10, n), rng.uniform(-10, w + 10, n)], axis=1)
    params = np.stack([rng.uniform(3, 14, n), rng.uniform(6, 40, n), rng.uniform(0, 2 * np.pi, n)], axis=1)
    corners = figures.rect_corners(centers, params)
    base, colors = base_picture(h, w, 1), colors_for(n, 2)
    np.testing.assert_array_equal(run(ctx, base, corners, colors), R.picture(base, corners, colors))


def test_scalar_base_through_a_table(ctx):
    vmin, vmax = 0.25, 0.75
    rng = np.random.default_rng(5)
    m = rng.uniform(-0.2, 1.2, (H, W)).astype(np.float32)            # below vmin, above vmax; W = 53 is no multiple of 64
    m[0, :6] = [vmin, vmax, np.nextafter(np.float32(vmin), np.float32(0)), np.nextafter(np.float32(vmax), np.float32(1)), -5.0, 9.0]
    edges = (vmin + (vmax - vmin) * np.arange(W) / 256.0 * 5).astype(np.float32)      # values near the table's bin edges
    m[3] = edges
    lut = figures.cmap_table("plasma")
    assert np.any(m < vmin) and np.any(m > vmax) and np.any(m == np.float32(vmin)) and np.any(m == np.float32(vmax))
    centers, params = forty_rectangles()
    corners, colors = figures.rect_corners(centers[:3], params[:3]), colors_for(3)
    for cor, col in ((corners, colors), (None, None)):
        got = ctx.draw_outlines(on_device(ctx, m), cor, col, lut=lut, vmin=vmin, vmax=vmax).cpu().numpy()
        want = R.scalar_base(m, lut, vmin, vmax)
        want = R.to_bytes(want if cor is None else R.draw(want, cor, col))
        np.testing.assert_array_equal(got, want)
    # the ends of the range take the ends of the table
    np.testing.assert_array_equal(got[0, 4], R.to_bytes(lut[None, :1])[0, 0])
    np.testing.assert_array_equal(got[0, 5], R.to_bytes(lut[None, 255:])[0, 0])
    np.testing.assert_array_equal(figures.map_picture(m, ctx, vmin=vmin, vmax=vmax),
                                  R.to_bytes(R.scalar_base(m, lut, vmin, vmax)))


def test_the_public_pictures(ctx):
    """``detection_picture`` / ``gt_picture``: corners from the rectangles, colours from the scores, green for the annotation"""
    base = base_picture(H, W, 2)
    rng = np.random.default_rng(11)
    pts = [Rectangle(int(rng.integers(0, H)), int(rng.integers(0, W)), size=float(rng.uniform(4, 9)),
                     ratio=float(rng.uniform(0.3, 0.9)), angle=float(rng.uniform(0, np.pi))) for _ in range(12)]
    scores = rng.uniform(0.1, 3.0, len(pts))
    params = [sra_to_wla(p.size, p.ratio, p.angle) for p in pts]
    corners = figures.rect_corners([(p.x, p.y) for p in pts], params)
    np.testing.assert_array_equal(figures.detection_picture(base, pts, scores, ctx), R.picture(base, corners, R.score_colors(scores)))
    np.testing.assert_array_equal(figures.detection_picture(base, [], [], ctx), R.to_bytes(base))
    labels = {"centers": np.array([[p.x, p.y] for p in pts]), "parameters": np.array(params)}
    np.testing.assert_array_equal(figures.gt_picture(base, labels, ctx), R.picture(base, corners, [(0, 1, 0)] * len(pts)))


def test_bad_arguments_are_refused(ctx):
    from mpp_cnn_rs_object_detection_amd.hip_api import MppError
    base = on_device(ctx, base_picture(H, W, 0))
    far = np.array([[[0, 0], [0, 5], [5, 2 ** 20 + 1], [5, 0]]], dtype=np.int32)
    with pytest.raises(MppError, match="beyond"):
        ctx.draw_outlines(base, far, colors_for(1))
    with pytest.raises(MppError, match="vmin"):
        ctx.draw_outlines(base[:, :, 0].contiguous(), lut=figures.cmap_table(), vmin=1.0, vmax=1.0)
    with pytest.raises(ValueError):
        ctx.draw_outlines(base, np.zeros((2, 4, 2), np.int32), colors_for(1))
