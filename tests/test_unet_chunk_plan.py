"""unet.chunk_plan: the crops of a score-map forward under a pixel budget (CPU only)."""
import numpy as np
import pytest

from mpp_cnn_rs_object_detection_amd import unet

DEPTH = 3
ALIGN = 2 ** DEPTH

CASES = [((700, 900), 420 * 420), ((700, 900), 300 * 300), ((203, 331), 200 * 200), ((37, 41), 96 * 104),
         ((2048, 2048), 640 * 640), ((5000, 60), 150 * 150), ((61, 3001), 160 * 160), ((999, 1001), 10 ** 6),
         ((1, 1), 64), ((9, 4000), 104 * 104)]


def check_plan(shape, budget, plan, region=None):
    H, W = shape
    x0, x1, y0, y1 = (0, H, 0, W) if region is None else region
    cover = np.zeros(shape, np.int32)
    for core, crop in plan:
        a, b, c, d = core
        assert x0 <= a < b <= x1 and y0 <= c < d <= y1
        cover[a:b, c:d] += 1
        for v, edge in ((a, x0), (c, y0)):
            assert v == edge or v % ALIGN == 0, (core, "a leading edge off the 2**depth grid")
        for v, edge in ((b, x1), (d, y1)):
            assert v == edge or v % ALIGN == 0, (core, "a trailing edge off the 2**depth grid")
        assert crop == unet.halo_crop(core, shape, align=ALIGN)
        assert unet.padded_pixels((crop[1] - crop[0], crop[3] - crop[2]), DEPTH) <= budget
    inside = cover[x0:x1, y0:y1]
    assert (inside == 1).all(), "the cores must cover every pixel exactly once"
    assert cover.sum() == inside.sum()


@pytest.mark.parametrize("shape,budget", CASES)
def test_cores_tile_the_image_and_crops_fit_the_budget(shape, budget):
    check_plan(shape, budget, unet.chunk_plan(shape, budget, DEPTH))


def test_an_image_within_the_budget_is_one_crop():
    assert unet.chunk_plan((700, 900), unet.padded_pixels((700, 900), DEPTH), DEPTH) == [((0, 700, 0, 900), (0, 700, 0, 900))]


def test_the_plan_has_the_least_halo_overhead_among_equal_core_grids():
    """brute force over every pair of core sizes (multiples of 2**depth) on small shapes"""
    for shape, budget in (((203, 331), 200 * 200), ((150, 500), 128 * 160), ((700, 900), 420 * 420)):
        plan = unet.chunk_plan(shape, budget, DEPTH)
        total = sum(unet.padded_pixels((c[1] - c[0], c[3] - c[2]), DEPTH) for _, c in plan)
        best = None
        for ch in range(ALIGN, shape[0] + ALIGN, ALIGN):
            for cw in range(ALIGN, shape[1] + ALIGN, ALIGN):
                cores = [(a, min(a + ch, shape[0]), c, min(c + cw, shape[1])) for a in range(0, shape[0], ch)
                         for c in range(0, shape[1], cw)]
                crops = [unet.halo_crop(k, shape, align=ALIGN) for k in cores]
                sizes = [unet.padded_pixels((c[1] - c[0], c[3] - c[2]), DEPTH) for c in crops]
                if max(sizes) <= budget and (best is None or sum(sizes) < best):
                    best = sum(sizes)
        assert total == best, (shape, total, best)


def test_a_plan_over_a_region_tiles_the_region_with_crops_in_the_image():
    shape, region, budget = (900, 1200), (130, 610, 75, 1001), 256 * 256
    plan = unet.chunk_plan(shape, budget, DEPTH, region=region)
    assert len(plan) > 4
    check_plan(shape, budget, plan, region)
    assert any(crop[0] < region[0] for _, crop in plan) and any(crop[3] > region[3] for _, crop in plan)  # the halo reaches out


def test_an_impossible_budget_raises():
    with pytest.raises(ValueError, match="no plan fits"):
        unet.chunk_plan((700, 900), 100 * 100, DEPTH)        # the smallest crop: 8-px cores + 2 x 48 px of halo
    with pytest.raises(ValueError):
        unet.chunk_plan((700, 900), 10 ** 5, DEPTH, region=(0, 700, 900, 901))
