"""Host side of the CNN-only baseline's detection step: the host greedy the GPU tests check the device against, pinned to the
reference's recorded output (tests/golden/cnn_baseline_golden.npz), and the box / polygon / hbb-line helpers."""
import math
import os

import numpy as np
import pytest

from helpers import GOLDEN
from mpp_cnn_rs_object_detection_amd import cnn_detection as cd
from mpp_cnn_rs_object_detection_amd import dota_eval

CASES = [("gt", 0.2), ("ge", 0.2), ("gt", 0.7), ("ge", 0.7)]


def ordered_keys(values: np.ndarray, flat: np.ndarray) -> np.ndarray:
    """(order-preserving bits of the float32 value) << 32 | row-major index: the device's rank key (-0 folded onto +0)"""
    v = np.where(values == 0, np.float32(0), values).astype(np.float32)
    b = v.view(np.uint32).astype(np.uint64)
    o = np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)
    return (o << np.uint64(32)) | flat.astype(np.uint64)


def host_greedy(det, thr, strict, nms_distance=6.0):
    """(centres [K,2] int64 in pick order, scores [K] float32, number of candidates): the threshold in float32, candidates sorted
    by key, each kept iff no kept centre lies within nms_distance (sqrt in double) -- utils/nms.py's walk with ties resolved"""
    det = np.asarray(det, dtype=np.float32)
    H, W = det.shape
    t = np.float32(thr)
    mask = det > t if strict else det >= t
    flat = np.flatnonzero(mask)
    vals = det.ravel()[flat]
    order = np.argsort(ordered_keys(vals, flat), kind="stable")[::-1]
    R = int(math.floor(nms_distance))
    dx, dy = np.mgrid[-R:R + 1, -R:R + 1]
    disk = ~(np.sqrt((dx * dx + dy * dy).astype(np.float64)) > nms_distance)
    kept = np.zeros((H + 2 * R, W + 2 * R), bool)
    out = []
    for i in order:
        r, c = divmod(int(flat[i]), W)
        if (kept[r:r + 2 * R + 1, c:c + 2 * R + 1] & disk).any():
            continue
        kept[r + R, c + R] = True
        out.append(i)
    out = np.array(out, dtype=np.int64)
    centers = np.stack([flat[out] // W, flat[out] % W], axis=1).astype(np.int64).reshape(-1, 2)
    return centers, vals[out].astype(np.float32), len(flat)


def mark_maps(cls, tie_rc, tie_k, tie_j):
    """[3][H][W][32] float32 mark maps whose argmax (first maximum) is ``cls`` [3][H][W]: a pattern of multiples of 1/128
    below 0.5, 0.75 at the class, and 0.75 also at class tie_j > cls of the tie pixels (tests/golden/make_cnn_baseline_golden.py records on them)"""
    h, w = cls.shape[1:]
    r = np.arange(h)[:, None, None]
    c = np.arange(w)[None, :, None]
    j = np.arange(32)[None, None, :]
    out = []
    for k in range(3):
        m = (((r * 31 + c * 17 + j * 7 + k * 3) % 64) / 128.0).astype(np.float32)
        np.put_along_axis(m, cls[k][:, :, None].astype(np.int64), np.float32(0.75), axis=2)
        out.append(m)
    for (rr, cc), k, jj in zip(tie_rc, tie_k, tie_j):
        out[k][rr, cc, jj] = np.float32(0.75)
    return out


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "cnn_baseline_golden.npz"))


@pytest.mark.parametrize("rule,thr", CASES)
def test_host_greedy_reproduces_the_reference(golden, rule, thr):
    key = f"{rule}_{int(round(thr * 10))}"
    det = golden["det"]
    centers, scores, n = host_greedy(det, thr, strict=rule == "gt")
    assert n == int(golden[f"{key}_n_cand"])
    mask = det > thr if rule == "gt" else det >= thr
    np.testing.assert_array_equal(np.flatnonzero(mask), golden[f"{key}_cand_flat"])
    np.testing.assert_array_equal(centers, golden[f"{key}_centers"])
    assert scores.dtype == np.float32 and np.array_equal(scores, golden[f"{key}_scores"])


def test_fixture_holds_the_float32_threshold_boundaries(golden):
    det = golden["det"]
    for thr in (0.2, 0.7):
        t = np.float32(thr)
        for v in (np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(2))):
            assert (det == v).sum() == 1
    assert float(np.float32(0.2)) > 0.2 and float(np.float32(0.7)) < 0.7       # rounds up / rounds down
    assert int(golden["gt_2_n_cand"]) + 1 == int(golden["ge_2_n_cand"])


@pytest.mark.parametrize("rule,thr", CASES)
def test_boxes_and_polygons_of_the_recorded_centres(golden, rule, thr):
    key = f"{rule}_{int(round(thr * 10))}"
    c = golden[f"{key}_centers"]
    np.testing.assert_array_equal(cd.posnet_boxes(c), golden[f"{key}_boxes"])
    np.testing.assert_allclose(cd.shapenet_polygons(c, golden[f"{key}_params"]), golden[f"{key}_polys"], rtol=0, atol=1e-9)


def test_box_polygons_and_bound():
    b = cd.posnet_boxes(np.array([[10, 20]]))
    np.testing.assert_array_equal(b, [[14, 4, 26, 16]])
    np.testing.assert_array_equal(cd.box_polygons(b), [[[14, 4], [26, 4], [26, 16], [14, 16]]])
    assert cd.output_bound(4096, 4096, 6.0) == (4096 // 5 + 1) ** 2
    assert cd.output_bound(3, 5, 0.5) == 15


def test_hbb_detection_lines_become_axis_aligned_quads():
    ids, conf, bb = dota_eval.parse_detections(["0007 0.9 1.0 2.0 5.0 7.0\n", "0008 0.25 -3.5 0.0 8.5 12.0", ""], "hbb")
    assert ids == ["0007", "0008"]
    np.testing.assert_array_equal(conf, [0.9, 0.25])
    np.testing.assert_array_equal(bb, [[1, 2, 5, 2, 5, 7, 1, 7], [-3.5, 0, 8.5, 0, 8.5, 12, -3.5, 12]])
    assert dota_eval._convex(bb).all()
    ids, conf, bb = dota_eval.parse_detections(["0001 0.5 0 0 4 0 4 4 0 4"], "obb")
    assert bb.shape == (1, 8)
    with pytest.raises(ValueError):
        dota_eval.parse_detections(["0001 0.5 0 0 4 0 4 4 0 4"], "hbb")
    with pytest.raises(ValueError):
        dota_eval.parse_detections(["0001 0.5 1 2 5 7"], "obb")
    assert dota_eval.parse_detections([], "hbb")[2].shape == (0, 8)
