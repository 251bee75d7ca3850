#!/usr/bin/env python3
"""Generate tests/golden/cnn_baseline_golden.npz by running the REFERENCE's detection step of the CNN-only baseline.

Run only in the build container (the reference is mounted read-only at /root/reference and never travels):

    python tests/golden/make_cnn_baseline_golden.py

Input: a 256 x 320 detection map of Gaussian blobs whose candidate values are all distinct (so the unstable
``np.argsort`` of ``utils/nms.py`` has no tie to order), plus isolated pixels at exactly float32(thr) and its two float32
neighbours for thr = 0.2 (float32 rounds up) and 0.7 (rounds down); three mark maps rebuilt exactly from uint8 class maps
(``tests/test_cnn_detection_host.mark_maps``) with a few pixels whose two top classes tie.

Recorded with the reference's ``utils.nms.nms_distance``, ``models.shape_net.mappings.output_vector_to_value``,
``base.shapes.rectangle.sra_to_wla`` and ``rect_to_poly``, for ``>`` (PosNet, pos_net_model.py:376-390) and ``>=``
(ShapeNet's PosNet call, shape_net_model.py:283-341) at both thresholds: the candidates in ``np.where`` order and their
scores (as row-major flat indices; the scores are det's), the NMS centres and scores in pick order, PosNet's 12-px boxes, ShapeNet's (w, l, angle) and polygons.
Only arrays are written; no reference source is copied.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, os.path.dirname(HERE))
sys.path.insert(3, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

from base.shapes.rectangle import rect_to_poly, sra_to_wla  # noqa: E402
from models.shape_net.mappings import ValueMapping, output_vector_to_value  # noqa: E402
from utils.nms import nms_distance  # noqa: E402

from test_cnn_detection_host import mark_maps  # noqa: E402  (the tests rebuild the mark maps the same way)

H, W = 256, 320
THRESHOLDS = (0.2, 0.7)
RULES = ("gt", "ge")             # det > thr (PosNet), det >= thr (ShapeNet / naive_detection)


def make_inputs(seed=7):
    rng = np.random.default_rng(seed)
    n_obj = 300
    cen = np.stack([rng.uniform(4, H - 4, n_obj), rng.uniform(4, W - 4, n_obj)], axis=1)
    peak = rng.uniform(0.25, 1.0, n_obj)
    sig = rng.uniform(1.2, 2.6, n_obj)
    rr, cc = np.mgrid[0:H, 0:W]
    det = np.zeros((H, W), np.float64)
    owner = np.full((H, W), -1)
    for i in range(n_obj):
        g = peak[i] * np.exp(-((rr - cen[i, 0]) ** 2 + (cc - cen[i, 1]) ** 2) / (2 * sig[i] ** 2))
        upd = g > det
        det[upd], owner[upd] = g[upd], i
    det[det < 0.15] = 0.0
    det = det.astype(np.float32)
    special = [np.float32(t) for t in THRESHOLDS]
    special = [v for t in special for v in (np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(2)))]
    # distinct candidate values, none equal to a boundary value
    nz = np.flatnonzero(det)
    used = set(float(v) for v in special)
    for i in nz[np.argsort(det.ravel()[nz], kind="stable")]:
        v = det.flat[i]
        while float(v) in used:
            v = np.nextafter(v, np.float32(2))
        det.flat[i] = v
        used.add(float(v))
    # isolated boundary pixels (nothing else within 8 px)
    spots = []
    for v in special:
        while True:
            r, c = int(rng.integers(8, H - 8)), int(rng.integers(8, W - 8))
            if not det[r - 8:r + 9, c - 8:c + 9].any():
                break
        det[r, c] = v
        spots.append((r, c))
    # mark classes: constant per blob, a coarse pattern elsewhere; ties at some blob pixels
    blob_cls = rng.integers(0, 31, (3, n_obj))
    cls = np.empty((3, H, W), np.uint8)
    for k in range(3):
        cls[k] = np.where(owner >= 0, blob_cls[k][np.maximum(owner, 0)], (rr // 16 + cc // 16 + 5 * k) % 32)
    hot = np.argwhere(det >= np.float32(0.2))
    pick = rng.choice(len(hot), 24, replace=False)
    tie_rc = hot[pick].astype(np.int32)
    tie_k = (np.arange(24) % 3).astype(np.int32)
    tie_j = np.array([int(rng.integers(cls[k, r, c] + 1, 32)) for (r, c), k in zip(tie_rc, tie_k)], np.int32)
    for (r, c), k in zip(tie_rc, tie_k):
        assert cls[k, r, c] < 31
    return det, cls, tie_rc, tie_k, tie_j, np.array(spots, np.int32)


def main():
    det, cls, tie_rc, tie_k, tie_j, spots = make_inputs()
    marks = mark_maps(cls, tie_rc, tie_k, tie_j)
    mappings = [ValueMapping(32, 0, 32), ValueMapping(32, 0, 1), ValueMapping(32, 0, np.pi, is_cyclic=True)]
    values_map = output_vector_to_value([np.expand_dims(np.moveaxis(m, -1, 0), 0) for m in marks], mappings)
    out = dict(det=det, mark_cls=cls, tie_rc=tie_rc, tie_k=tie_k, tie_j=tie_j, spots=spots,
               thresholds=np.array(THRESHOLDS), nms_distance=np.float64(6.0))
    for thr in THRESHOLDS:
        for rule in RULES:
            key = f"{rule}_{int(round(thr * 10))}"
            mask = det > thr if rule == "gt" else det >= thr
            cand = np.array(np.where(mask)).T
            cscore = det[cand[:, 0], cand[:, 1]]
            assert len(np.unique(cscore)) == len(cscore)
            centers, scores = nms_distance(cand, cscore, threshold=6)
            centers = np.array(centers, np.int64).reshape(-1, 2)
            scores = np.array(scores, np.float32)
            boxes = np.array([[c[1] - 6, c[0] - 6, c[1] + 6, c[0] + 6] for c in centers], np.int64).reshape(-1, 4)
            params = np.array([sra_to_wla(values_map[0][0][c[0], c[1]], values_map[1][0][c[0], c[1]], values_map[2][0][c[0], c[1]])
                               for c in centers], np.float64).reshape(-1, 3)
            polys = np.array([rect_to_poly(c, p[0], p[1], p[2]) for c, p in zip(centers, params)], np.float64).reshape(-1, 4, 2)
            classes = np.stack([np.argmax(m[centers[:, 0], centers[:, 1]], axis=1) for m in marks], axis=1).astype(np.int64)
            out.update({f"{key}_n_cand": np.int64(len(cand)), f"{key}_cand_flat": (cand[:, 0] * W + cand[:, 1]).astype(np.int32),
                        f"{key}_centers": centers.astype(np.int32),
                        f"{key}_scores": scores, f"{key}_boxes": boxes.astype(np.int32), f"{key}_params": params,
                        f"{key}_polys": polys, f"{key}_classes": classes.astype(np.uint8)})
            print(f"{key}: {len(cand)} candidates, {len(centers)} kept")
    path = os.path.join(HERE, "cnn_baseline_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
