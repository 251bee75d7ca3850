"""Detection step of the CNN-only baseline: what PosNet and ShapeNet make of their score maps without the point process.

* ``detect_centers``: threshold + greedy distance NMS of a detection map on the device (``mpp_detect_centers``,
  ``csrc/mpp_detect.hip``) -- PosNet's ``np.where(map > min_confidence)`` + ``nms_distance(.., threshold=6)``
  (``position_net/pos_net_model.py:376-380``), ShapeNet's ``>=`` form (``shape_net/shape_net_model.py:283-288``);
* ``mark_params``: ``output_vector_to_value`` + ``sra_to_wla`` at those centres (``shape_net_model.py:323-328``), the argmax
  classes from ``mpp_mark_classes``, the values from the ``ValueMapping`` tables on the host;
* ``posnet_boxes`` / ``box_polygons`` / ``shapenet_polygons``: the boxes and polygons each reference model writes.

Maps are torch tensors on the GPU (as ``unet.ScoreMapNets.infer`` leaves them); numpy arrays are uploaded.  There is no host
fallback: without the HIP library these functions raise.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import numpy as np

from . import hip_api, shapes

NMS_DISTANCE = 6.0      # utils/nms.py is called with threshold=6 by both models
BOX_SIZE = 12           # PosNet's boxes around a centre (pos_net_model.py:387-390)
E_OUTPUT_FULL = -13     # mpp_detect_centers: more centres kept than the output holds

_contexts: Dict[int, "hip_api.MppContext"] = {}


def context(device: int = 0) -> "hip_api.MppContext":
    """One library context per device, shared by the calls of this module."""
    if device not in _contexts:
        _contexts[device] = hip_api.MppContext(device)
    return _contexts[device]


def _on_device(a, device):
    import torch
    if torch.is_tensor(a):
        return a if a.is_cuda else a.to(device if device is not None else 0)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device if device is not None else 0)


def _map2d(det):
    """(H, W, ld) of a float32 [H, W] device map with unit column stride (a view into a wider map is fine)"""
    import torch
    if det.dim() != 2 or det.dtype != torch.float32 or (det.numel() > 1 and det.shape[1] > 1 and det.stride(1) != 1):
        raise ValueError("detect_centers: expected a float32 [H, W] map with unit column stride")
    H, W = int(det.shape[0]), int(det.shape[1])
    if H == 0 or W == 0:
        return H, W, W
    return H, W, max(int(det.stride(0)), W) if H > 1 else W


def output_bound(H: int, W: int, nms_distance: float) -> int:
    """Most centres the NMS can keep on an H x W map: two pixels of one k x k block, k = floor(d / sqrt 2) + 1, lie within d."""
    k = int(math.floor(nms_distance / math.sqrt(2.0))) + 1 if nms_distance >= 1.0 else 1
    return max(1, -(-H // k) * -(-W // k))


def detect_centers(det, min_confidence: float, strict: bool, nms_distance: float = NMS_DISTANCE, device=None,
                   cap: int = None) -> Tuple[np.ndarray, np.ndarray, int]:
    """Kept centres [K, 2] int64 (row, col) in pick order, their scores [K] float32 and the number of candidates.

    Candidates are ``det > min_confidence`` (``strict``, PosNet) or ``det >= min_confidence`` in float32; ties of value go to
    the larger row-major index.  ``cap`` (tests): size of the output buffer, default a bound no map can exceed."""
    import torch
    det = _on_device(det, device)
    H, W, ld = _map2d(det)
    dev = det.device.index
    ctx = context(dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    cap = output_bound(H, W, nms_distance) if cap is None else int(cap)
    xy = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=det.device)
    scores = torch.empty(max(cap, 1), dtype=torch.float32, device=det.device)
    n_cand, n_kept = hip_api.C.c_int64(0), hip_api.C.c_int64(0)
    rc = ctx._L.mpp_detect_centers(ctx._h, H, W, ld, hip_api._ptr(det), float(min_confidence), int(bool(strict)),
                                   float(nms_distance), cap, hip_api._ptr(xy), hip_api._ptr(scores), hip_api.C.byref(n_cand),
                                   hip_api.C.byref(n_kept))
    ctx._check(rc)
    k = int(n_kept.value)
    return xy[:k].cpu().numpy().astype(np.int64), scores[:k].cpu().numpy(), int(n_cand.value)


def mark_classes(marks: Sequence, centers) -> np.ndarray:
    """argmax class (first maximum) of the three mark maps ([H, W, 32] each) at ``centers`` [K, 2]: [K, 3] int64."""
    import torch
    m = [_on_device(x, None) for x in marks]
    dev = m[0].device
    shape = tuple(m[0].shape)
    for x in m:
        if x.dim() != 3 or x.shape[2] != hip_api.NCLASS or tuple(x.shape) != shape or x.dtype != torch.float32 \
                or x.stride(2) != 1 or x.stride(1) != hip_api.NCLASS or x.stride(0) != m[0].stride(0) or x.device != dev:
            raise ValueError("mark_classes: three float32 [H, W, 32] maps with contiguous pixels and one row pitch")
    H, W = shape[0], shape[1]
    ld = int(m[0].stride(0)) // hip_api.NCLASS if H > 1 else W
    c = np.ascontiguousarray(np.asarray(centers, dtype=np.int32).reshape(-1, 2))
    if len(c) == 0:
        return np.zeros((0, 3), np.int64)
    ctx = context(dev.index)
    ctx.set_stream(torch.cuda.current_stream(dev.index).cuda_stream)
    xy = torch.from_numpy(c).to(dev)
    cls = torch.empty((len(c), 3), dtype=torch.int32, device=dev)
    ctx._check(ctx._L.mpp_mark_classes(ctx._h, H, W, ld, hip_api._ptr(m[0]), hip_api._ptr(m[1]), hip_api._ptr(m[2]), len(c),
                                       hip_api._ptr(xy), hip_api._ptr(cls)))
    out = cls.cpu().numpy().astype(np.int64)
    if (out < 0).any():
        raise ValueError("mark_classes: a centre lies outside the map")
    return out


def mark_values(marks: Sequence, centers, mappings) -> np.ndarray:
    """(size, ratio, angle) at ``centers``: ``output_vector_to_value`` read at each centre, [K, 3] float64."""
    cls = mark_classes(marks, centers)
    return np.stack([mappings[k].class_to_value(cls[:, k]) for k in range(3)], axis=1).astype(np.float64).reshape(-1, 3)


def mark_params(marks: Sequence, centers, mappings) -> np.ndarray:
    """ShapeNet's rectangle (w, l, angle) at each centre: ``sra_to_wla`` of ``mark_values``, [K, 3] float64."""
    v = mark_values(marks, centers, mappings)
    w, l, a = shapes.sra_to_wla(v[:, 0], v[:, 1], v[:, 2])
    return np.stack([w, l, a], axis=1).reshape(-1, 3)


def posnet_boxes(centers, size: int = BOX_SIZE) -> np.ndarray:
    """PosNet's boxes ``[c1 - s1, c0 - s1, c1 + s2, c0 + s2]`` (x1, y1, x2, y2; s1 = size // 2, s2 = size - s1), [K, 4]."""
    c = np.asarray(centers, dtype=np.int64).reshape(-1, 2)
    s1 = size // 2
    s2 = size - s1
    return np.stack([c[:, 1] - s1, c[:, 0] - s1, c[:, 1] + s2, c[:, 0] + s2], axis=1)


def box_polygons(boxes) -> np.ndarray:
    """[K, 4, 2] corners (x1,y1) (x2,y1) (x2,y2) (x1,y2) of (x1, y1, x2, y2) boxes (pos_net_model.py:413)"""
    b = np.asarray(boxes).reshape(-1, 4)
    return np.stack([b[:, [0, 1]], b[:, [2, 1]], b[:, [2, 3]], b[:, [0, 3]]], axis=1)


def shapenet_polygons(centers, params) -> np.ndarray:
    """``rect_to_poly(c, w, l, angle)`` of each centre and ShapeNet rectangle, [K, 4, 2] (shape_net_model.py:340-341)"""
    c = np.asarray(centers).reshape(-1, 2)
    p = np.asarray(params, dtype=np.float64).reshape(-1, 3)
    if len(c) == 0:
        return np.zeros((0, 4, 2))
    return np.array([shapes.rect_to_poly(ci, pi[0], pi[1], pi[2]) for ci, pi in zip(c, p)])
