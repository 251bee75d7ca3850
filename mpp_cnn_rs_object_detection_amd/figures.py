"""The result pictures of ``infer``: rectangle outlines over the picture, composed on the device.

Mirrors what the reference draws per image (``models/mpp/mpp_model.py:306-323`` through ``_pred_to_image2`` of
``models/shape_net/display.py:37-59``): ``NNNN_detection.png`` with the detections coloured by Papangelou score through
``plasma`` and ``NNNN_gt.png`` with the annotation in green.  The outlines are scattered and the picture composed by
``csrc/mpp_figures.hip`` (``MppContext.draw_outlines``); only the finished 8-bit picture leaves the device.  DESIGN.md
section 11 states the line rule, the ownership order and the 8-bit rule, and what is left out (the score text).
"""
from __future__ import annotations

import sys

import numpy as np

from .shapes import rect_to_poly, sra_to_wla

GT_COLOR = (0.0, 1.0, 0.0)


def rect_corners(centers, params) -> np.ndarray:
    """[n,4,2] int32 (row, col): ``rect_to_poly(center, short=a, long=b, angle)`` truncated toward zero, as
    ``pts.astype(np.int32)`` of the reference does"""
    polys = [rect_to_poly((c[0], c[1]), short=p[0], long=p[1], angle=p[2]) for c, p in zip(centers, params)]
    return np.trunc(np.asarray(polys, dtype=np.float64).reshape(-1, 4, 2)).astype(np.int32)


def score_colors(scores, cmap: str = "plasma") -> np.ndarray:
    """[n,3] float32: ``cmap(np.clip(score / max_score, 0, max_score))[:3]`` with max_score the largest score (1.0 without
    detections) -- the reference's own expression, upper clip bound included"""
    from matplotlib import pyplot as plt
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    max_score = 1.0 if len(scores) == 0 else float(np.max(scores))
    cm = plt.get_cmap(cmap)
    return np.array([cm(np.clip(s / max_score, 0, max_score))[:3] for s in scores], dtype=np.float32).reshape(-1, 3)


def cmap_table(cmap: str = "plasma") -> np.ndarray:
    """the 256 colours of a matplotlib colormap, [256,3] float32"""
    from matplotlib import pyplot as plt
    return np.asarray(plt.get_cmap(cmap)(np.arange(256))[:, :3], dtype=np.float32)


def _on_device(a, ctx):
    """a float32 picture or map as a contiguous tensor on the ctx's GPU (a tensor already there is borrowed), complete
    before the ctx's stream reads it"""
    import torch
    dev = torch.device("cuda", ctx.device)
    if not hasattr(a, "data_ptr"):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    a = a.to(device=dev, dtype=torch.float32).contiguous()
    torch.cuda.current_stream(dev).synchronize()
    return a


def _picture(image, ctx):
    img = _on_device(image, ctx)
    if img.dim() != 3 or img.shape[2] < 3:
        raise ValueError(f"expected an [H,W,3] picture, got {tuple(img.shape)}")
    return img if img.shape[2] == 3 else img[:, :, :3].contiguous()


def detection_picture(image, detections, scores, ctx, cmap: str = "plasma") -> np.ndarray:
    """``NNNN_detection.png``: image [H,W,3] float32 in 0..1 (numpy, or a tensor on the ctx's GPU); detections an iterable of
    ``Rectangle`` (an ``EPointsSet``, a list); scores their Papangelou scores.  Returns uint8 [H,W,3]."""
    pts = list(detections)
    params = [sra_to_wla(p.size, p.ratio, p.angle) for p in pts]
    corners = rect_corners([(p.x, p.y) for p in pts], params)
    return ctx.draw_outlines(_picture(image, ctx), corners, score_colors(scores, cmap)).cpu().numpy()


def gt_picture(image, labels, ctx) -> np.ndarray:
    """``NNNN_gt.png``: the annotation (``labels['centers']``, ``labels['parameters']`` = (a, b, angle)) in green"""
    corners = rect_corners(labels["centers"], labels["parameters"])
    colors = np.tile(np.asarray(GT_COLOR, dtype=np.float32), (len(corners), 1))
    return ctx.draw_outlines(_picture(image, ctx), corners, colors).cpu().numpy()


def map_picture(det_map, ctx, cmap: str = "plasma", vmin: float = 0.0, vmax: float = 1.0) -> np.ndarray:
    """``NNNN_detection_map.png``: a scalar map [H,W] (the detection map: 0..1) through a colormap"""
    m = _on_device(det_map, ctx)
    if m.dim() != 2:
        raise ValueError(f"expected an [H,W] map, got {tuple(m.shape)}")
    return ctx.draw_outlines(m, lut=cmap_table(cmap), vmin=vmin, vmax=vmax).cpu().numpy()


#: outline colour of the detections on the birth-energy picture (the diverging table runs blue - grey - red)
BIRTH_OUTLINE_COLOR = (0.0, 0.0, 0.0)


def birth_vmax(dE) -> float:
    """colour range of a birth-energy map: the 0.9 quantile of |dE| over its finite values, as the reference's
    ``show_papangelou`` scales its deltas (utils/figures/analyse_mpp.py:25-29); 1.0 when there are none (or when that
    quantile is 0: a range needs a width)"""
    a = np.asarray(dE.detach().cpu().numpy() if hasattr(dE, "data_ptr") else dE, dtype=np.float64).reshape(-1)
    a = np.abs(a[np.isfinite(a)])
    if a.size == 0:
        return 1.0
    q = float(np.quantile(a, 0.9))
    return q if q > 0.0 else 1.0


def birth_energy_picture(dE, detections, ctx, vmax: float = None) -> np.ndarray:
    """``NNNN_birth_energy.png``: the birth-energy map dE [H,W] (``EPointsSet.birth_energy_map``; numpy, or a tensor on the
    ctx's GPU) clipped to [-vmax, vmax] through the 256 colours of ``coolwarm`` -- blue where a birth would lower the energy,
    red where the energy rejects it -- under the outlines of ``detections``.  ``vmax``: ``birth_vmax(dE)`` by default.  The
    scalar path of ``draw_outlines`` does all of it on float32 values; a NaN pixel takes the table's first colour, as that
    path clips it to the lower bound.  Returns uint8 [H,W,3]."""
    if vmax is None:
        vmax = birth_vmax(dE)
    if not (vmax > 0.0 and np.isfinite(vmax)):
        raise ValueError(f"birth_energy_picture: vmax must be positive and finite, got {vmax!r}")
    m = _on_device(dE, ctx)
    if m.dim() != 2:
        raise ValueError(f"expected an [H,W] map, got {tuple(m.shape)}")
    pts = list(detections)
    params = [sra_to_wla(p.size, p.ratio, p.angle) for p in pts]
    corners = rect_corners([(p.x, p.y) for p in pts], params)
    colors = np.tile(np.asarray(BIRTH_OUTLINE_COLOR, dtype=np.float32), (len(corners), 1))
    return ctx.draw_outlines(m, corners, colors, lut=cmap_table("coolwarm"), vmin=-float(vmax), vmax=float(vmax)).cpu().numpy()


def save_png(path: str, rgb: np.ndarray) -> None:
    """uint8 [H,W,3] -> PNG, with whichever of matplotlib or PIL the process has imported already"""
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"save_png: expected uint8 [H,W,3], got {rgb.dtype} {rgb.shape}")
    if "PIL.Image" not in sys.modules and "matplotlib.pyplot" in sys.modules:
        sys.modules["matplotlib.pyplot"].imsave(path, rgb, format="png")
        return
    from PIL import Image
    Image.fromarray(rgb, mode="RGB").save(path, format="PNG")
