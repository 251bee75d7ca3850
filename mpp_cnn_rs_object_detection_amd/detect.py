"""Run the detector on any image file: ``main.py -p detect -m mpp -c <config> --images PATH [PATH ...] --out DIR``.

No dataset, annotation or ``paths_config`` dataset entry is needed: the picture is read as 8-bit RGB, reduced to the model's
ground sampling distance when it is finer (the float64 anti-aliased rescale of the dataset translation, ``MppContext.rescale``),
handed to ``MPPModel.infer_image`` as an ``ImageWMaps`` that carries only ``image`` (the U-Nets compute the score maps on the
device), and the detections are mapped back to the pixels of the file.  Per image ``<stem>_detections.csv`` (source pixels),
``<stem>_results.pkl`` (the keys of ``infer``'s pickle, in the pixels the model saw, plus ``scale`` and ``source_shape``) and,
with ``figures``, ``<stem>_detection.png`` drawn on the picture the model saw.  With ``inference.birth_map`` of the model's
config (``--birth-map``) also ``<stem>_birth_energy.png`` and the key ``birth_summary`` of the pickle (``MPPModel.birth_map``).
With ``inference.birth_complete`` (``--birth-complete``) the detections are completed from the birth-energy map first
(``MPPModel.complete``): every file shows the completed list and the pickle has the key ``birth_complete``.  With
``inference.descent`` (``--descent``) they go through the local descent (``MPPModel.descend``): every file shows the descended
list and the pickle has the key ``descent``.
"""
from __future__ import annotations

import os
import pickle
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from .custom_types import ImageWMaps
from .dataset_translation import read_rgb, rescale_image_tables
from .mappings import default_mappings
from .shapes import Rectangle, rect_to_poly, sra_to_wla

IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg", ".tif", ".tiff", ".bmp")
CSV_COLUMNS = ["row", "col", "score", "r0", "c0", "r1", "c1", "r2", "c2", "r3", "c3", "size", "ratio", "angle"]


def resolve_scale(gsd: Optional[float], model_gsd: float = 0.5) -> float:
    """``gsd / model_gsd`` (1 without ``gsd``); a picture coarser than the model is refused -- the rescale is a reduction only"""
    if gsd is None:
        return 1.0
    if not (gsd > 0 and model_gsd > 0):
        raise ValueError(f"--gsd {gsd} and --model-gsd {model_gsd} must be positive")
    scale = float(gsd) / float(model_gsd)
    if scale > 1:
        raise ValueError(f"--gsd {gsd} is coarser than --model-gsd {model_gsd}: the picture would have to be enlarged by "
                         f"{scale:.4g}, and only reductions are built")
    return scale


def to_source(p, n_in: int, n_out: int):
    """coordinates along an axis of the picture the model saw (``n_out`` pixels) -> along the same axis of the source
    (``n_in`` pixels): ``(p + 0.5) * n_in / n_out - 0.5``, the rescale's own sampling positions (``rescale_tables``)"""
    if n_in == n_out:
        return np.asarray(p, dtype=np.float64)
    return (np.asarray(p, dtype=np.float64) + 0.5) * n_in / n_out - 0.5


def list_images(paths: Sequence[str]) -> List[str]:
    """the files named, a directory standing for its image files in sorted order"""
    out = []
    for p in paths:
        if os.path.isdir(p):
            out += [os.path.join(p, f) for f in sorted(os.listdir(p)) if f.lower().endswith(IMAGE_EXTENSIONS)]
        elif os.path.isfile(p):
            out.append(p)
        else:
            raise FileNotFoundError(p)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in out]
    if len(set(stems)) != len(stems):
        raise ValueError("two of the images share a file name stem: their results would overwrite each other")
    return out


@dataclass
class DetectResult:
    detections: Any                   # what ``infer_image`` returns: the merged rectangles, in the pixels the model saw
    scores: np.ndarray                # their Papangelou scores
    image: np.ndarray                 # the picture the model saw, float32 [h,w,3] in 0..1
    scale: float
    source_shape: Tuple[int, int]
    birth: Any = None                 # ``inference.birth_map``: (dE [h,w] float64 device tensor, summary dict) of ``MPPModel.birth_map``
    complete: Any = None              # ``inference.birth_complete``: the summary dict of ``MPPModel.complete`` (``detections`` are completed)
    descent: Any = None               # ``inference.descent``: the summary dict of ``MPPModel.descend`` (``detections`` are descended)
    relocate: Any = None              # ``inference.relocate``: the summary dict of ``MPPModel.relocate`` (``detections`` are relocated)
    tempering: Any = None             # ``inference.tempering``: ``last_run["tempering"]`` (exchange rates, the winners' rungs)
    recombine: Any = None             # ``inference.recombine``: ``last_run["recombine"]`` (per tile: status, clusters, energies)

    def polygons(self) -> np.ndarray:
        """[n,4,2] corners in the pixels the model saw (``rect_to_poly`` of (a, b, angle), as ``infer`` stores them)"""
        return np.array([rect_to_poly((p.x, p.y), *sra_to_wla(p.size, p.ratio, p.angle)) for p in self.detections],
                        dtype=np.float64).reshape(-1, 4, 2)

    def rows(self) -> np.ndarray:
        """[n,14] float64, ``CSV_COLUMNS``: centre, score and corners in source pixels, marks as sampled"""
        pts = list(self.detections)
        (H, W), (h, w) = self.source_shape, self.image.shape[:2]
        centers = np.array([[p.x, p.y] for p in pts], dtype=np.float64).reshape(-1, 2)
        poly = self.polygons()
        out = np.zeros((len(pts), len(CSV_COLUMNS)))
        out[:, 0], out[:, 1] = to_source(centers[:, 0], H, h), to_source(centers[:, 1], W, w)
        out[:, 2] = np.asarray(self.scores, dtype=np.float64)
        out[:, 3:11:2], out[:, 4:11:2] = to_source(poly[:, :, 0], H, h), to_source(poly[:, :, 1], W, w)
        out[:, 11:] = np.array([[p.size, p.ratio, p.angle] for p in pts], dtype=np.float64).reshape(-1, 3)
        return out


def detect_image(model, rgb_uint8: np.ndarray, gsd: Optional[float] = None, model_gsd: float = 0.5, seed: Optional[int] = None,
                 name: str = "image") -> DetectResult:
    """One picture, uint8 [H,W,3], through ``model`` (an ``MPPModel`` with nets).  The seed comes from the model's generator, one
    per call, as ``infer`` draws them (``seed``: a seed drawn already)."""
    rgb = np.asarray(rgb_uint8)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"detect_image: expected uint8 [H,W,3], got {rgb.dtype} {rgb.shape}")
    if model.nets is None:
        raise ValueError("detect_image: the model has no nets (main.load_nets)")
    scale = resolve_scale(gsd, model_gsd)
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    if scale != 1.0:
        import torch
        _, tables = rescale_image_tables(H, W, scale)
        src = torch.from_numpy(np.ascontiguousarray(rgb)).to(torch.device("cuda", model.device))
        rgb = model._figure_ctx().rescale(src, tables).cpu().numpy()
    image = np.divide(rgb, 255, dtype=np.float32)                  # as plt.imread gives an 8-bit PNG
    data = ImageWMaps(name=name, shape=tuple(image.shape[:2]), image=image, detection_map=None, param_dist_maps=None,
                      mappings=default_mappings(),
                      param_names=Rectangle.PARAMETERS, labels=None, gt_config=[])
    model.last_birth = model.last_complete = model.last_descent = model.last_relocate = None
    detections, scores = model.infer_image(data, seed=seed)
    return DetectResult(detections=detections, scores=np.asarray(scores, dtype=np.float64), image=image, scale=scale,
                        source_shape=(H, W), birth=getattr(model, "last_birth", None), complete=getattr(model, "last_complete", None),
                        descent=getattr(model, "last_descent", None), relocate=getattr(model, "last_relocate", None),
                        tempering=(getattr(model, "last_run", None) or {}).get("tempering"),
                        recombine=(getattr(model, "last_run", None) or {}).get("recombine"))


def write_results(result: DetectResult, out_dir: str, stem: str, min_score: Optional[float] = None, figures: bool = False,
                  ctx=None) -> None:
    pts = list(result.detections)
    rows = result.rows()
    if min_score is not None:
        rows = rows[rows[:, 2] >= min_score]
    with open(os.path.join(out_dir, f"{stem}_detections.csv"), "w") as f:
        f.write(",".join(CSV_COLUMNS) + "\n")
        for r in rows:
            f.write(",".join(repr(float(v)) for v in r) + "\n")
    record = {"detection": result.polygons(), "detection_points": [p.as_row() for p in pts], "detection_type": "poly",
              "detection_center": np.array([[p.x, p.y] for p in pts]).reshape(-1, 2),
              "detection_score": list(map(float, result.scores)),
              "detection_params": [sra_to_wla(p.size, p.ratio, p.angle) for p in pts],
              "scale": result.scale, "source_shape": tuple(result.source_shape)}
    if result.birth is not None:
        record["birth_summary"] = result.birth[1]
    if result.complete is not None:
        record["birth_complete"] = result.complete
    if result.descent is not None:
        record["descent"] = result.descent
    if result.relocate is not None:
        record["relocate"] = result.relocate
    if result.tempering is not None:
        record["tempering"] = result.tempering
    if result.recombine is not None:
        record["recombine"] = result.recombine
    with open(os.path.join(out_dir, f"{stem}_results.pkl"), "wb") as f:
        pickle.dump(record, f)
    if figures:
        from . import figures as F
        F.save_png(os.path.join(out_dir, f"{stem}_detection.png"), F.detection_picture(result.image, pts, result.scores, ctx))
    if result.birth is not None:
        from . import figures as F
        F.save_png(os.path.join(out_dir, f"{stem}_birth_energy.png"), F.birth_energy_picture(result.birth[0], pts, ctx))


def detect_files(model, paths: Sequence[str], out_dir: str, gsd: Optional[float] = None, model_gsd: float = 0.5,
                 min_score: Optional[float] = None, figures: bool = False) -> List[str]:
    """``-p detect``: every image of ``paths`` in order, one seed of the model's generator each.  Returns the files read."""
    resolve_scale(gsd, model_gsd)                                  # (a refusal comes before any work)
    files = list_images(paths)
    os.makedirs(out_dir, exist_ok=True)
    for path in files:
        stem = os.path.splitext(os.path.basename(path))[0]
        result = detect_image(model, read_rgb(path), gsd=gsd, model_gsd=model_gsd, name=stem)
        write_results(result, out_dir, stem, min_score=min_score, figures=figures,
                      ctx=model._figure_ctx() if figures or result.birth is not None else None)
        print(f"{path}: {len(result.scores)} detection(s)")
    return files
