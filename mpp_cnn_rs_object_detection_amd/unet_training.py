"""Training the two U-Nets (the reference's step 1: ``main.py -p train -m posnet|shapenet``).

* the ``train`` and ``val`` images of a dataset stay on the device (uint8 HWC) with one CSR table of objects per image;
* a patch plan is a small ``(image, anchor row, anchor col)`` table drawn on the host with the recipe of the reference's
  ``data/patch_making.py:17-100`` and ``data/patch_samplers.py:39-200`` (uniform + object samplers), never rasterised;
* ``mpp_train_batch`` (csrc/mpp_train.hip) builds a whole batch -- crop, augmentation, labels -- in one launch (two with
  histogram matching, whose tables a small kernel builds first from the per-image histograms of the resident subset, and
  one more for the patches that draw a spatial op of the recipe: shadow, fog, CLAHE, downscale, median / box blur);
* PosNet's hard-example mining (``pos_net_model.py:234-269, 303-321``): every ``error_update_interval`` epochs each training
  image is forwarded, ``mpp_posnet_error_map`` keeps ``|target mask - predicted mask|`` per 8 x 8 cell as a uint8 density, and
  from then on half of the plan's anchors come from ``mpp_density_anchors`` (``ErrorDensities``);
* ``mpp_posnet_loss`` / ``mpp_shapenet_loss`` compute the loss and its gradient in one launch each, wrapped as
  ``torch.autograd.Function``s; the convolutions and BatchNorm go through PyTorch-ROCm autograd;
* the model directory, ``log.json``, checkpoints, ``model.pt`` and ``model_div_clf.pt`` follow ``utils/training.py:43-83``,
  ``utils/logger.py:36-57`` and ``base/base_model.py:35-49``, so that ``unet.load_torch_model`` / ``ScoreMapNets`` read them.

The patch draws come from the trainer's own ``np.random.Generator(42)``; the reference's process pool pickles its generator
into every worker, so its draws are not reproducible in the first place.
"""
from __future__ import annotations

import glob
import json
import logging
import os
import pickle
import re
import shutil
from datetime import datetime
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import hip_api, unet
from .mappings import ValueMapping
from .paths import fetch_data_paths, get_dataset_base_path, get_model_base_path

KINDS = ("posnet", "shapenet")
CHECKPOINT_INTERVAL = 4          # Logger.log_model(checkpoint_interval=4) in both reference models
POSNET_LR = 1e-3                 # pos_net_model.py:93 hard-codes it
SEED = 42                        # np.random.default_rng(42), and the key of the device draws
DENSITY_WEIGHT = 1 / 2           # d_sampler_weight of pos_net_model.py:319


# ---- configuration ----------------------------------------------------------------------------------------------------------
def check_config(config: Dict, kind: str) -> None:
    """Raise ``NotImplementedError`` naming the key for every option outside what is built; no silent fallback."""
    if kind not in KINDS:
        raise ValueError(f"kind {kind!r}: expected one of {KINDS}")
    loss = config.get("loss", {})
    if loss.get("focal_loss"):
        raise NotImplementedError(f"loss.focal_loss = {loss['focal_loss']!r}: only focal_loss false is built")
    if kind == "posnet":
        if loss.get("target_mode") not in ("uvec", "vec"):
            raise NotImplementedError(f"loss.target_mode = {loss.get('target_mode')!r}: only 'uvec' and 'vec' are built")
        md = loss.get("max_distance")
        if isinstance(md, str) or md is None or isinstance(md, bool):
            raise NotImplementedError(f"loss.max_distance = {md!r}: only a number is built ('auto' is not)")
        for key in ("learn_mask", "compute_relevant", "balanced_mask_loss", "vec_loss_on_prod"):
            if not loss.get(key):
                raise NotImplementedError(f"loss.{key} = {loss.get(key)!r}: only the shipped value true is built")
    else:
        if loss.get("mask_mode") != "shapes":
            raise NotImplementedError(f"loss.mask_mode = {loss.get('mask_mode')!r}: only 'shapes' is built")
        n = config.get("trainer", {}).get("n_classes", 32)
        if not 1 <= int(n) <= hip_api.NCLASS:
            raise NotImplementedError(f"trainer.n_classes = {n!r}: at most {hip_api.NCLASS} classes are built")
    aug = config.get("data_loader", {}).get("augment_params")
    if aug is not None and aug.get("aug_level", "medium") not in ("medium", "strong"):
        raise NotImplementedError(f"data_loader.augment_params.aug_level = {aug.get('aug_level')!r}: 'medium' or 'strong'")


def shipped_config(kind: str) -> Dict:
    """model_configs/posnet/config_pos.json or model_configs/shapenet/config_shape.json"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "posnet/config_pos.json" if kind == "posnet" else "shapenet/config_shape.json"
    with open(os.path.join(repo, "model_configs", name)) as f:
        return json.load(f)


def shape_mappings(config: Dict) -> List[ValueMapping]:
    """size, ratio, angle mappings of ``shape_net_model.py:80-85``"""
    n = int(config.get("trainer", {}).get("n_classes", 32))
    m = config.get("mappings", {})
    return [ValueMapping(n, m.get("size_mapping_min", 0), m.get("size_mapping_max", 32)), ValueMapping(n, 0, 1),
            ValueMapping(n, 0, np.pi, is_cyclic=True)]


def labels_struct(config: Dict, kind: str) -> hip_api.TrainLabelsC:
    lab = hip_api.TrainLabelsC()
    loss = config.get("loss", {})
    if kind == "posnet":
        lab.kind, lab.uvec = 0, int(loss["target_mode"] == "uvec")
        lab.max_distance = float(loss["max_distance"])
        sd = loss.get("bin_map_dil")
        lab.sigma_dil = 0.6 if sd is None else float(sd)
    else:
        lab.kind = 1
        maps = shape_mappings(config)
        lab.n_classes = maps[0].n_classes
        for k, m in enumerate(maps):
            lab.cyclic[k] = int(m.is_cyclic)
            for i, e in enumerate(m.feature_mapping):
                lab.edges[k][i] = float(e)
    return lab


def aug_flags(config: Dict, kind: str, histograms: bool = False, spatial: bool = False) -> int:
    """train-time flags of mpp_train_batch: D4 + photometric when ``augment_params`` is present (utils/training.py:102-106),
    the class perturbation for ShapeNet (shape_net_model.py:87-92).  ``histograms``: the caller builds its batches from a
    ``ResidentSubset`` through a ``BatchBuilder``, which hands the per-image histograms to the context; then, and only
    then, ``hist_match_images`` sets MPP_AUG_HISTMATCH (data/augmentation.py:26-29).  The flag without that table is an
    error of mpp_train_batch, so a caller that has not said so gets the flags of the ops that need no table.
    ``spatial``: with ``augment_params`` also MPP_AUG_SPATIAL, the ops of the recipe that are not one formula per pixel
    (shadow, fog, CLAHE, downscale, median / box blur); it needs a patch size that is a multiple of 8 in 32..512."""
    flags = hip_api.AUG_PERTURB if kind == "shapenet" else 0
    aug = config.get("data_loader", {}).get("augment_params")
    if aug is not None:
        flags |= hip_api.AUG_GEOMETRIC
        flags |= hip_api.AUG_STRONG if aug.get("aug_level", "medium") == "strong" else hip_api.AUG_MEDIUM
        if histograms and aug.get("hist_match_images"):
            flags |= hip_api.AUG_HISTMATCH
        if spatial:
            flags |= hip_api.AUG_SPATIAL
    return flags


def aug_params(mctx: hip_api.MppContext, flags: int, seed: int, epoch: int, batch: int, B: int, P: int,
               n_images: int) -> np.ndarray:
    """What ``mpp_train_batch`` with the same key draws for each of the B patches of a batch: a structured array of
    ``hip_api.AUG_RECORD_DTYPE`` (which ops apply, their parameters, the shadow vertices and the haze points)."""
    return mctx.train_aug_params(flags, seed, epoch, batch, B, P, n_images)


# ---- D4 of objects (host restatement of csrc/mpp_train.hip, used by the tests) ---------------------------------------------
def d4_points(rc: np.ndarray, k: int, flip: int, P: int) -> np.ndarray:
    """pixel coordinates (row, col) under np.rot90 k times, then flip 1 vertical, 2 horizontal, 3 both"""
    r, c = np.asarray(rc, dtype=np.float64)[..., 0].copy(), np.asarray(rc, dtype=np.float64)[..., 1].copy()
    for _ in range(k):
        r, c = P - 1 - c, r
    if flip & 1:
        r = P - 1 - r
    if flip & 2:
        c = P - 1 - c
    return np.stack([r, c], axis=-1)


def d4_angle(angle, k: int, flip: int):
    """angle of the transformed rectangle so that its rect_to_poly polygon is the D4 image of the original, in [0, pi)"""
    t = np.asarray(angle, dtype=np.float64) + k * (np.pi / 2)
    if flip in (1, 2):
        t = -t
    elif flip == 3:
        t = t + np.pi
    m = np.fmod(t, np.pi)
    m = np.where(m < 0, m + np.pi, m)
    return np.where(m >= np.pi, m - np.pi, m)


def d4_image(img: np.ndarray, k: int, flip: int) -> np.ndarray:
    out = np.rot90(img, k, axes=(0, 1))
    if flip & 1:
        out = out[::-1]
    if flip & 2:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


# ---- resident data and the patch plan --------------------------------------------------------------------------------------
class ResidentSubset:
    """The images of ``<dataset>/<subset>`` as one uint8 device buffer plus the CSR object tables."""

    def __init__(self, dataset: str, subset: str, device: int):
        from PIL import Image
        paths = fetch_data_paths(dataset, subset)
        if not paths["images"]:
            raise FileNotFoundError(f"no images in {dataset}/{subset}")
        if not (len(paths["images"]) == len(paths["annotations"]) == len(paths["metadata"])):
            raise ValueError(f"{dataset}/{subset}: images, annotations and metadata differ in number")
        imgs, centers, params, n_obj = [], [], [], []
        ids = [re.match(r"[^0-9]*([0-9]+).*.png", os.path.basename(pf)) for pf in paths["images"]]
        self.ids = [m.group(1) if m else os.path.splitext(os.path.basename(pf))[0] for m, pf in zip(ids, paths["images"])]
        for pf, af, mf in zip(paths["images"], paths["annotations"], paths["metadata"]):
            with Image.open(pf) as im:
                a = np.asarray(im)
            if a.dtype != np.uint8:
                raise ValueError(f"{pf}: only 8-bit images are built")
            imgs.append(np.repeat(a[:, :, None], 3, axis=2) if a.ndim == 2 else a[:, :, :3])
            with open(af, "rb") as f:
                lab = pickle.load(f)
            centers.append(lab["centers"])
            params.append(lab["parameters"])
            with open(mf) as f:
                n_obj.append(int(json.load(f)["n_objects"]))
        self._upload(imgs, centers, params, n_obj, device)

    @classmethod
    def from_arrays(cls, images: Sequence[np.ndarray], centers: Sequence, params: Sequence, device: int) -> "ResidentSubset":
        """uint8 [H,W,3] images with their (row, col) centres and (a, b, angle) parameters (tests, benchmarks)"""
        self = cls.__new__(cls)
        self.ids = [f"{i:04}" for i in range(len(images))]
        self._upload(list(images), list(centers), list(params), [len(np.asarray(c).reshape(-1, 2)) for c in centers], device)
        return self

    def _upload(self, imgs, centers, params, n_obj, device):
        imgs = [np.ascontiguousarray(a, dtype=np.uint8) for a in imgs]
        centers = [np.asarray(c, dtype=np.int64).reshape(-1, 2) for c in centers]
        params = [np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in params]
        starts = np.concatenate([[0], np.cumsum([len(c) for c in centers])]).astype(np.int32)
        self.n_images = len(imgs)
        self.shapes = np.array([a.shape[:2] for a in imgs], dtype=np.int64)
        self.n_objects = np.array(n_obj, dtype=np.int64)
        self.centers = centers
        self.obj_start_host = starts
        off = np.cumsum([0] + [x.size for x in imgs])
        self.img_off_host = off[:-1]
        self._hist = None
        dev = torch.device("cuda", device)
        self.images = torch.from_numpy(np.concatenate([x.ravel() for x in imgs])).to(dev)
        self.img_off = torch.from_numpy(off[:-1].astype(np.int64)).to(dev)
        self.img_hw = torch.from_numpy(self.shapes.astype(np.int32)).to(dev)
        self.obj_start = torch.from_numpy(starts).to(dev)
        n = int(starts[-1])
        # an empty table still gets a valid pointer
        self.obj_centers = torch.from_numpy(np.concatenate(centers).astype(np.int32).reshape(-1, 2) if n else
                                            np.zeros((1, 2), np.int32)).to(dev)
        self.obj_params = torch.from_numpy(np.concatenate(params).reshape(-1, 3) if n else np.zeros((1, 3))).to(dev)
        s = hip_api.TrainDataC()
        s.images, s.img_off, s.img_hw = self.images.data_ptr(), self.img_off.data_ptr(), self.img_hw.data_ptr()
        s.obj_start, s.n_images = self.obj_start.data_ptr(), self.n_images
        s.centers, s.params = self.obj_centers.data_ptr(), self.obj_params.data_ptr()
        self.struct = s

    def histograms(self, mctx: hip_api.MppContext) -> torch.Tensor:
        """[n_images,3,256] counts of the 8-bit values per image and channel, computed on the device at the first call"""
        if self._hist is None:
            self._hist = torch.empty((self.n_images, 3, 256), dtype=torch.int32, device=self.images.device)
            mctx.image_histograms(self.struct, self._hist)
        return self._hist

    def image(self, i: int) -> torch.Tensor:
        """image i as a [H,W,3] uint8 view of the resident buffer"""
        H, W = (int(v) for v in self.shapes[i])
        off = int(self.img_off_host[i])
        return self.images[off:off + H * W * 3].view(H, W, 3)

    def image_centers(self, i: int) -> Optional[torch.Tensor]:
        """the [n,2] int32 centres of image i on the device (None: no objects)"""
        s, e = int(self.obj_start_host[i]), int(self.obj_start_host[i + 1])
        return self.obj_centers[s:e] if e > s else None


def sampler_weights(unf_weight: float, obj_weight: float, with_density: bool = False) -> np.ndarray:
    """MixedSampler's weights: [unf, obj] normalised; with the density sampler ``add_sampler(d, 1/2)``'s
    [unf (1 - 1/2), obj (1 - 1/2), 1/2], normalised again (patch_samplers.py:172-179)"""
    w = np.array([unf_weight, obj_weight], dtype=np.float64)
    w = w / w.sum()
    if with_density:
        w = np.array([wi * (1 - DENSITY_WEIGHT) for wi in w] + [DENSITY_WEIGHT])
        w = w / np.sum(w)
    return w


def sample_density_per_image(shapes: np.ndarray, n_objects: np.ndarray, n_patches: int, unf_weight: float,
                             obj_weight: float, density_sums: Optional[np.ndarray] = None) -> np.ndarray:
    """MixedSampler([UniformSampler, ObjectSampler]).sample_density_per_image (patch_samplers.py:39-200); with
    ``density_sums`` (the per-image sums of the error densities, not all zero) the DensitySampler is the third sampler"""
    n_images = len(shapes)
    if n_images > n_patches:
        raise ValueError(f"{n_images} images but only {n_patches} patches (UniformSampler asserts n_images <= n_patches)")
    pixel_count = shapes[:, 0] * shapes[:, 1]
    dens = []
    for count in (pixel_count, n_objects):
        s = (count / np.sum(count)) * (n_patches - n_images) + 1
        dens.append(s / np.sum(s))
    w = np.array([unf_weight, obj_weight]) / np.sum(np.array([unf_weight, obj_weight]))
    if density_sums is not None:
        sums = np.asarray(density_sums, dtype=np.float64)
        dens.append(sums / np.sum(sums))
        w = sampler_weights(unf_weight, obj_weight, True)
    d = np.sum([wi * di for wi, di in zip(w, dens)], axis=0)
    return d / np.sum(d)


def make_plan(rng: np.random.Generator, data: ResidentSubset, n_patches: int, pm: Dict, densities=None, epoch: int = 0,
              return_samplers: bool = False):
    """[n, 3] int32 (image, anchor row, anchor col): rng.multinomial over the images, then per patch a sampler drawn by
    weight -- uniform anchor, or an object centre + N(0, sigma) -- clipped to [0, shape] (_make_patches, _make_one_patch).

    ``densities`` (an ``ErrorDensities``, or anything with ``sums`` [n_images] and ``anchors(rows, seed, epoch)``) adds the
    DensitySampler with weight 1/2: its rows get their anchors from ``mpp_density_anchors`` in one call, keyed by
    (SEED, epoch) and the plan row; an image whose density sums to 0 gets a uniform anchor (patch_samplers.py:146-147).  If
    every image sums to 0 (the reference would divide 0 by 0) the plan is made without it.  ``return_samplers``: also the
    sampler of every row (0 uniform, 1 object, 2 density)."""
    sums = None if densities is None else np.asarray(densities.sums, dtype=np.int64)
    if sums is not None and sums.sum() == 0:
        logging.warning("every error density sums to 0: this patch plan is made without the density sampler")
        sums = None
    dens = sample_density_per_image(data.shapes, data.n_objects, pm["n_patches"], pm["unf_sampler_weight"],
                                    pm["obj_sampler_weight"], sums)
    w = sampler_weights(pm["unf_sampler_weight"], pm["obj_sampler_weight"], sums is not None)
    sigma = pm.get("obj_sampler_sigma") or 0
    per_image = rng.multinomial(n=n_patches, pvals=dens)
    rows, which_all, drawn = [], [], []
    for i, k in enumerate(per_image):
        shape = data.shapes[i]
        centers = data.centers[i]
        for _ in range(int(k)):
            which = int(rng.choice(len(w), p=w))
            if which == 2 and sums[i] > 0:
                drawn.append((i, len(rows)))
                anchor = (0, 0)                       # filled in below
            elif which == 1 and len(centers) > 0:
                anchor = rng.choice(centers, axis=0).astype(int)
                if sigma != 0:
                    anchor = rng.normal(anchor, sigma).astype(int)
                anchor = np.clip(anchor, (0, 0), shape)
            else:
                anchor = rng.integers((0, 0), shape)
            rows.append((i, int(anchor[0]), int(anchor[1])))
            which_all.append(which)
    plan = np.array(rows, dtype=np.int32).reshape(-1, 3)
    if drawn:
        drawn = np.array(drawn, dtype=np.int32)
        plan[drawn[:, 1], 1:] = densities.anchors(drawn, SEED, epoch)
    return (plan, np.array(which_all, dtype=np.int64)) if return_samplers else plan


def density_anchors_host(dens: np.ndarray, shape, words: np.ndarray) -> np.ndarray:
    """What ``mpp_density_anchors`` computes for one image, restated with numpy: dens [ch,cw] uint8, words the 64-bit Philox
    words of the rows -> [n,2] anchors (the tests compare the kernel with this)"""
    d = np.asarray(dens, dtype=np.uint64)
    rowcum = np.cumsum(d.sum(axis=1, dtype=np.uint64), dtype=np.uint64)
    cellcum = np.cumsum(d, axis=1, dtype=np.uint64)
    total = int(rowcum[-1])
    out = np.zeros((len(words), 2), dtype=np.int64)
    for k, w in enumerate(words):
        r = (int(w) * total) >> 64
        i = int(np.searchsorted(rowcum, np.uint64(r), side="right"))
        rr = r - (int(rowcum[i - 1]) if i else 0)
        j = int(np.searchsorted(cellcum[i], np.uint64(rr), side="right"))
        out[k] = (min(hip_api.DENSITY_CELL * i, int(shape[0])), min(hip_api.DENSITY_CELL * j, int(shape[1])))
    return out


def density_words(rows, seed: int, epoch: int) -> np.ndarray:
    """the 64-bit Philox word of each plan row: key (seed, epoch), counter (row, 0, 3, 0), words (1 << 32 | 0)"""
    out = []
    for r in rows:
        o = hip_api.philox([int(r) & 0xffffffff, 0, 3, 0], [seed & 0xffffffff, epoch & 0xffffffff])
        out.append((int(o[1]) << 32) | int(o[0]))
    return np.array(out, dtype=np.uint64)


class ErrorDensities:
    """PosNet's error densities of the training images, resident on the device: per image a [ceil(H/8), ceil(W/8)] uint8 map
    of ``|target mask - sigmoid(out[2])|`` (block means, 256 levels), their integer prefix tables and sums."""

    def __init__(self, data: ResidentSubset, mctx: hip_api.MppContext, max_distance: float):
        self.data, self.mctx, self.max_distance = data, mctx, float(max_distance)
        dev = data.images.device
        c = hip_api.DENSITY_CELL
        self.cells = -(-data.shapes // c)
        n_cells = self.cells[:, 0] * self.cells[:, 1]
        self.cell_off_host = np.concatenate([[0], np.cumsum(n_cells)]).astype(np.int64)
        self.row_off_host = np.concatenate([[0], np.cumsum(self.cells[:, 0])]).astype(np.int64)
        self.cell_off = torch.from_numpy(self.cell_off_host[:-1].copy()).to(dev)
        self.row_off = torch.from_numpy(self.row_off_host[:-1].copy()).to(dev)
        self.dens = torch.zeros(int(self.cell_off_host[-1]), dtype=torch.uint8, device=dev)
        self.cellcum = torch.zeros(int(self.cell_off_host[-1]), dtype=torch.int32, device=dev)
        self.rowcum = torch.zeros(int(self.row_off_host[-1]), dtype=torch.int64, device=dev)
        self.totals = torch.zeros(data.n_images, dtype=torch.int64, device=dev)
        self.sums = np.zeros(data.n_images, dtype=np.int64)
        self.ready = False

    def map(self, i: int) -> torch.Tensor:
        """the [ch,cw] uint8 density of image i (a view)"""
        a, b = int(self.cell_off_host[i]), int(self.cell_off_host[i + 1])
        return self.dens[a:b].view(int(self.cells[i, 0]), int(self.cells[i, 1]))

    def add(self, i: int, out: torch.Tensor, crop=(0, 0), core=None, cell: Optional[torch.Tensor] = None):
        """the cells of ``core`` (default: all) of image i from the raw PosNet output ``out`` [3,h,w] of the crop at ``crop``;
        the first core of an image (x0 = y0 = 0) restarts its sum"""
        if core is None or (core[0] == 0 and core[2] == 0):
            self.totals[i:i + 1].zero_()
        self.mctx.posnet_error_map(out, self.data.shapes[i], self.data.image_centers(i), self.max_distance, self.map(i),
                                   self.totals[i:i + 1], cell=cell, crop=crop, core=core)

    @torch.no_grad()
    def update(self, model: nn.Module, max_pixels: Optional[int] = None):
        """Forward every image (eval mode, float32; whole when it fits ``max_pixels`` and the device memory, else the crops of
        ``unet.chunk_plan``) and remake the densities, their prefix tables and sums."""
        was_training = model.training
        model.eval()
        depth = model.backbone.depth
        plan_depth = max(depth, 3)                 # cores on multiples of 8: a cell never straddles two crops
        dev = self.data.images.device

        def forward(x):
            padded, _ = unet.pad_before_infer(x, depth)
            return model(padded.unsqueeze(0))[0].contiguous()

        for i in range(self.data.n_images):
            H, W = (int(v) for v in self.data.shapes[i])
            x = self.data.image(i).permute(2, 0, 1).float() / 255
            plan = None
            if max_pixels is not None and unet.padded_pixels((H, W), depth) > max_pixels:
                plan = unet.chunk_plan((H, W), max_pixels, plan_depth)
            else:
                out = None
                try:
                    out = forward(x)
                except torch.cuda.OutOfMemoryError:
                    pass            # (handled outside the except clause, as ScoreMapNets.infer does)
                if out is None:
                    torch.cuda.synchronize(dev)
                    torch.cuda.empty_cache()
                    budget = int(0.8 * torch.cuda.mem_get_info(dev)[0] / unet.FORWARD_BYTES_PER_PIXEL)
                    plan = unet.chunk_plan((H, W), max(budget, 1), plan_depth)
                    logging.warning(f"error densities: the {H} x {W} forward ran out of device memory; tiled under {budget} "
                                    f"pixels per forward ({len(plan)} crops)")
                else:
                    self.add(i, out)
            if plan is not None:
                for core, (cx0, cx1, cy0, cy1) in plan:
                    out = forward(x[:, cx0:cx1, cy0:cy1])
                    self.add(i, out, crop=(cx0, cy0), core=core)
                    del out
        model.train(was_training)
        self.finish()

    def finish(self):
        """prefix tables and host sums of the current maps"""
        self.mctx.density_prefix(self.data.img_hw, self.cell_off, self.row_off, int(self.row_off_host[-1]), self.dens,
                                 self.cellcum, self.rowcum)
        self.sums = self.totals.cpu().numpy().astype(np.int64)
        self.ready = True

    def anchors(self, rows: np.ndarray, seed: int, epoch: int) -> np.ndarray:
        """rows [n,2] (image, plan row) -> [n,2] anchors (``mpp_density_anchors``)"""
        dev = self.dens.device
        r = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 2)).to(dev)
        out = torch.empty_like(r)
        self.mctx.density_anchors(self.data.img_hw, self.cell_off, self.row_off, self.cellcum, self.rowcum, r, seed, epoch, out)
        return out.cpu().numpy()

    def write_pngs(self, directory: str) -> List[str]:
        """``<directory>/<id>.png``: the uint8 maps as gray images, one level per value (what compute_errors leaves behind)"""
        from PIL import Image
        os.makedirs(directory, exist_ok=True)
        host = self.dens.cpu().numpy()
        files = []
        for i, name in enumerate(self.data.ids):
            a, b = int(self.cell_off_host[i]), int(self.cell_off_host[i + 1])
            files.append(os.path.join(directory, f"{name}.png"))
            Image.fromarray(host[a:b].reshape(int(self.cells[i, 0]), int(self.cells[i, 1]))).save(files[-1])
        return files


# ---- the batch builder -----------------------------------------------------------------------------------------------------
class BatchBuilder:
    """Output buffers of mpp_train_batch for one (kind, B, P), reused from batch to batch."""

    def __init__(self, mctx: hip_api.MppContext, labels: hip_api.TrainLabelsC, P: int, device: int, with_dist: bool = False):
        self.mctx, self.labels, self.P, self.dev = mctx, labels, int(P), torch.device("cuda", device)
        self.kind = "posnet" if labels.kind == 0 else "shapenet"
        self.with_dist = with_dist
        self._bufs: Dict[int, Dict[str, torch.Tensor]] = {}
        self.status = torch.zeros(1, dtype=torch.int32, device=self.dev)

    def buffers(self, B: int) -> Dict[str, torch.Tensor]:
        if B not in self._bufs:
            P, d = self.P, self.dev
            b = {"patch": torch.empty((B, 3, P, P), dtype=torch.float32, device=d),
                 "sums": torch.empty((B, (P + hip_api.TRAIN_BAND - 1) // hip_api.TRAIN_BAND, 2), dtype=torch.float64, device=d)}
            if self.kind == "posnet":
                b["vec"] = torch.empty((B, 2, P, P), dtype=torch.float32, device=d)
                b["mask"] = torch.empty((B, P, P), dtype=torch.float32, device=d)
                b["dil"] = torch.empty((B, P, P), dtype=torch.float32, device=d)
                if self.with_dist:
                    b["dist"] = torch.empty((B, P, P), dtype=torch.float32, device=d)
            else:
                b["cls"] = torch.empty((3, B, P, P), dtype=torch.uint8, device=d)
                b["cover"] = torch.empty((B, P, P), dtype=torch.uint8, device=d)
            self._bufs[B] = b
        return self._bufs[B]

    def build(self, data: ResidentSubset, desc: torch.Tensor, flags: int, seed: int, epoch: int, batch: int,
              fresh: bool = False) -> Dict[str, torch.Tensor]:
        """one launch; returns the buffers (fresh: new tensors, not the reused ones)"""
        B = int(desc.shape[0])
        out = dict(self.buffers(B))
        if fresh:
            out = {k: torch.empty_like(v) for k, v in out.items()}
        out["status"] = self.status
        if flags & hip_api.AUG_HISTMATCH:
            self.mctx.train_set_histograms(data.histograms(self.mctx))
        self.mctx.train_batch(data.struct, self.labels, desc, self.P, flags, seed, epoch, batch, out)
        return {k: v for k, v in out.items() if k != "status"}

    def check(self):
        n = int(self.status.item())
        if n:
            raise RuntimeError(f"a patch holds {n} objects, more than the {hip_api.TRAIN_MAX_OBJ} the batch builder keeps in LDS")


# ---- the fused losses as autograd functions --------------------------------------------------------------------------------
class PosNetLossFn(torch.autograd.Function):
    """PointingVectorLoss (+ the divergence classifier's term when w, b are given): returns (loss, vec, mask, div)."""

    @staticmethod
    def forward(ctx, out, w, b, vec, mask, dil, sums, mctx):
        out = out.contiguous()
        res = torch.empty(8, dtype=torch.float64, device=out.device)
        need = out.requires_grad or (w is not None and w.requires_grad) or (b is not None and b.requires_grad)
        grad = torch.empty_like(out) if need else None
        mctx.posnet_loss(out, vec, mask, dil, sums, res, grad=grad,
                         w=None if w is None else w.detach().contiguous(), b=None if b is None else b.detach().contiguous())
        ctx.save_for_backward(grad, res)
        ctx.wshape = None if w is None else (w.shape, b.shape)
        vals = res[:4].float()
        loss, vl, ml, dl = vals[3], vals[0], vals[1], vals[2]
        ctx.mark_non_differentiable(vl, ml, dl)
        return loss, vl, ml, dl

    @staticmethod
    def backward(ctx, g, *_):
        grad, res = ctx.saved_tensors
        gw = gb = None
        if ctx.wshape is not None:
            gw = (res[4].float() * g).reshape(ctx.wshape[0])
            gb = (res[5].float() * g).reshape(ctx.wshape[1])
        return grad * g, gw, gb, None, None, None, None, None


class ShapeNetLossFn(torch.autograd.Function):
    """PixelCELoss over the three heads: returns (loss, loss_feat0, loss_feat1, loss_feat2)."""

    @staticmethod
    def forward(ctx, l0, l1, l2, cls, cover, sums, mctx):
        logits = [t.contiguous() for t in (l0, l1, l2)]
        res = torch.empty(8, dtype=torch.float64, device=l0.device)
        grads = [torch.empty_like(t) for t in logits] if any(t.requires_grad for t in (l0, l1, l2)) else None
        mctx.shapenet_loss(logits, cls, cover, sums, res, grads=grads)
        ctx.save_for_backward(*(grads or []))
        vals = res[:4].float()
        f0, f1, f2 = vals[0], vals[1], vals[2]
        ctx.mark_non_differentiable(f0, f1, f2)
        return vals[3], f0, f1, f2

    @staticmethod
    def backward(ctx, g, *_):
        return tuple(t * g for t in ctx.saved_tensors) + (None, None, None, None)


def posnet_loss(mctx, out, labels: Dict[str, torch.Tensor], div_conv: Optional[nn.Conv2d] = None) -> Dict[str, torch.Tensor]:
    w = b = None
    if div_conv is not None:
        w, b = div_conv.weight, div_conv.bias
    loss, vl, ml, dl = PosNetLossFn.apply(out, w, b, labels["vec"], labels["mask"], labels["dil"], labels["sums"], mctx)
    d = {"vec_loss": vl, "loss": loss, "mask_loss": ml}       # the reference's key order
    if div_conv is not None:
        d["div_loss"] = dl
    return d


def shapenet_loss(mctx, logits: Sequence[torch.Tensor], labels: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    loss, f0, f1, f2 = ShapeNetLossFn.apply(logits[0], logits[1], logits[2], labels["cls"], labels["cover"], labels["sums"], mctx)
    return {"loss_feat0": f0, "loss_feat1": f1, "loss_feat2": f2, "loss": loss}


# ---- the model directory ---------------------------------------------------------------------------------------------------
class TrainLog:
    """utils/logger.py:36-57: lists per key in log.json, a checkpoint every CHECKPOINT_INTERVAL epochs (only the latest kept)"""

    def __init__(self, save_dir: str, log: Optional[Dict] = None):
        self.save_dir, self.log = save_dir, log or {}

    def update(self, epoch: int, metrics: Dict[str, float], model: nn.Module):
        self.log.setdefault("epoch", []).append(epoch)
        self.log.setdefault("timestamp", []).append(datetime.now().strftime("%m/%d/%y-%H:%M:%S"))
        for k, v in metrics.items():
            self.log.setdefault(k, []).append(float(v))
        if epoch % CHECKPOINT_INTERVAL == 0:
            for p in glob.glob(os.path.join(self.save_dir, "checkpoint_*.pt")):
                os.remove(p)
            torch.save(model.state_dict(), os.path.join(self.save_dir, f"checkpoint_{epoch:04}.pt"))
        with open(os.path.join(self.save_dir, "log.json"), "w") as f:
            json.dump(self.log, f, indent=1)


def startup(config: Dict, kind: str, overwrite: bool, resume: bool, model_base: Optional[str]) -> str:
    """utils/training.py:43-83 (startup_config): the model directory and its config.json"""
    save_path = os.path.join(model_base or get_model_base_path(), kind, config["model_name"])
    if os.path.exists(save_path) and not resume:
        if not overwrite:
            raise FileExistsError(f"found model in {save_path} (-o overwrites it, -r resumes)")
        shutil.rmtree(save_path)
    os.makedirs(save_path, exist_ok=True)
    cfg = os.path.join(save_path, "config.json")
    if not os.path.exists(cfg):
        with open(cfg, "w") as f:
            json.dump(config, f, indent=1)
    return save_path


def _world_size() -> int:
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        ws = max(ws, torch.distributed.get_world_size())
    return ws


# ---- the trainer -----------------------------------------------------------------------------------------------------------
def train_unet(config: Dict, kind: str, dataset: Optional[str] = None, device: int = 0, overwrite: bool = False,
               resume: bool = False, model_base: Optional[str] = None) -> str:
    """Train PosNet or ShapeNet as ``main.py -p train -m posnet|shapenet`` does; returns the model directory."""
    check_config(config, kind)
    if _world_size() > 1:
        raise RuntimeError("U-Net training runs on one GPU: start it without torchrun (or with --nproc-per-node 1)")
    if config.get("trainer", {}).get("figure_interval") is not None:
        logging.warning("not built, ignored: trainer.figure_interval (figures)")
    error_interval = config.get("data_loader", {}).get("error_update_interval")
    if error_interval is not None and kind == "shapenet":
        logging.warning("data_loader.error_update_interval: ShapeNet has no error update (nor has the reference's); ignored")
        error_interval = None
    save_path = startup(config, kind, overwrite, resume, model_base)
    dl, tr = config["data_loader"], config["trainer"]
    dataset = dataset or dl["dataset"]
    pm = dl["patch_maker_params"]
    P, batch_size, n_epochs = int(pm["patch_size"]), int(tr["batch_size"]), int(tr["n_epochs"])
    hidden = config.get("model", {}).get("hidden_dims", list(unet.HIDDEN_DIMS))
    dev = torch.device("cuda", device)
    torch.cuda.set_device(dev)

    if kind == "posnet":
        model = unet.PosNet(hidden_dims=hidden).to(dev)
        div_clf = nn.Sequential(nn.Identity(), nn.Conv2d(1, 1, kernel_size=(1, 1))).to(dev) if "div_clf_model" in config else None
    else:
        model = unet.ShapeNet(hidden_dims=hidden, out_feat_size=int(tr.get("n_classes", 32))).to(dev)
        div_clf = None

    last_epoch, log = 0, TrainLog(save_path)
    if resume:
        if os.path.exists(os.path.join(save_path, "log.json")):
            with open(os.path.join(save_path, "log.json")) as f:
                log = TrainLog(save_path, json.load(f))
        if os.path.exists(os.path.join(save_path, "model.pt")):
            logging.info(f"{save_path}/model.pt exists: nothing left to train")
            return save_path
        ck = sorted(glob.glob(os.path.join(save_path, "checkpoint_*.pt")))
        if not ck:
            raise FileNotFoundError(f"nothing to resume from in {save_path}")
        model.load_state_dict(torch.load(ck[-1], map_location=dev, weights_only=True))
        last_epoch = int(re.match(r"checkpoint_([0-9]+).pt", os.path.basename(ck[-1])).group(1))

    params = list(model.parameters()) + (list(div_clf.parameters()) if div_clf is not None else [])
    lr = POSNET_LR if kind == "posnet" else float(config["loss"]["learning_rate"])
    optimizer = torch.optim.Adam(params=params, lr=lr)

    mctx = hip_api.MppContext(device)
    mctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    builder = BatchBuilder(mctx, labels_struct(config, kind), P, device)
    flags_train = aug_flags(config, kind, histograms=True, spatial=True)
    if flags_train & hip_api.AUG_SPATIAL and (P % 8 or not 32 <= P <= 512):
        raise NotImplementedError(f"data_loader.patch_maker_params.patch_size = {P}: the augmentation recipe (CLAHE's 8 x 8 "
                                  "tiles, the fog's haze list) is built for multiples of 8 in 32..512")
    train_data = ResidentSubset(dataset, "train", device)
    val_data = ResidentSubset(dataset, "val", device)
    rng = np.random.default_rng(SEED)
    n_patches = int(pm["n_patches"])
    plan_train = torch.from_numpy(make_plan(rng, train_data, n_patches, pm)).to(dev)
    plan_val = torch.from_numpy(make_plan(rng, val_data, n_patches // 2, pm)).to(dev)
    update_interval = int(dl["dataset_update_interval"])
    # the error densities persist between error updates; a resumed run has none until its next error epoch
    densities = ErrorDensities(train_data, mctx, float(config["loss"]["max_distance"])) if error_interval is not None else None

    def run_epoch(epoch: int, train: bool) -> Dict[str, float]:
        plan, data = (plan_train, train_data) if train else (plan_val, val_data)
        model.train(train)
        if div_clf is not None:
            div_clf.train(train)
        vals: List[torch.Tensor] = []
        keys = None
        for bi, s in enumerate(range(0, len(plan), batch_size)):
            desc = plan[s:s + batch_size]
            lab = builder.build(data, desc, flags_train if train else 0, SEED, epoch, bi)
            with torch.set_grad_enabled(train):
                out = model(lab["patch"])
                if kind == "posnet":
                    d = posnet_loss(mctx, out, lab, div_clf[1] if (train and div_clf is not None) else None)
                else:
                    d = shapenet_loss(mctx, out, lab)
            if train:
                optimizer.zero_grad()
                d["loss"].backward()
                optimizer.step()
            keys = list(d)
            vals.append(torch.stack([v.detach() for v in d.values()]))
        builder.check()
        m = torch.stack(vals).cpu().numpy()
        return {k: float(np.mean(m[:, i])) for i, k in enumerate(keys)}

    for epoch in range(last_epoch, n_epochs):
        train_m = run_epoch(epoch, True)
        val_m = run_epoch(epoch, False)
        print(f"[{epoch:04}] Train " + " ".join(f"{k}: {v:.3f}" for k, v in train_m.items()) + " | Eval " +
              " ".join(f"{k}: {v:.3f}" for k, v in val_m.items()), flush=True)
        log.update(epoch, {**{"train_" + k: v for k, v in train_m.items()}, **{"val_" + k: v for k, v in val_m.items()}}, model)
        if epoch % update_interval == 0 and epoch != 0:
            if densities is not None and epoch % int(error_interval) == 0:
                densities.update(model)
                densities.write_pngs(os.path.join(get_dataset_base_path(), "error_maps", dataset, "train",
                                                  os.path.split(save_path)[1]))
            plan = make_plan(rng, train_data, n_patches, pm, densities if densities is not None and densities.ready else None,
                             epoch)
            plan_train = torch.from_numpy(plan).to(dev)

    torch.save(model.state_dict(), os.path.join(save_path, "model.pt"))
    if div_clf is not None:
        torch.save(div_clf.state_dict(), os.path.join(save_path, "model_div_clf.pt"))
    torch.cuda.synchronize(dev)
    mctx.close()
    return save_path
