#!/usr/bin/env python3
"""Generate tests/golden/unet_train_golden.npz by running the REFERENCE's training losses and label processors.

Run only in the build container (the reference is mounted read-only at /root/reference and never travels):

    python tests/golden/make_unet_train_golden.py

Inputs come from tests/unet_train_cases.py (seeded generators); only recorded outputs are written:

* ``PointingVectorLoss`` (learn_mask, compute_relevant, balanced_mask_loss, vec_loss_on_prod) in train form -- with the
  reference's ``Divergence`` + ``Conv2d(1, 1, 1)`` at fixed w, b on ``cat(out[:, :2], sigmoid(out[:, 2:3]))`` -- and in val
  form: the loss dicts, dL/dout, dL/dw, dL/db;
* ``PixelCELoss``: the loss dict and the three dL/dlogits;
* ``ShapePatchProcessor`` (mask_mode shapes, no perturbation) on three patches: value_class_map and loss_mask;
* scipy's ``distance_transform_edt`` of the same patches' centre maps and the dilated map of ``PosPatchProcessor``
  (``exp(-0.5 (d / 0.6)^2)``, zeroed below 1e-5).

``shapes`` mode imports modules that are absent here: empty ``skimage.segmentation`` and ``albumentations`` stubs go into
``sys.modules`` (never called in this mode), and ``skimage.draw`` is the shim under _shim/ with ``polygon2mask`` attached
the way scikit-image defines it (the pixels ``polygon(rows, cols, shape)`` returns).
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shim"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, os.path.dirname(HERE))
sys.path.insert(3, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.ndimage import distance_transform_edt  # noqa: E402

import skimage  # noqa: E402  (the shim)
import skimage.draw as _draw  # noqa: E402


def _polygon2mask(image_shape, polygon):
    polygon = np.asarray(polygon)
    rr, cc = _draw.polygon(polygon[:, 0], polygon[:, 1], image_shape)
    mask = np.zeros(image_shape, dtype=bool)
    mask[rr, cc] = True
    return mask


_draw.polygon2mask = _polygon2mask
seg = types.ModuleType("skimage.segmentation")
seg.watershed = None
sys.modules["skimage.segmentation"] = seg
skimage.segmentation = seg
sys.modules["albumentations"] = types.ModuleType("albumentations")

from model_parts.losses.pixel_ce_loss import PixelCELoss  # noqa: E402
from model_parts.losses.pos_loss import PointingVectorLoss  # noqa: E402
from models.position_net.torch_div import Divergence  # noqa: E402
from models.shape_net.data_loaders import LossMaskParams, ShapePatchProcessor  # noqa: E402
from models.shape_net.mappings import ValueMapping  # noqa: E402

import unet_train_cases as cases  # noqa: E402


def posnet(out_np, vec, mask, dil, with_div):
    out = torch.tensor(out_np, requires_grad=True)
    crit = PointingVectorLoss(learn_mask=True, compute_mask=True, balanced_mask_loss=True, focal_loss=False,
                              vec_loss_on_prod=True)
    div_clf = torch.nn.Sequential(Divergence(div_channels=[0, 1], mask_channel=2), torch.nn.Conv2d(1, 1, kernel_size=(1, 1)))
    with torch.no_grad():
        div_clf[1].weight.fill_(cases.DIV_W)
        div_clf[1].bias.fill_(cases.DIV_B)
    div_score = None
    if with_div:
        div_score = div_clf(torch.concat([out[:, :2], torch.sigmoid(out[:, [2]])], dim=1))
    d = crit(out, torch.tensor(vec), target_mask=torch.tensor(mask), div_score=div_score,
             center_bin_map=torch.tensor(dil) if with_div else None)
    d["loss"].backward()
    rec = {k: np.float64(v.item()) for k, v in d.items()}
    rec["grad"] = out.grad.numpy()
    if with_div:
        rec["dw"] = np.float64(div_clf[1].weight.grad.item())
        rec["db"] = np.float64(div_clf[1].bias.grad.item())
    return rec


def main():
    res = {}
    out, vec, mask, dil = cases.posnet_loss_inputs()
    for form, with_div in (("train", True), ("val", False)):
        for k, v in posnet(out, vec, mask, dil, with_div).items():
            res[f"pos_{form}_{k}"] = v

    logits, cls, cover, loss_mask = cases.shapenet_loss_inputs()
    lt = [torch.tensor(x, requires_grad=True) for x in logits]
    d = PixelCELoss(focal_loss=False)(lt, [torch.tensor(c) for c in cls], loss_mask=torch.tensor(loss_mask))
    d["loss"].backward()
    for k, v in d.items():
        res[f"ce_{k}"] = np.float64(v.item())
    for h in range(3):
        res[f"ce_grad{h}"] = lt[h].grad.numpy()

    maps = [ValueMapping(32, 0, 32), ValueMapping(32, 0, 1), ValueMapping(32, 0, np.pi, is_cyclic=True)]
    proc = ShapePatchProcessor(mappings=maps, class_perturbation_dict=None, rng=np.random.default_rng(0),
                               mask_params=LossMaskParams(mode="shapes"))
    P = cases.LABEL_P
    for i, (c, p) in enumerate(cases.label_patches()):
        patch = np.zeros((P, P, 3), np.float32)
        _, lab = proc.process(patch, c, p, idx=0)
        res[f"shape{i}_cls"] = np.stack([v.numpy() for v in lab["value_class_map"]]).astype(np.uint8)
        res[f"shape{i}_loss_mask"] = lab["loss_mask"].numpy().astype(np.float64)
        binmap = np.zeros((P, P), dtype=bool)
        for cc in c:
            binmap[cc[0], cc[1]] = 1
        dist = distance_transform_edt(1 - binmap)
        dilm = np.exp(-0.5 * np.square(dist / 0.6))
        dilm[dilm < 1e-5] = 0
        res[f"shape{i}_distance"] = dist
        res[f"shape{i}_dil"] = dilm.astype(np.float32)
    # MixedSampler densities of the shipped weights (patch_making.py:29-44), read from metadata files as the reference does
    import json
    import tempfile
    from data.patch_samplers import MixedSampler, ObjectSampler, UniformSampler
    shapes, n_objects = cases.density_images()
    with tempfile.TemporaryDirectory() as tmp:
        metas = []
        for i, (sh, n) in enumerate(zip(shapes, n_objects)):
            metas.append(os.path.join(tmp, f"{i:04}.json"))
            with open(metas[-1], "w") as f:
                json.dump({"shape": [int(sh[0]), int(sh[1])], "n_objects": int(n)}, f)
        rng = np.random.default_rng(42)
        for n_patches in (16384, 300):
            s = MixedSampler(n_patches=n_patches, samplers=[UniformSampler(n_patches=n_patches, patch_size=128, rng=rng),
                                                            ObjectSampler(n_patches=n_patches, patch_size=128, rng=rng, sigma=10)],
                             weights=[0.33, 0.66], rng=rng)
            s.initialise(metas, metas, metas)
            res[f"density_{n_patches}"] = s.sample_density_per_image
    out_path = os.path.join(HERE, "unet_train_golden.npz")
    np.savez_compressed(out_path, **res)
    print(out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
