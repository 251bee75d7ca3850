#!/usr/bin/env python3
"""U-Net training throughput at the shipped configs (B = 64, P = 128, hidden 32..256) on a synthetic dataset:

* patches/s of whole training steps (batch build, forward, loss, backward, Adam), each timed window ending in a device sync;
* one step split by device events: batch build, forward, loss, backward, Adam;
* A/B in the same process: the same step with the losses written as plain torch ops (pos_loss.py / pixel_ce_loss.py);
* ``--no-histmatch``: the same steps without MPP_AUG_HISTMATCH (what the batch build cost before histogram matching);
* ``--no-spatial``: the same steps without MPP_AUG_SPATIAL (what it cost before shadow, fog, CLAHE, downscale and blur);
* ``--build-repeats N``: N more timings of the batch build alone (device events around 20 builds each), for its spread;
* ``--error-update``: one error update of PosNet on the same data (forward of every image + mpp_posnet_error_map, then the
  prefix tables) and one patch plan of the shipped size with density rows (mpp_density_anchors), next to a training epoch.

    python profiles/tools/bench_unet_train.py [--steps 20] [--warmup 5] [--no-histmatch] [--no-spatial] [--error-update]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mpp_cnn_rs_object_detection_amd import hip_api, shapes, synth, unet  # noqa: E402
from mpp_cnn_rs_object_detection_amd import unet_training as ut  # noqa: E402

B, P = 64, 128


def torch_pos(out, lab, conv):
    eps = 1e-5
    s = torch.sigmoid(out[:, 2])
    vec_loss = torch.mean(torch.square(out[:, :2] * torch.stack([s, s], 1) - lab["vec"]))
    m, d = lab["mask"], lab["dil"]
    beta = 1 - torch.sum(m) / m.numel()
    mask_loss = torch.mean(-beta * m * torch.log(s + eps) - (1 - beta) * (1 - m) * torch.log(1 - s + eps))
    div = torch.gradient(out[:, 0], dim=1)[0] + torch.gradient(out[:, 1], dim=2)[0]
    q = torch.sigmoid(conv(torch.unsqueeze(div * s, 1)))[:, 0]
    beta_d = 1 - torch.sum(d) / d.numel()
    div_loss = torch.mean(-beta_d * d * torch.log(q + eps) - (1 - beta_d) * (1 - d) * torch.log(1 - q + eps))
    return vec_loss + mask_loss + div_loss


def torch_shape(logits, lab):
    cover = lab["cover"].double()
    cnt = cover.sum((1, 2), keepdim=True)
    lm = torch.where(cnt > 0, cover / cnt.clamp(min=1), torch.zeros_like(cover))
    loss = 0
    for h in range(3):
        ce = torch.nn.functional.cross_entropy(logits[h], lab["cls"][h].long(), reduction="none")
        loss = loss + torch.mean(torch.sum(ce * lm, dim=(1, 2)))
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-histmatch", action="store_true")
    ap.add_argument("--no-spatial", action="store_true")
    ap.add_argument("--build-repeats", type=int, default=0)
    ap.add_argument("--error-update", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    imgs, cs, ps = [], [], []
    for k in range(4):
        img, xy, marks = synth.make_scene_image((512, 512), 900, seed=k)
        imgs.append((img * 255).astype(np.uint8))
        cs.append(xy)
        ps.append(np.stack(shapes.sra_to_wla(marks[:, 0], marks[:, 1], marks[:, 2]), 1))
    data = ut.ResidentSubset.from_arrays(imgs, cs, ps, 0)
    mctx = hip_api.MppContext(0)
    mctx.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(0)
    desc = torch.tensor(np.stack([rng.integers(0, 4, B), rng.integers(0, 512, B), rng.integers(0, 512, B)], 1).astype(np.int32),
                        device="cuda")
    results = {}
    for kind in ("posnet", "shapenet"):
        cfg = ut.shipped_config(kind)
        bld = ut.BatchBuilder(mctx, ut.labels_struct(cfg, kind), P, 0)
        flags = ut.aug_flags(cfg, kind, histograms=not args.no_histmatch, spatial=not args.no_spatial)
        net = (unet.PosNet() if kind == "posnet" else unet.ShapeNet()).cuda().train()
        conv = torch.nn.Conv2d(1, 1, 1).cuda()
        opt = torch.optim.Adam(list(net.parameters()) + list(conv.parameters()), lr=1e-3)
        for fused in (True, False):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            split = np.zeros(5)

            def step(i, timed):
                if timed:
                    ev[0].record()
                lab = bld.build(data, desc, flags, 42, 0, i)
                if timed:
                    ev[1].record()
                out = net(lab["patch"])
                if timed:
                    ev[2].record()
                if kind == "posnet":
                    loss = ut.posnet_loss(mctx, out, lab, conv)["loss"] if fused else torch_pos(out, lab, conv)
                else:
                    loss = ut.shapenet_loss(mctx, out, lab)["loss"] if fused else torch_shape(out, lab)
                if timed:
                    ev[3].record()
                opt.zero_grad()
                loss.backward()
                if timed:
                    ev[4].record()
                opt.step()
                if timed:
                    ev[5].record()
            for i in range(args.warmup):
                step(i, False)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(args.steps):
                step(i, False)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / args.steps
            for i in range(5):
                step(i, True)
                torch.cuda.synchronize()
                split += [ev[q].elapsed_time(ev[q + 1]) for q in range(5)]
            split /= 5
            name = f"{kind}_{'fused' if fused else 'torch_losses'}"
            results[name] = {"ms_per_step": ms, "patches_per_s": B / ms * 1e3,
                             "split_ms": dict(zip(["batch_build", "forward", "loss", "backward", "adam"], split.round(3).tolist()))}
            print(json.dumps({name: results[name]}), flush=True)
        if args.build_repeats:
            times = []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for r in range(args.build_repeats + 1):                # (the first one warms up)
                e0.record()
                for i in range(20):
                    bld.build(data, desc, flags, 42, 0, i)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) / 20)
            t = np.array(times[1:])
            print(json.dumps({f"{kind}_batch_build_ms": {"flags": flags, "median": round(float(np.median(t)), 4),
                                                         "min": round(float(t.min()), 4), "max": round(float(t.max()), 4),
                                                         "repeats": len(t)}}), flush=True)
    bld.check()
    if args.error_update:
        error_update(data, mctx, results["posnet_fused"]["ms_per_step"])
    mctx.close()


def error_update(data, mctx, ms_per_step):
    """seconds of one error update and milliseconds of the anchors of one plan, next to an epoch of the shipped config"""
    import time
    cfg = ut.shipped_config("posnet")
    pm = cfg["data_loader"]["patch_maker_params"]
    net = unet.PosNet().cuda()
    ed = ut.ErrorDensities(data, mctx, cfg["loss"]["max_distance"])
    ed.update(net)                                       # warm-up: the forward's algorithm search
    torch.cuda.synchronize()
    t = time.perf_counter()
    ed.update(net)
    torch.cuda.synchronize()
    update_s = time.perf_counter() - t
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    out = net(torch.zeros((1, 3, 512, 512), device="cuda"))[0].detach().contiguous()
    e0.record()
    for i in range(data.n_images):
        ed.add(i, out)
    e1.record()
    ed.mctx.density_prefix(data.img_hw, ed.cell_off, ed.row_off, int(ed.row_off_host[-1]), ed.dens, ed.cellcum, ed.rowcum)
    e2.record()
    torch.cuda.synchronize()
    kernel_ms, prefix_ms = e0.elapsed_time(e1), e1.elapsed_time(e2)
    ed.update(net)
    plan, which = ut.make_plan(np.random.default_rng(0), data, pm["n_patches"], pm, ed, epoch=16, return_samplers=True)
    rows = np.stack([plan[which == 2, 0], np.nonzero(which == 2)[0]], 1).astype(np.int32)
    r = torch.from_numpy(rows).cuda()
    a = torch.empty_like(r)
    args_ = (data.img_hw, ed.cell_off, ed.row_off, ed.cellcum, ed.rowcum, r, 42, 16, a)
    mctx.density_anchors(*args_)
    e0.record()
    for _ in range(10):
        mctx.density_anchors(*args_)
    e1.record()
    torch.cuda.synchronize()
    t = time.perf_counter()
    ut.make_plan(np.random.default_rng(0), data, pm["n_patches"], pm, ed, epoch=16)
    plan_s = time.perf_counter() - t
    steps = -(-pm["n_patches"] // B)
    print(json.dumps({"error_update": {
        "images": data.n_images, "update_s": round(update_s, 4), "error_kernel_ms_all_images": round(kernel_ms, 3),
        "prefix_ms": round(prefix_ms, 3), "density_rows": int(len(rows)), "anchors_kernel_ms": round(e0.elapsed_time(e1) / 10, 4),
        "make_plan_host_s": round(plan_s, 3), "epoch_s": round(steps * ms_per_step / 1e3, 2),
        "share_of_16_epochs": round(update_s / (16 * steps * ms_per_step / 1e3), 6)}}), flush=True)


if __name__ == "__main__":
    main()
