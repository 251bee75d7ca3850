"""Peak device memory and time of the score-map forward, whole image vs. crops under a budget (profiles/unet_tiled.md),
and the forward's bytes per padded pixel (unet.FORWARD_BYTES_PER_PIXEL).  Random weights, float32.

    python profiles/tools/unet_tiled.py [--size 4096] [--out bench_out/unet_tiled.json]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from mpp_cnn_rs_object_detection_amd import unet  # noqa: E402


def nets(min_fused=None):
    torch.manual_seed(0)
    n = unet.ScoreMapNets(unet.PosNet().eval(), unet.ShapeNet().eval(), device=0)
    if min_fused is not None:
        n.min_fused_pixels = min_fused
    return n


def measure(n, img, budget, reps=3):
    H, W = img.shape[:2]
    n.infer(img, max_pixels=budget)                       # warm-up: kernels, algorithms, allocator pools
    torch.cuda.synchronize()
    n._keep = None
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        out = n.infer(img, max_pixels=budget)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
        del out
    peak = torch.cuda.max_memory_allocated() - base - unet.MAP_BYTES_PER_PIXEL * H * W
    n._keep = None
    plan = unet.chunk_plan((H, W), budget, 3) if budget else [(None, (0, H, 0, W))]
    padded = sum(unet.padded_pixels((c[1] - c[0], c[3] - c[2]), 3) for _, c in plan)
    largest = max(unet.padded_pixels((c[1] - c[0], c[3] - c[2]), 3) for _, c in plan)
    return {"budget": budget, "crops": len(plan), "peak_minus_maps_MiB": peak / 2 ** 20, "ms_median": 1e3 * sorted(times)[len(times) // 2],
            "halo_overhead": padded / (H * W) - 1, "largest_crop_px": largest, "bytes_per_padded_px_of_largest_crop": peak / largest}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default="bench_out/unet_tiled.json")
    a = ap.parse_args()
    g = torch.Generator().manual_seed(1)
    img = torch.rand((a.size, a.size, 3), generator=g).cuda()
    res = {"size": a.size, "gpu": torch.cuda.get_device_name(0), "runs": []}
    n = nets()
    for budget in (None, 2048 * 2048, 1024 * 1024, 640 * 640):
        r = measure(n, img, budget)
        res["runs"].append(r)
        print(json.dumps(r), flush=True)
    # bytes per padded pixel of one forward (maps excluded), both paths: the fused channels-last one (>= min_fused_pixels)
    # and the module one (smaller images)
    res["bytes_per_px"] = {}
    for name, size, mf in (("fused_2048", 2048, None), ("fused_1024", 1024, 0), ("module_992", 992, None), ("module_640", 640, None)):
        r = measure(nets(mf), img[:size, :size].contiguous(), None)
        res["bytes_per_px"][name] = r["bytes_per_padded_px_of_largest_crop"]
        print(name, r, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
