#!/usr/bin/env python3
"""Time the CNN-only baseline's detection step (mpp_detect_centers) on synthetic DOTA-density maps.

    python profiles/tools/bench_cnn_detect.py [--sizes 1024 2048 4096] [--thresholds 0.2 0.1] [--reps 5] [--no-host]

Maps: objects on synth.make_gt's 14-px lattice (jittered), a Gaussian bump (sigma 1.2 px) per object over a 0.02 floor, plus
uniform noise in [0, 0.05): about 1 object per 200 px^2, as dense as a DOTA parking lot.  Per size and threshold: candidates,
kept centres, resolve launches, the median wall time of the whole call (host round trips included, from the Python entry to
the centres on the host) and the device time between two events around it, and the test's host greedy on the same map.
Prints one JSON line per case.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def dota_like_map(n: int, seed: int = 9) -> np.ndarray:
    from mpp_cnn_rs_object_detection_amd import synth
    xy, _ = synth.make_gt(n, 10 ** 7, tile_id=seed)
    det = np.full((n, n), 0.02, np.float32)
    yy, xx = np.mgrid[-5:6, -5:6]
    bump = np.exp(-(yy ** 2 + xx ** 2) / (2 * 1.2 ** 2)).astype(np.float32)
    for x, y in xy:
        x0, y0, x1, y1 = max(0, x - 5), max(0, y - 5), min(n, x + 6), min(n, y + 6)
        det[x0:x1, y0:y1] = np.maximum(det[x0:x1, y0:y1], bump[x0 - x + 5:x1 - x + 5, y0 - y + 5:y1 - y + 5])
    det += np.random.default_rng(seed).random(det.shape, dtype=np.float32) * np.float32(0.05)
    return det


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.2, 0.1])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host greedy")
    args = ap.parse_args()
    import torch
    from mpp_cnn_rs_object_detection_amd import cnn_detection as cd
    ctx = cd.context(0)
    for n in args.sizes:
        det_np = dota_like_map(n)
        det = torch.from_numpy(det_np).cuda()
        for thr in args.thresholds:
            cd.detect_centers(det, thr, True)                # warm-up (workspace allocation)
            wall, dev = [], []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                c, s, n_cand = cd.detect_centers(det, thr, True)
                e1.record()
                e1.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(e0.elapsed_time(e1))
            rec = {"size": n, "threshold": thr, "candidates": n_cand, "kept": len(c),
                   "resolve_launches": ctx.get_option("detect_launches"), "wall_ms_median": float(np.median(wall)),
                   "wall_ms_min": float(np.min(wall)), "event_ms_median": float(np.median(dev))}
            if not args.no_host:
                from test_cnn_detection_host import host_greedy
                t0 = time.perf_counter()
                hc, hs, hn = host_greedy(det_np, thr, True)
                rec["host_greedy_s"] = time.perf_counter() - t0
                rec["host_equal"] = bool(hn == n_cand and np.array_equal(hc, c) and np.array_equal(hs, s))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
