#!/usr/bin/env python3
"""The rescale of dataset translation (``MppContext.rescale``, csrc/mpp_rescale.hip) on one GPU:

* ``--kernel``: device-event time of one call (table upload + both kernels of every band) for 2213 x 3553 @ 0.21193735055
  (DOTA image 2781) and a synthetic 16384 x 16384 @ 0.5, after warm-up, over ``--repeats`` calls; bytes moved from shapes;
* ``--scipy`` / ``--scipy-large``: wall time of the scipy restatement (tests/rescale_ref.py) for the first / second input
  on this host, one run each;
* ``--translate``: ``translate_dota`` on the tree the end-to-end test fabricates (five pictures of about 3000 x 3000), the
  per-image split into decode / upload / kernel / download / encode and the wall time of the whole call.

    python profiles/tools/bench_rescale.py --kernel --scipy --translate [--repeats 10] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from mpp_cnn_rs_object_detection_amd import dataset_translation as dt  # noqa: E402

CASES = {"dota_2781": (2213, 3553, 0.21193735055), "synthetic_16k": (16384, 16384, 0.5)}


def picture(H, W):
    rng = np.random.default_rng(0)
    row = rng.integers(0, 256, (1, W, 3), dtype=np.uint8)
    return (row + rng.integers(0, 256, (H, 1, 1), dtype=np.uint8)).astype(np.uint8)      # cheap to make, not flat


def kernel_times(repeats, warmup=3):
    import torch
    from mpp_cnn_rs_object_detection_amd import hip_api
    ctx = hip_api.MppContext(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    res = {}
    for name, (H, W, scale) in CASES.items():
        (oh, ow), tables = dt.rescale_image_tables(H, W, scale)
        src = torch.from_numpy(picture(H, W)).cuda()
        out = torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ms = []
        with torch.cuda.stream(stream):
            for k in range(warmup + repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                ctx.rescale(src, tables, out=out)
                e1.record(stream)
                stream.synchronize()
                if k >= warmup:
                    ms.append(e0.elapsed_time(e1))
        bands = ctx.get_option("rescale_bands")
        # compulsory traffic: the source once, the float64 intermediate written and read once, the 8-bit output
        moved = H * W * 3 + 2 * H * ow * 3 * 8 + oh * ow * 3
        res[name] = {"shape": [H, W], "scale": scale, "out": [oh, ow], "taps": [int(tables[0].shape[1]), int(tables[2].shape[1])],
                     "bands": bands, "workspace_bytes": ctx.get_option("rescale_bytes"), "ms_median": float(np.median(ms)),
                     "ms_min": float(min(ms)), "ms_max": float(max(ms)), "repeats": repeats, "bytes_compulsory": moved,
                     "GBps_of_compulsory": moved / (float(np.median(ms)) * 1e-3) / 1e9}
        print(name, json.dumps(res[name]), flush=True)
        del src, out
    return res


def scipy_time(name):
    from rescale_ref import rescale_ref, to_uint8
    H, W, scale = CASES[name]
    img = picture(H, W)
    c = time.perf_counter()
    to_uint8(rescale_ref(img, scale))
    s = time.perf_counter() - c
    print(f"scipy restatement {name}: {s:.2f} s", flush=True)
    return s


def translate_split():
    from translation_cases import Golden, build_dota_tree, dota_config, write_paths_config
    gold = Golden()
    with tempfile.TemporaryDirectory() as tmp:
        build_dota_tree(os.path.join(tmp, "raw"), gold)
        write_paths_config(tmp)
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            c = time.perf_counter()
            timings = dt.translate_dota(dota_config(os.path.join(tmp, "raw"), gold))
            wall = time.perf_counter() - c
        finally:
            os.chdir(cwd)
    keys = ("decode", "upload", "kernel", "download", "encode")
    for t in sorted(timings, key=lambda t: t["id"]):
        print("image", t["id"], " ".join(f"{k} {t[k]:.4f} s" for k in keys), flush=True)
    total = {k: float(sum(t[k] for t in timings)) for k in keys}
    print("sum over images:", json.dumps(total), f"wall of translate_dota: {wall:.2f} s", flush=True)
    return {"per_image": timings, "sum": total, "wall_s": wall, "workers": min(16, os.cpu_count() or 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--scipy-large", action="store_true")
    ap.add_argument("--translate", action="store_true")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {}
    if a.kernel:
        res["kernel"] = kernel_times(a.repeats)
    if a.translate:
        res["translate"] = translate_split()
    if a.scipy:
        res["scipy_dota_2781_s"] = scipy_time("dota_2781")
    if a.scipy_large:
        res["scipy_synthetic_16k_s"] = scipy_time("synthetic_16k")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
