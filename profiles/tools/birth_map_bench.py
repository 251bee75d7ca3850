#!/usr/bin/env python3
"""What the birth-energy map costs (profiles/birth_map.md): pre-pass + map + summary, timed with HIP events on the ctx's
stream, median of ``--reps`` after a warm-up, profiler off.

    python profiles/tools/birth_map_bench.py OUT.json [--reps N]

* 16 chains of 256 x 256: the 1024 x 1024 synthetic scene of ``restarts_bench.py`` (16 tiles), each tile's chain after the
  shipped ``mpp_log`` schedule (30 003 steps from a naive init);
* one 2048 x 2048 image (the same mosaic, 8 x 8 tiles) with the merged detections ``infer_image`` returns for it;
* the only way before: the candidates of the 64 x 64 sub-lattice (every 4th pixel) of one 256 x 256 tile through
  ``delta_batch`` (host clock: the call ends in its copy back), scaled by the pixel ratio 16 and compared with one chain's
  share of the map."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
SEED = 5


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def model_and_scene(n_side):
    from mpp_cnn_rs_object_detection_amd import mappings, synth
    from mpp_cnn_rs_object_detection_amd.custom_types import ImageWMaps
    from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel
    from mpp_cnn_rs_object_detection_amd.shapes import Rectangle
    det, marks, gt_xy, _ = synth.make_mosaic(n_side=n_side, tile=256, n_objects=50, first_tile_id=300, noise=0.2)
    data = ImageWMaps(name="0000", shape=det.shape, image=None, detection_map=det, param_dist_maps=marks,
                      mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS, gt_config=[])
    with open(os.path.join(REPO, "model_configs", "mpp", "config_mpp_log.json")) as f:
        cfg = json.load(f)
    cwd = os.getcwd()
    os.chdir(REPO)
    try:
        model = MPPModel(cfg, phase="val", load=True)
    finally:
        os.chdir(cwd)
    return data, model, cfg


def timed_maps(ctx, reps, marks=False):
    """[ms] of ``birth_energy_map(summary=True)`` between two events on the ctx's stream"""
    import torch
    st = torch.cuda.Stream()
    ctx.set_stream(st.cuda_stream)
    out, mk, _ = ctx.birth_energy_map(marks=marks)                      # warm-up (and the workspace)
    ms = []
    with torch.cuda.stream(st):
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            _, _, s = ctx.birth_energy_map(out=out, marks=mk if marks else False)
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    ctx.set_stream(None)
    return ms, out, s


def chains_16(reps):
    import numpy as np
    from mpp_cnn_rs_object_detection_amd.data_loaders import crop_image_w_maps
    from mpp_cnn_rs_object_detection_amd.sampler import TileBatchSampler, resolve_schedule
    data, model, cfg = model_and_scene(4)
    p = cfg["inference"]["rjmcmc_params"]
    patch, anchors = model.tile_layout(data.shape[:2])
    tiles = [crop_image_w_maps(data, a, patch) for a in anchors]
    s = TileBatchSampler(tiles, model.energy_setup, model.energy_model, spec_waves=None)
    s.init("naive")
    alpha, Tt, total, snaps = resolve_schedule(1, p["init_temperature"], p["alpha_t"], p["burn_in"], p["samples_interval"],
                                               p["target_temperature"], p.get("iter_multiplier"))
    s.run(total, snaps, 1, p["init_temperature"], alpha, Tt, seed=SEED, chain0=0, as_arrays=True)
    ctx = s.ctx
    ms, out, summ = timed_maps(ctx, reps)
    ms_marks, _, _ = timed_maps(ctx, reps, marks=True)
    row = {"what": "16 chains of 256 x 256", "chains": int(ctx.get_option("n_chains")), "steps": total,
           "points_per_chain": float(ctx.counts().mean()), "map_ms": spread(ms), "map_with_marks_ms": spread(ms_marks),
           "n_negative": [int(v) for v in summ["n_negative"]], "min_dE": [float(v) for v in summ["min_dE"]]}
    # the only way before: delta_batch on the every-4th-pixel lattice of tile 0, with the marks the map reports
    _, cand, _ = ctx.birth_energy_map(marks=True)
    cand = cand[0].cpu().numpy()
    pix = np.stack(np.meshgrid(np.arange(0, 256, 4), np.arange(0, 256, 4), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int32)
    packed = ([[] for _ in pix], [pix[i:i + 1] for i in range(len(pix))], [cand[pix[i, 0], pix[i, 1]][None] for i in range(len(pix))])
    ref = ctx.delta_batch(0, *packed)                                    # warm-up
    got = out[0].cpu().numpy()[pix[:, 0], pix[:, 1]]
    row["max_abs_map_minus_delta_batch"] = float(np.max(np.abs(got - ref)))
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.delta_batch(0, *packed)
        t.append((time.perf_counter() - t0) * 1e3)
    row["delta_batch_4096_cases_ms"] = spread(t)
    row["delta_batch_scaled_to_a_tile_ms"] = statistics.median(t) * 16
    row["map_ms_per_chain"] = statistics.median(ms) / row["chains"]
    row["ratio_delta_batch_over_map"] = row["delta_batch_scaled_to_a_tile_ms"] / row["map_ms_per_chain"]
    print(json.dumps(row), flush=True)
    ctx.close()
    return row


def image_2048(reps):
    from mpp_cnn_rs_object_detection_amd.point_set import EPointsSet
    data, model, _ = model_and_scene(8)
    merged, _ = model.infer_image(data, seed=SEED)
    pts = list(merged)
    unit, pair = model.energy_setup.make_energies(data)
    agg = EPointsSet(pts, tuple(data.shape[:2]), unit, pair, image_data=data, point_capacity=max(1024, len(pts) + 64))
    agg._use(model.energy_model)
    ms, _, summ = timed_maps(agg._ctx, reps)
    row = {"what": "one 2048 x 2048 image, merged detections", "points": len(pts), "map_ms": spread(ms),
           "pre_pass_grid": int(agg._ctx.get_option("birth_map_grid")), "n_negative": int(summ["n_negative"][0]),
           "min_dE": float(summ["min_dE"][0]), "argmin": [int(summ["x"][0]), int(summ["y"][0])]}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import logging
    logging.getLogger().setLevel(logging.WARNING)
    res = {"chains_16": chains_16(args.reps), "image_2048": image_2048(args.reps)}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
