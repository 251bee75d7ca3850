#!/usr/bin/env python3
"""What the greedy completion costs (profiles/birth_complete.md): ``mpp_birth_complete`` against the host walk it replaces,
host clock around the whole call (both end in a copy back), median of ``--reps`` after a warm-up, profiler off.  Before every
repetition the chains get their starting state back (untimed).

    python profiles/tools/birth_complete_bench.py OUT.json --what device|walk [--reps N]

``--what walk`` needs nothing this feature added: with ``MPP_LIB_PATH`` pointing at the library of the commit before it, the
walk is timed on that library (the two new symbols are then not looked up).

* 16 chains of 256 x 256 and one 2048 x 2048 image: the scenes and the chains' end states of ``birth_map_bench.py``;
* the walk: per round ONE ``birth_energy_map(marks=True)`` for all chains, both tensors to the host, the numpy selection of
  ``tests/birth_complete_ref.py`` per open chain, ``set_points(old + new)`` per chain that grew."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), HERE]
MAX_ROUNDS = 16
SELECT_MS = []                                               # per walk: the time spent in the numpy selection (a Python loop)


def walk_all(ctx, max_inter):
    from birth_complete_ref import select_minima_ref
    T, cap = ctx.get_option("n_chains"), ctx.get_option("point_capacity")
    state = [(xy.astype(np.int32), mk.copy()) for xy, mk in ctx.get_points_all()]
    rep = [dict(status=-1, rounds=0, n_added=0, gain=0.0) for _ in range(T)]
    SELECT_MS.append(0.0)
    while any(r["status"] < 0 for r in rep):
        dE, cand, _ = ctx.birth_energy_map(marks=True)
        d, c = dE.cpu().numpy(), cand.cpu().numpy()
        for t in range(T):
            r = rep[t]
            if r["status"] >= 0:
                continue
            t0 = time.perf_counter()
            kxy, kv, _ = select_minima_ref(d[t], 0.0, 2.0 * max_inter)
            SELECT_MS[-1] += (time.perf_counter() - t0) * 1e3
            if len(kxy) == 0:
                r["status"] = 0
                continue
            xy, mk = state[t]
            if len(xy) + len(kxy) > cap:
                r["status"] = 2
                continue
            for v in kv:
                r["gain"] += float(v)
            state[t] = (np.concatenate([xy, kxy]).astype(np.int32), np.concatenate([mk, c[t][kxy[:, 0], kxy[:, 1]]]))
            ctx.set_points(t, *state[t])
            r["rounds"] += 1
            r["n_added"] += len(kxy)
            if r["rounds"] >= MAX_ROUNDS:
                r["status"] = 1
    return rep


def device_all(ctx, max_inter):
    return [dict(status=int(r["status"]), rounds=int(r["rounds"]), n_added=int(r["n_added"]), gain=float(r["gain"]))
            for r in ctx.birth_complete(max_rounds=MAX_ROUNDS)]


def timed(ctx, fn, reps, max_inter):
    start = [(xy.copy(), mk.copy()) for xy, mk in ctx.get_points_all()]
    ms, rep = [], None
    for i in range(reps + 1):                                # (the first one warms up: workspaces, code objects)
        for t, (xy, mk) in enumerate(start):
            ctx.set_points(t, xy, mk)
        ctx.synchronize()
        t0 = time.perf_counter()
        rep = fn(ctx, max_inter)
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
    spread = lambda v: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "n": len(v)}
    sel = SELECT_MS[-len(ms):] if SELECT_MS else []
    rest = spread([a - b for a, b in zip(ms, sel)]) if sel else None          # the walk without its Python loop
    del SELECT_MS[:]
    return spread(ms), rest, rep, start


def row(what, ctx, fn, reps, max_inter):
    ms, rest, rep, start = timed(ctx, fn, reps, max_inter)
    out = {"what": what, "chains": len(rep), "points_before": [len(xy) for xy, _ in start], "ms": ms,
           "ms_without_the_numpy_selection": rest,
           "rounds": [r["rounds"] for r in rep], "n_added": [r["n_added"] for r in rep], "status": [r["status"] for r in rep],
           "gain": [r["gain"] for r in rep], "points_after": [int(v) for v in ctx.counts()]}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--what", choices=["device", "walk"], required=True)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import logging
    logging.getLogger().setLevel(logging.WARNING)
    from mpp_cnn_rs_object_detection_amd import hip_api
    if args.what == "walk" and os.environ.get("MPP_LIB_PATH"):
        for name in ("mpp_select_minima", "mpp_birth_complete"):
            hip_api.PROTOTYPES.pop(name, None)
    fn = device_all if args.what == "device" else walk_all
    import birth_map_bench as B
    from mpp_cnn_rs_object_detection_amd.data_loaders import crop_image_w_maps
    from mpp_cnn_rs_object_detection_amd.point_set import EPointsSet
    from mpp_cnn_rs_object_detection_amd.sampler import TileBatchSampler, resolve_schedule
    res = {"what": args.what, "library": os.environ.get("MPP_LIB_PATH") or "this commit's"}

    data, model, cfg = B.model_and_scene(4)
    max_inter = float(max(t.max_dist for t in model.energy_setup.make_energies(data)[1]))
    p = cfg["inference"]["rjmcmc_params"]
    patch, anchors = model.tile_layout(data.shape[:2])
    s = TileBatchSampler([crop_image_w_maps(data, a, patch) for a in anchors], model.energy_setup, model.energy_model, spec_waves=None)
    s.init("naive")
    alpha, Tt, total, snaps = resolve_schedule(1, p["init_temperature"], p["alpha_t"], p["burn_in"], p["samples_interval"],
                                               p["target_temperature"], p.get("iter_multiplier"))
    s.run(total, snaps, 1, p["init_temperature"], alpha, Tt, seed=B.SEED, chain0=0, as_arrays=True)
    res["chains_16"] = row("16 chains of 256 x 256, the chains' end state", s.ctx, fn, args.reps, max_inter)
    s.ctx.close()

    data, model, _ = B.model_and_scene(8)
    merged, _ = model.infer_image(data, seed=B.SEED)
    pts = list(merged)
    unit, pair = model.energy_setup.make_energies(data)
    agg = EPointsSet(pts, tuple(data.shape[:2]), unit, pair, image_data=data, point_capacity=max(1024, 2 * len(pts) + 64))
    agg._use(model.energy_model)
    res["image_2048"] = row("one 2048 x 2048 image, merged detections", agg._ctx, fn, args.reps, max_inter)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
