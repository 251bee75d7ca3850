#!/usr/bin/env python3
"""What the local descent does and costs (profiles/descent.md): ``mpp_descend`` against the host walk of
``tests/descent_ref.py`` on the same GPU, host clock around the whole call (both end in a copy back), median of ``--reps``
after a warm-up, profiler off.  Before every repetition the chain gets its starting state back (untimed).

    python profiles/tools/descent_bench.py OUT.json [--reps N] [--walk-reps N] [--rounds R]

* the scene of ``recombine.md`` / ``birth_complete.md``: ``synth.make_mosaic(4, 256, 50, first_tile_id=300, noise=0.2)``,
  1024 x 1024, 800 objects, through ``MPPModel.infer_image`` with the shipped ``config_mpp_log.json`` (seed 5); the descent
  starts from the merged detections, the image as one tile of one context (what ``MPPModel.descend`` builds);
* the walk: per round ``papangelou`` -> the double loop over the candidates -> ``set_points(survivors)``, then
  ``birth_energy_map(marks=True)`` -> both tensors to the host -> the numpy selection -> ``set_points(old + new)``: calls
  this feature did not touch.  The time the walk spends in its two Python selections is reported apart;
* the selection among points alone (``select_points`` on the starting state's points and Papangelou values) next to
  ``papangelou_all`` on the same state: what the scan over the chain's points costs beside the pass that feeds it."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), HERE]
PYTHON_MS = [0.0]


def spread(v):
    return {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "n": len(v)}


def timed_python(fn):
    def wrapped(*a, **k):
        t0 = time.perf_counter()
        out = fn(*a, **k)
        PYTHON_MS[0] += (time.perf_counter() - t0) * 1e3
        return out
    return wrapped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--walk-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=64)
    args = ap.parse_args()
    import logging
    logging.getLogger().setLevel(logging.WARNING)
    import birth_map_bench as B
    import descent_ref
    from mpp_cnn_rs_object_detection_amd.point_set import EPointsSet
    descent_ref.select_points_ref = timed_python(descent_ref.select_points_ref)
    descent_ref.select_minima_ref = timed_python(descent_ref.select_minima_ref)

    data, model, _ = B.model_and_scene(4)
    max_inter = float(max(t.max_dist for t in model.energy_setup.make_energies(data)[1]))
    merged, _ = model.infer_image(data, seed=B.SEED)
    pts = list(merged)
    unit, pair = model.energy_setup.make_energies(data)
    agg = EPointsSet(pts, tuple(data.shape[:2]), unit, pair, image_data=data, point_capacity=max(1024, 2 * len(pts) + 64))
    agg._use(model.energy_model)
    ctx = agg._ctx
    start = ctx.get_points(0)
    res = {"scene": "make_mosaic(4, 256, 50, first_tile_id=300, noise=0.2), 1024 x 1024", "points_before": len(start[0]),
           "point_capacity": ctx.get_option("point_capacity"), "max_rounds": args.rounds, "rows": []}

    def reset():
        ctx.set_points(0, *start)
        ctx.synchronize()

    # the selection's scan beside the pass that feeds it
    import torch
    p = ctx.papangelou_all()
    xy_d = torch.from_numpy(np.ascontiguousarray(start[0], dtype=np.int32)).to(f"cuda:{ctx.device}")
    p_d = torch.from_numpy(np.ascontiguousarray(p[0, :len(start[0])])).to(f"cuda:{ctx.device}")
    t_sel, t_pap = [], []
    for i in range(args.reps + 1):
        t0 = time.perf_counter()
        keep, nc, nk = ctx.select_points(xy_d, p_d, 0.0, 2.0 * max_inter)
        t1 = time.perf_counter()
        ctx.papangelou_all()
        t2 = time.perf_counter()
        if i:
            t_sel.append((t1 - t0) * 1e3)
            t_pap.append((t2 - t1) * 1e3)
    res["selection_alone"] = {"points": len(start[0]), "candidates": nc, "kept": nk, "select_points_ms": spread(t_sel),
                              "papangelou_all_ms": spread(t_pap)}
    print(json.dumps(res["selection_alone"]), flush=True)

    for what, label in ((1, "deaths"), (2, "births"), (3, "deaths and births")):
        ms, rep = [], None
        for i in range(args.reps + 1):                       # (the first one warms up: workspaces, code objects)
            reset()
            e0 = float(ctx.total_energy_all()[0])
            t0 = time.perf_counter()
            rep = ctx.descend(what=what, max_rounds=args.rounds)[0]
            if i:
                ms.append((time.perf_counter() - t0) * 1e3)
        e1 = float(ctx.total_energy_all()[0])
        device = {k: (float(rep[k]) if rep[k].dtype.kind == "f" else int(rep[k])) for k in rep.dtype.names}
        final = ctx.get_points(0)
        wms, wpy, walk = [], [], None
        for i in range(args.walk_reps + 1):
            reset()
            PYTHON_MS[0] = 0.0
            t0 = time.perf_counter()
            walk = descent_ref.host_walk(ctx, 0, max_inter, what=what, max_rounds=args.rounds)
            if i:
                wms.append((time.perf_counter() - t0) * 1e3)
                wpy.append(PYTHON_MS[0])
        same = bool(np.array_equal(final[0], walk["xy"]) and np.array_equal(final[1], walk["marks"]) and
                    device["gain_births"] == walk["gain_births"] and device["gain_deaths"] == walk["gain_deaths"])
        loops = device["rounds"] + (1 if device["status"] == 0 else 0)       # the rounds the loop ran: those that changed the chain and the one that closed it
        row = {"what": label, "device_ms": spread(ms), "rounds_run": loops, "device_ms_per_round": spread(ms)["median"] / max(loops, 1),
               "walk_ms": spread(wms), "walk_ms_in_python_selections": spread(wpy),
               "walk_ms_without_them": spread([a - b for a, b in zip(wms, wpy)]), "report": device, "E_before": e0, "E_after": e1,
               "same_state_and_gains_as_the_walk": same}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
