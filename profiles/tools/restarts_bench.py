#!/usr/bin/env python3
"""What restarts cost and what they find (profiles/restarts.md): a 1024 x 1024 synthetic scene (16 tiles of 256 px) through
``MPPModel.infer_image`` with ``inference.restarts`` = 1, 2, 4, 8, 16; ``total_energy_all`` against the loop of
``total_energy`` calls it replaces; and ``restarts`` = 1 of this tree against a built copy of the parent commit, the two
alternating in one call.

    python profiles/tools/restarts_bench.py OUT.json [--parent DIR] [--reps N]

Profiler off.  Every shape is warmed up before it is timed.  Wall times are a host clock around ``infer_image``, which ends
in the copy of the merged detections to the host (a synchronise); ``kernel_ms`` is the chain kernels' device time.
``--parent DIR``: a ``git archive`` copy of the parent commit with ``libmppgpu.so`` built in it.  The A/B runs one worker
process per tree (``--worker``), each warmed up, and asks them for one repetition in turn."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SEED = 5


def scene_and_model(root, restarts=None):
    sys.path.insert(0, root)
    import numpy as np  # noqa: F401
    from mpp_cnn_rs_object_detection_amd import mappings, synth
    from mpp_cnn_rs_object_detection_amd.custom_types import ImageWMaps
    from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel
    from mpp_cnn_rs_object_detection_amd.shapes import Rectangle
    det, marks, gt_xy, _ = synth.make_mosaic(n_side=4, tile=256, n_objects=50, first_tile_id=300, noise=0.2)
    data = ImageWMaps(name="0000", shape=det.shape, image=None, detection_map=det, param_dist_maps=marks,
                      mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS, gt_config=[])
    with open(os.path.join(REPO, "model_configs", "mpp", "config_mpp_log.json")) as f:
        cfg = json.load(f)
    if restarts is not None:
        cfg["inference"]["restarts"] = restarts
    cwd = os.getcwd()
    os.chdir(REPO)                           # (paths_config.json and the stored model are resolved from here)
    try:
        model = MPPModel(cfg, phase="val", load=True)
    finally:
        os.chdir(cwd)
    return data, model, len(gt_xy)


def digest(detections, scores):
    import numpy as np
    h = hashlib.sha256()
    h.update(np.asarray([(p.x, p.y, p.size, p.ratio, p.angle) for p in detections], dtype=np.float64).tobytes())
    h.update(np.asarray(scores, dtype=np.float64).tobytes())
    return h.hexdigest()[:16]


def one_run(data, model):
    t0 = time.perf_counter()
    det, scores = model.infer_image(data, seed=SEED)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, float(model.last_run["kernel_ms"]), det, scores


def worker(root):
    """restarts absent: one repetition per line read, answered with a JSON line"""
    import logging
    data, model, _ = scene_and_model(root)
    logging.getLogger().setLevel(logging.WARNING)
    for _ in range(2):
        one_run(data, model)
    print(json.dumps({"ready": root}), flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        wall, kernel, det, scores = one_run(data, model)
        print(json.dumps({"wall_ms": wall, "kernel_ms": kernel, "n": len(det), "digest": digest(det, scores)}), flush=True)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def sweep(reps):
    import logging
    import numpy as np
    out = []
    for R in (1, 2, 4, 8, 16):
        data, model, n_gt = scene_and_model(REPO, R)
        logging.getLogger().setLevel(logging.WARNING)
        one_run(data, model)                                  # warm-up of this shape
        walls, kernels = [], []
        for _ in range(reps):
            wall, kernel, det, scores = one_run(data, model)
            walls.append(wall); kernels.append(kernel)
        run = model.last_run
        n_tiles = len(run["anchors"])
        row = {"restarts": R, "tiles": n_tiles, "chains": R * n_tiles, "wall_ms": spread(walls), "kernel_ms": spread(kernels),
               "kernel_ms_per_chain": statistics.median(kernels) / (R * n_tiles), "detections": len(det), "objects": n_gt,
               "digest": digest(det, scores)}
        if R > 1:
            e, w = run["replica_energy"], run["replica_winner"]
            gain = e[0] - e[w, np.arange(n_tiles)]
            row.update(share_not_replica0=float(np.mean(w != 0)), mean_gain_per_tile=float(np.mean(gain)),
                       energy_replica0=float(e[0].sum()), energy_winners=float(e[w, np.arange(n_tiles)].sum()))
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def energy_call(reps):
    """total_energy_all against n_chains calls of total_energy, on sampled states of 64 and 256 chains"""
    import numpy as np
    from mpp_cnn_rs_object_detection_amd.data_loaders import crop_image_w_maps
    from mpp_cnn_rs_object_detection_amd.sampler import TileBatchSampler, resolve_schedule
    out = []
    for R in (4, 16):
        data, model, _ = scene_and_model(REPO, R)
        patch, anchors = model.tile_layout(data.shape[:2])
        tiles = [crop_image_w_maps(data, a, patch) for a in anchors]
        s = TileBatchSampler(tiles, model.energy_setup, model.energy_model, spec_waves=None, restarts=R)
        s.init("naive")
        alpha, Tt, total, snaps = resolve_schedule(1, 1.0, 0.999, 30000, 1, 0.0)
        s.run(total, snaps, 1, 1.0, alpha, Tt, seed=SEED, chain0=0, as_arrays=True)
        ctx, n = s.ctx, s.ctx.get_option("n_chains")
        both = (ctx.total_energy_all(), np.array([ctx.total_energy(t) for t in range(n)]))      # warm-up of both
        assert np.array_equal(*both)
        t_all, t_loop = [], []
        for _ in range(reps):
            t0 = time.perf_counter(); ctx.total_energy_all(); t_all.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for t in range(n):
                ctx.total_energy(t)
            t_loop.append((time.perf_counter() - t0) * 1e3)
        row = {"chains": n, "points_per_chain": float(ctx.counts().mean()), "total_energy_all_ms": spread(t_all),
               "loop_of_total_energy_ms": spread(t_loop)}
        print(json.dumps(row), flush=True)
        out.append(row)
        ctx.close()
    return out


def ab(parent, reps):
    procs = {}
    for name, root in (("parent", parent), ("this", REPO)):
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root], stdin=subprocess.PIPE,
                                       stdout=subprocess.PIPE, text=True)
    try:
        for p in procs.values():
            assert "ready" in json.loads(p.stdout.readline())
        rows = {"parent": [], "this": []}
        for _ in range(reps):
            for name in ("parent", "this"):
                procs[name].stdin.write("go\n"); procs[name].stdin.flush()
                rows[name].append(json.loads(procs[name].stdout.readline()))
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait(timeout=60)
    res = {}
    for name, r in rows.items():
        res[name] = {"wall_ms": spread([x["wall_ms"] for x in r]), "kernel_ms": spread([x["kernel_ms"] for x in r]),
                     "digests": sorted({x["digest"] for x in r}), "detections": r[0]["n"]}
    # the parent against itself: its even repetitions against its odd ones
    pw = [x["wall_ms"] for x in rows["parent"]]
    res["parent_vs_itself_wall_ms"] = {"even_median": statistics.median(pw[0::2]), "odd_median": statistics.median(pw[1::2])}
    res["same_bytes"] = res["parent"]["digests"] == res["this"]["digests"] and len(res["this"]["digests"]) == 1
    lo, hi = res["parent"]["wall_ms"]["min"], res["parent"]["wall_ms"]["max"]
    res["this_median_within_parent_range"] = lo <= res["this"]["wall_ms"]["median"] <= hi or res["this"]["wall_ms"]["median"] < lo
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--parent")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--worker")
    args = ap.parse_args()
    if args.worker:
        worker(args.worker)
        return
    res = {"sweep": sweep(args.reps), "energy_call": energy_call(20)}
    if args.parent:
        res["r1_against_parent"] = ab(os.path.abspath(args.parent), max(10, 2 * args.reps))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
