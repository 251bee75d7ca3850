"""Sweep `handover_at` (x 256: steps committed per round of 8 at which the hot start hands the chain to the deep rounds), 4.0 to
7.0 in steps of 0.5: the bench tile in this process (best kernel ms of three chains per value), and with --mosaic the 64-tile
mosaic of `bench.py --full --mosaic 4`, one bench process per value (MPP_HANDOVER_AT sets the option in every context).
`python profiles/tools/handover_sweep.py [--mosaic]`"""
import json, os, subprocess, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import bench
from mpp_cnn_rs_object_detection_amd import hip_api, kernels, mappings, synth

VALUES = range(1024, 1792 + 1, 128)


def one_tile():
    setup, model = bench.load_model()
    maps = mappings.default_mappings()
    t = synth.make_tile(512, 200, tile_id=0)
    ctx = hip_api.MppContext(0, point_capacity=1024, spec_waves=8)
    ctx.set_maps(t.det, t.marks); ctx.set_model(model, maps)
    ctx.naive_init(setup.detection_threshold, 6.0)
    ctx.set_kernels(kernels.make_kernels(maps, 1.0), intensity=np.maximum(1, ctx.counts()[:1]).astype(np.float64))
    for at in VALUES:
        ctx.set_option("handover_at", at)
        ms = []
        for _ in range(4):
            ctx.naive_init(setup.detection_threshold, 6.0); ctx.set_schedule(1.0, 0.999, 0.0)
            ctx.run(100001, seed=0); ms.append(ctx.last_kernel_ms())
        print(json.dumps({"handover_at": at, "x": at / 256, "tile_kernel_ms": [round(v, 3) for v in ms[1:]]}), flush=True)


def mosaic():
    for at in VALUES:
        env = dict(os.environ, MPP_HANDOVER_AT=str(at))
        out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--full", "--steps", "1", "--warmup", "0", "--no-cpu-baseline",
                              "--no-convergence", "--scene", "0", "--dataset-images", "0", "--batched-tiles", "0"], env=env, capture_output=True, text=True,
                             timeout=300)
        m = json.loads(out.stdout.strip().splitlines()[-1]).get("mosaic", {})
        print(json.dumps({"handover_at": at, "x": at / 256, "mosaic_chain_kernel_ms": m.get("chain_kernel_ms_rank0"), "mosaic_total_s": m.get("total_s"),
                          "error": m.get("error")}), flush=True)


if __name__ == "__main__":
    mosaic() if "--mosaic" in sys.argv else one_tile()
