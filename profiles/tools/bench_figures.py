"""What `--figures` adds per image on ONE MI355X: the config-5 scene (4096 x 4096, ~5 000 rectangles, seeded random nets as in
`bench_config5.py`) through `infer_image`, then the three pictures of `MPPModel._write_figures` step by step -- upload of the
float picture (48 MB x 4), outline scatter + compose (`MppContext.draw_outlines`; timed on its own with the picture resident),
copy-out of the 8-bit picture (48 MB), PNG encoding on the host.  Prints one JSON line; best of three."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch
from test_gpu_configs import calibrate_div_clf, make_model, random_nets
from mpp_cnn_rs_object_detection_amd import figures, mappings, synth
from mpp_cnn_rs_object_detection_amd.custom_types import ImageWMaps
from mpp_cnn_rs_object_detection_amd.shapes import Rectangle, sra_to_wla

size = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
img, gt_xy, gt_marks = synth.make_scene_image((size, size), int(5250 * (size / 4096) ** 2), noise=0.02, seed=5)
nets = random_nets()
calibrate_div_clf(nets, img[:1024, :1024])
mpp = make_model("mpp_hrcM.json", nets=nets)
data = ImageWMaps(name="0005", shape=(size, size), image=img, detection_map=None, param_dist_maps=None,
                  mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS, gt_config=[])


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


out = {"image": size}
best = None
for rep in range(3):
    mpp.rng = np.random.default_rng(0)
    region, t_nets = timed(lambda: mpp.region_maps(data))
    (pts, scores), t_infer = timed(lambda: mpp.infer_image(data, region_data=region))
    best = min(best or 1e9, t_nets + t_infer)
out["infer_image_s"], out["detections"] = best, len(pts)

ctx = mpp._figure_ctx()
pts = list(pts)
corners = figures.rect_corners([(p.x, p.y) for p in pts], [sra_to_wla(p.size, p.ratio, p.angle) for p in pts])
colors = figures.score_colors(scores)
dev = torch.device("cuda", 0)
steps = {}
for rep in range(3):
    pic, t_up = timed(lambda: torch.from_numpy(img).to(dev))
    rgb8, t_draw = timed(lambda: ctx.draw_outlines(pic, corners, colors))
    host, t_down = timed(lambda: rgb8.cpu().numpy())
    map8, t_map = timed(lambda: ctx.draw_outlines(region.detection_map, lut=figures.cmap_table(), vmin=0.0, vmax=1.0))
    _, t_whole = timed(lambda: figures.detection_picture(img, pts, scores, ctx))
    t0 = time.perf_counter(); figures.save_png("/dev/null", host); t_png = time.perf_counter() - t0
    for k, v in (("upload_picture_s", t_up), ("scatter_compose_s", t_draw), ("copy_out_s", t_down), ("map_compose_s", t_map),
                 ("detection_picture_s", t_whole), ("png_encode_host_s", t_png)):
        steps[k] = min(steps.get(k, 1e9), v)
out.update(steps)
print(json.dumps(out))
