"""The tiled score-map forward: window epilogues, crops under a pixel budget, the out-of-memory fallback, and the
plumbing up to main.py.  Random weights (test_unet.recipe_state_dict); what the maps 'detect' is meaningless."""
import copy
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import REPO
from test_gpu_pipeline import synthetic_dataset, write_image  # noqa: F401  (a fixture)
from test_unet import recipe_state_dict
from mpp_cnn_rs_object_detection_amd import hip_api, unet

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


@pytest.fixture(scope="module")
def modules():
    pos, shp = unet.PosNet(), unet.ShapeNet()
    pos.load_state_dict(recipe_state_dict(pos, 1))
    shp.load_state_dict(recipe_state_dict(shp, 2))
    return pos.eval(), shp.eval()


def make_nets(modules, **kw):
    return unet.ScoreMapNets(copy.deepcopy(modules[0]), copy.deepcopy(modules[1]), device=0, div_clf=(-10.8, -2.1), **kw)


@pytest.fixture(scope="module")
def image():
    return np.random.default_rng(5).random((700, 900, 3), dtype=np.float32)


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


# ---- 1. window epilogues ---------------------------------------------------------------------------------------------
WINDOWS = [(0, 0, None, None), (0, 0, 17, 29), (0, 100, 5, 60), (None, 40, 5, 77), (50, 0, 60, 3), (70, None, 40, 1),
           (100, 123, 50, 1), (3, 5, 1, 200), (48, 64, 40, 64), (13, 7, 33, 45), (None, None, 1, 1)]


def resolve(win, H, W):
    wx0, wy0, h, w = win
    h = H if h is None else min(h, H - (wx0 or 0))
    w = W if w is None else min(w, W - (wy0 or 0))
    return (H - h if wx0 is None else wx0), (W - w if wy0 is None else wy0), h, w


@pytest.mark.parametrize("H,W", [(203, 331), (96, 128)])
def test_window_epilogues_equal_the_full_crop_epilogue_bit_for_bit(modules, H, W):
    nets = make_nets(modules)
    ctx = nets.ctx
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(H)
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    pos_out = torch.randn((3, Hp, Wp), generator=g).cuda()
    logits = (3.0 * torch.randn((32, Hp, Wp), generator=g)).cuda()
    hid = torch.relu(torch.randn((1, 32, Hp, Wp), generator=g)).cuda().contiguous(memory_format=torch.channels_last)
    wh, bh = nets._packed_heads()
    # full-crop references
    ref = {}
    d = torch.empty((H, W), device="cuda"); m = torch.empty((H, W, 32), device="cuda")
    ctx.posnet_epilogue(pos_out, H, W, -10.8, -2.1, d); ctx.shapenet_epilogue(logits, H, W, m)
    ref["planar"] = (d, [m])
    for dt in (torch.float32, torch.bfloat16):
        po = pos_out.to(dt).unsqueeze(0).contiguous(memory_format=torch.channels_last)
        lg = logits.to(dt).unsqueeze(0).contiguous(memory_format=torch.channels_last)
        d = torch.empty((H, W), device="cuda"); m = torch.empty((H, W, 32), device="cuda")
        ctx.posnet_epilogue_nhwc(po, H, W, -10.8, -2.1, d); ctx.shapenet_epilogue_nhwc(lg, H, W, m)
        ref[dt] = (d, [m], po, lg)
    hm = [torch.empty((H, W, 32), device="cuda") for _ in range(3)]
    ctx.shapenet_heads(hid, wh, bh, H, W, hm)
    for win in WINDOWS:
        if (win[0] or 0) >= H or (win[1] or 0) >= W:
            continue
        wx0, wy0, h, w = resolve(win, H, W)
        ox, oy = 8, 4 if wy0 % 4 == 0 else 5           # (a 16-byte aligned det row where the window allows float4 stores)
        big = (H + 20, W + 24)

        def dest(ch):
            t = torch.full(big + ((ch,) if ch > 1 else ()), SENTINEL, device="cuda")
            return t, t[ox:ox + h, oy:oy + w]

        def check(full, t, what):
            torch.cuda.synchronize()
            assert torch.equal(bits(t[ox:ox + h, oy:oy + w]), bits(full[wx0:wx0 + h, wy0:wy0 + w])), (what, win)
            t = t.clone(); t[ox:ox + h, oy:oy + w] = SENTINEL
            assert bool((t == SENTINEL).all()), (what, win, "written outside the window")

        t, v = dest(1); ctx.posnet_epilogue(pos_out, H, W, -10.8, -2.1, v, wx0=wx0, wy0=wy0); check(ref["planar"][0], t, "posnet")
        t, v = dest(32); ctx.shapenet_epilogue(logits, H, W, v, wx0=wx0, wy0=wy0); check(ref["planar"][1][0], t, "shapenet")
        for dt in (torch.float32, torch.bfloat16):
            full_d, full_m, po, lg = ref[dt]
            t, v = dest(1); ctx.posnet_epilogue_nhwc(po, H, W, -10.8, -2.1, v, wx0=wx0, wy0=wy0); check(full_d, t, f"posnet nhwc {dt}")
            t, v = dest(32); ctx.shapenet_epilogue_nhwc(lg, H, W, v, wx0=wx0, wy0=wy0); check(full_m[0], t, f"shapenet nhwc {dt}")
        dests = [dest(32) for _ in range(3)]
        ctx.shapenet_heads(hid, wh, bh, H, W, [v for _, v in dests], wx0=wx0, wy0=wy0)
        for k in range(3):
            check(hm[k], dests[k][0], f"heads {k}")
    # a window outside the crop is refused by the library, a destination that is not a window view by the binding
    t = torch.zeros((H + 1, W), device="cuda")
    with pytest.raises(hip_api.MppError, match="outside"):
        ctx.posnet_epilogue(pos_out, H, W, -10.8, -2.1, t[:H], wx0=1, wy0=0)
    with pytest.raises(ValueError):
        ctx.shapenet_epilogue(logits, H, W, torch.zeros((H, W, 16, 2), device="cuda"), wx0=0, wy0=0)


def test_the_full_shapenet_epilogue_refuses_marks_off_a_16_byte_boundary():
    """The whole-crop call runs the window kernel, whose float4 stores need aligned marks: a map 4 bytes into its storage is refused
    before any launch.  2 x 69: one full 64-pixel block (the 16-byte loads) plus a 5-pixel tail (the scalar loads)."""
    ctx = hip_api.MppContext(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    H, W = 2, 69
    logits = torch.randn((32, 8, 72), generator=torch.Generator().manual_seed(69)).cuda()
    store = torch.full((H * W * 32 + 1,), SENTINEL, device="cuda")
    marks = store[1:].view(H, W, 32)
    assert marks.is_contiguous() and marks.data_ptr() % 16 == 4
    with pytest.raises(hip_api.MppError, match="aligned"):
        ctx.shapenet_epilogue(logits, H, W, marks)
    torch.cuda.synchronize()
    assert bool((store == SENTINEL).all())


# ---- 2.-3. tiled forward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,dtype", [("fused", torch.float32), ("module", torch.float32), ("fused", torch.bfloat16),
                                        ("module", torch.bfloat16)])
def test_tiled_maps_equal_infer_region_per_core_and_the_whole_forward(modules, image, path, dtype):
    nets = make_nets(modules, dtype=dtype)
    if path == "fused":
        nets.min_fused_pixels = 0
    budget = 400 * 400
    plan = unet.chunk_plan(image.shape[:2], budget, 3)
    assert len(plan) >= 6 and len({c[0] for c, _ in plan}) >= 2 and len({c[2] for c, _ in plan}) >= 3
    det, marks = nets.infer(image, max_pixels=budget)
    torch.cuda.synchronize()
    # Each core runs the crop infer_region(core) runs, through the same code.  On the MI355X two identical forwards of one
    # crop on the fused channels-last path differ in the last bits (up to 6e-6 in float32; the module path repeats bit
    # for bit: test output below), so the bound is the tightest that holds for a repeated forward, not bitwise equality.
    # The drift is the library's channels-last convolutions': the project's own kernels on that path (csrc/mpp_conv.hip)
    # repeat bit for bit, several tiles per workgroup included (tests/test_gpu_unet_conv_float64.py).
    tol_core = 1e-5 if dtype == torch.float32 else 0.08
    worst, repeat = 0.0, 0.0
    for core, _ in plan:
        x0, x1, y0, y1 = core
        rd, rm = nets.infer_region(image, core)
        rd2, _ = nets.infer_region(image, core)
        torch.cuda.synchronize()
        repeat = max(repeat, float((rd - rd2).abs().max()))
        worst = max([worst, float((det[x0:x1, y0:y1] - rd).abs().max())] +
                    [float((marks[k][x0:x1, y0:y1] - rm[k]).abs().max()) for k in range(3)])
    print(f"{path} {dtype}: tiled core vs infer_region(core) max |diff| {worst:.3g}; repeated infer_region {repeat:.3g}")
    assert worst <= tol_core
    # against the whole-image forward: float32 within the region bound of test_gpu_multirank.  bfloat16: on this noise image
    # the whole-image bfloat16 forward itself lies up to ~0.1 from the float32 maps (above test_unet's 0.08 on its image), so
    # the tiled bfloat16 maps must stay within 0.08 of the float32 maps, or within 1.25 x the whole bfloat16 forward's error
    wd, wm = nets.infer(image)
    torch.cuda.synchronize()
    if dtype == torch.float32:
        tol = 1e-3
    else:
        rd, rm = make_nets(modules).infer(image)
        torch.cuda.synchronize()
        whole_err = max([float((wd - rd).abs().max())] + [float((a - b).abs().max()) for a, b in zip(wm, rm)])
        tiled_err = max([float((det - rd).abs().max())] + [float((a - b).abs().max()) for a, b in zip(marks, rm)])
        print(f"{path} bfloat16 vs float32: whole {whole_err:.3g}, tiled {tiled_err:.3g}")
        tol, wd, wm = max(0.08, 1.25 * whole_err), rd, rm
    assert float((det - wd).abs().max()) <= tol
    for k in range(3):
        assert float((marks[k] - wm[k]).abs().max()) <= tol
        np.testing.assert_allclose(marks[k].sum(-1).cpu().numpy(), 1.0, atol=1e-4)


def test_a_budget_over_the_image_or_a_region_runs_the_untiled_forward(modules, image):
    nets = make_nets(modules, max_forward_pixels=unet.padded_pixels(image.shape[:2], 3))
    a = nets.infer(image)
    b = make_nets(modules).infer(image)
    torch.cuda.synchronize()
    assert float((a[0] - b[0]).abs().max()) <= 1e-5 and all(float((x - y).abs().max()) <= 1e-5 for x, y in zip(a[1], b[1]))
    # a region whose crop is over the budget is built from a plan over the region: equal to the tiled whole image there
    # when the region is the whole image, and within the region bound of test_gpu_multirank otherwise
    small = make_nets(modules, max_forward_pixels=300 * 300)
    region = (100, 520, 200, 880)
    rd, rm = small.infer_region(image, region)
    td, tm = small.infer(image)
    torch.cuda.synchronize()
    assert float((rd - td[100:520, 200:880]).abs().max()) <= 1e-3
    fd, fm = small.infer_region(image, (0, 700, 0, 900))
    torch.cuda.synchronize()
    assert float((fd - td).abs().max()) <= 1e-5 and all(float((x - y).abs().max()) <= 1e-5 for x, y in zip(fm, tm))


# ---- 4. memory --------------------------------------------------------------------------------------------------------
def test_tiled_peak_memory_is_a_quarter_of_the_whole_forward(modules):
    nets = make_nets(modules)
    H = W = 2048
    img = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(3)).cuda()
    maps = H * W * unet.MAP_BYTES_PER_PIXEL
    peaks = {}
    for name, budget in (("whole", None), ("tiled", 640 * 640), ("whole2", None)):
        nets.infer(img, max_pixels=budget)        # warm-up: kernels, algorithms, the allocator's pools
        torch.cuda.synchronize()
        nets._keep = None
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = nets.infer(img, max_pixels=budget)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base - maps
        del out
        nets._keep = None
    ratio = peaks["tiled"] / peaks["whole"]
    print(f"peak minus maps: whole {peaks['whole'] / 2**20:.0f} MiB, tiled (640^2) {peaks['tiled'] / 2**20:.0f} MiB, ratio {ratio:.3f}")
    assert ratio <= 0.25


# ---- 5. out-of-memory fallback ---------------------------------------------------------------------------------------
def test_an_out_of_memory_whole_forward_falls_back_to_crops(modules, image, monkeypatch, caplog):
    nets = make_nets(modules)
    H, W = image.shape[:2]
    budget = 300 * 300
    free = int((budget + 0.5) * unet.FORWARD_BYTES_PER_PIXEL / 0.8) + unet.MAP_BYTES_PER_PIXEL * H * W
    expect_d, expect_m = nets.infer(image, max_pixels=budget)
    torch.cuda.synchronize()
    real, calls = nets._forward, []

    def forward(img, win=None):
        calls.append(win is None)
        if win is None:
            raise torch.cuda.OutOfMemoryError("simulated")
        return real(img, win)

    monkeypatch.setattr(nets, "_forward", forward)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (free, 2 * free))
    with caplog.at_level(logging.WARNING):
        det, marks = nets.infer(image)
    torch.cuda.synchronize()
    n = len(unet.chunk_plan((H, W), budget, 3))
    assert calls[0] and not any(calls[1:]) and len(calls) == 1 + n
    assert any(f"{H} x {W}" in r.message and f"({n} crops)" in r.message for r in caplog.records), caplog.text
    assert float((det - expect_d).abs().max()) <= 1e-5 and all(float((x - y).abs().max()) <= 1e-5 for x, y in zip(marks, expect_m))


# ---- 6. end to end ----------------------------------------------------------------------------------------------------
def run_main(root, tag, extra):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py"), "-p", "infer", "-m", "mpp", "-c", str(root / "cfg_unet.json"),
                        "-d", "SYNTH", "-o", "--unet"] + extra, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = root / "data" / "inference" / "SYNTH" / "val" / "mpp_hrcM"
    files = {os.path.relpath(os.path.join(d, f), out): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(out) for f in fs}
    os.rename(out, out.parent / f"mpp_hrcM_{tag}")
    return files


def test_main_with_a_forward_budget(synthetic_dataset, modules):  # noqa: F811
    root, _ = synthetic_dataset
    write_image(root, "val", 8, 23)
    for kind, name, net in (("posnet", "posvec_dota", modules[0]), ("shapenet", "shape_dota", modules[1])):
        d = root / "models_storage" / kind / name
        os.makedirs(d, exist_ok=True)
        torch.save(net.state_dict(), d / "model.pt")
    cfg = json.load(open(root / "model_configs" / "mpp" / "mpp_hrcM.json"))
    cfg["inference"]["rjmcmc_params"]["burn_in"] = 2000
    with open(root / "cfg_unet.json", "w") as f:
        json.dump(cfg, f)
    plain = run_main(root, "plain", [])
    same = run_main(root, "same", ["--unet-max-pixels", str(unet.padded_pixels((300, 420), 3))])
    assert sorted(plain) == sorted(same) and any(f.endswith("_results.pkl") for f in plain)
    for f in plain:
        assert plain[f] == same[f], f"{f} differs with a budget at least the image size"
    tiled = run_main(root, "tiled", ["--unet-max-pixels", str(200 * 200)])
    assert sorted(tiled) == sorted(plain)
    # in process: the maps MPPModel samples on under a budget are the tiled ScoreMapNets.infer maps
    from matplotlib import pyplot as plt
    from mpp_cnn_rs_object_detection_amd import mappings
    from mpp_cnn_rs_object_detection_amd.custom_types import ImageWMaps
    from mpp_cnn_rs_object_detection_amd.mpp_model import MPPModel
    from mpp_cnn_rs_object_detection_amd.shapes import Rectangle
    img = plt.imread(root / "data" / "SYNTH" / "val" / "images" / "0008.png")[:, :, :3]
    nets = make_nets(modules, max_forward_pixels=200 * 200)
    cwd = os.getcwd()
    os.chdir(REPO)
    try:
        model = MPPModel(cfg, phase="val", load=True, nets=nets)
    finally:
        os.chdir(cwd)
    data = ImageWMaps(name="0008", shape=img.shape[:2], image=img, detection_map=None, param_dist_maps=None,
                      mappings=mappings.default_mappings(), param_names=Rectangle.PARAMETERS, gt_config=[])
    region = model.region_maps(data)
    assert tuple(region.crop_data["tl_anchor"]) == (0, 0) and tuple(region.shape) == img.shape[:2]
    td, tm = nets.infer(img)
    torch.cuda.synchronize()
    assert float((region.detection_map - td).abs().max()) <= 1e-5
    assert all(float((x - y).abs().max()) <= 1e-5 for x, y in zip(region.param_dist_maps, tm))
