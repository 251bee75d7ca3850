"""Histogram matching in the batch builder and PosNet's error-density resampling on the GPU: mpp_train_batch with
MPP_AUG_HISTMATCH against the NumPy statement of skimage's match_histograms, mpp_posnet_error_map against its float64 formula
(whole and in windows), mpp_density_prefix / mpp_density_anchors against np.cumsum / np.searchsorted on the same Philox words,
and train_unet through an error update."""
import json
import logging
import os

import numpy as np
import pytest

from mpp_cnn_rs_object_detection_amd import hip_api, shapes, synth, unet
from mpp_cnn_rs_object_detection_amd import unet_training as ut
from test_gpu_unet_training import POS_CFG, SHP_CFG, tiny_config, write_dataset
from test_unet_resampling_host import match_lut

pytestmark = pytest.mark.gpu
HM = hip_api.AUG_HISTMATCH


@pytest.fixture(scope="module")
def mctx():
    import torch
    c = hip_api.MppContext(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def npy(t):
    return t.cpu().numpy()


def desc_of(rows):
    import torch
    return torch.tensor(np.asarray(rows, dtype=np.int32).reshape(-1, 3), device="cuda")


def scene(shape, n, seed):
    img, xy, marks = synth.make_scene_image(shape, n, seed=seed)
    params = np.stack(shapes.sra_to_wla(marks[:, 0], marks[:, 1], marks[:, 2]), 1)
    return (img * 255).astype(np.uint8), xy.astype(np.int64), params


def crop(img, ar, ac, P):
    """the zero-padded P x P read at anchor - P/2 (uint8)"""
    out = np.zeros((P, P, 3), np.uint8)
    r0, c0 = ar - P // 2, ac - P // 2
    ra, rb, ca, cb = max(0, r0), min(img.shape[0], r0 + P), max(0, c0), min(img.shape[1], c0 + P)
    if rb > ra and cb > ca:
        out[ra - r0:rb - r0, ca - c0:cb - c0] = img[ra:rb, ca:cb]
    return out


def hist_draws(seed, epoch, batch, patch, n_images):
    """the three draws of a patch: Philox stream 0, index 5 -> (apply, template, blend)"""
    w = hip_api.philox([batch, patch, 0, 5], [seed, epoch]).astype(np.float64)
    u = (w + 0.5) / 4294967296.0
    return bool(u[0] < 0.5), min(n_images - 1, int(u[1] * n_images)), 0.1 + u[2] * 0.65


def hist_images():
    imgs = [scene((96, 96), 40, 1)[0], scene((80, 120), 50, 2)[0], scene((64, 64), 20, 3)[0]]
    one = np.empty((40, 56, 3), np.uint8)
    one[:] = (50, 100, 200)                                           # a one-colour template
    rng = np.random.default_rng(9)
    imgs += [one, rng.integers(0, 256, size=(70, 50, 3), dtype=np.uint8)]
    return imgs


def test_image_histograms_equal_bincount(mctx):
    imgs = hist_images() + [np.random.default_rng(4).integers(0, 256, size=(300, 500, 3), dtype=np.uint8)]   # > one slice
    data = ut.ResidentSubset.from_arrays(imgs, [np.zeros((0, 2))] * len(imgs), [np.zeros((0, 3))] * len(imgs), 0)
    got = npy(data.histograms(mctx))
    for i, im in enumerate(imgs):
        for ch in range(3):
            assert np.array_equal(got[i, ch], np.bincount(im[..., ch].ravel(), minlength=256)), (i, ch)


def test_histogram_matching_equals_the_numpy_statement(mctx):
    imgs = hist_images()
    n = len(imgs)
    data = ut.ResidentSubset.from_arrays(imgs, [np.zeros((0, 2))] * n, [np.zeros((0, 3))] * n, 0)
    counts = [[np.bincount(im[..., ch].ravel(), minlength=256) for ch in range(3)] for im in imgs]
    P, B, seed, epoch = 32, 1024, 11, 3
    rng = np.random.default_rng(6)
    builder = ut.BatchBuilder(mctx, ut.labels_struct(POS_CFG, "posnet"), P, 0)
    applied, templates, worst = 0, np.zeros(n, np.int64), 0.0
    total = 0
    for batch in range(4):                                           # 4096 patches
        rows = []
        for b in range(B):
            i = int(rng.integers(0, n))
            H, W = imgs[i].shape[:2]
            # anchors anywhere in [0, shape]: many crops hang over the border; the first few sit on the corners
            rows.append((i, int(rng.integers(0, H + 1)), int(rng.integers(0, W + 1))))
        rows[0], rows[1], rows[2] = (0, 0, 0), (1, 80, 120), (3, 20, 28)
        desc = desc_of(rows)
        plain = npy(builder.build(data, desc, 0, seed, epoch, batch, fresh=True)["patch"])
        got = npy(builder.build(data, desc, HM, seed, epoch, batch, fresh=True)["patch"])
        for b, (i, ar, ac) in enumerate(rows):
            apply, tmpl, blend = hist_draws(seed, epoch, batch, b, n)
            total += 1
            if not apply:
                assert np.array_equal(got[b], plain[b]), (batch, b)
                continue
            assert 0.1 <= blend <= 0.75
            applied += 1
            templates[tmpl] += 1
            s = crop(imgs[i], ar, ac, P)
            assert np.array_equal(plain[b], (s.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
            for ch in range(3):
                lut = match_lut(s[..., ch], counts[tmpl][ch])
                want = np.clip(blend * lut[s[..., ch]] + (1 - blend) * s[..., ch], 0, 255) / 255
                err = float(np.max(np.abs(got[b, ch].astype(np.float64) - want)))
                worst = max(worst, err)
                # the LUT, the blend and the division: one float32 rounding each of a value <= 1 (2.4e-7 together)
                assert err <= 1e-6, (batch, b, ch, err)
    print(f"histogram matching: {applied} of {total} applied, templates {templates.tolist()}, worst error {worst:.3g}")
    assert total >= 4096
    assert abs(applied / total - 0.5) < 4 * np.sqrt(0.25 / total)
    for k in range(n):
        p = 1 / n
        assert abs(templates[k] / applied - p) < 4 * np.sqrt(p * (1 - p) / applied), (k, templates)
    # a one-colour template maps every value to that colour
    lut = match_lut(imgs[0][..., 0], counts[3][0])
    assert np.all(lut == 50)


@pytest.mark.parametrize("kind", ["posnet", "shapenet"])
def test_histogram_matching_moves_no_other_draw(mctx, kind):
    sc = [scene((128, 128), 80, 5), scene((96, 160), 70, 6)]
    data = ut.ResidentSubset.from_arrays([s[0] for s in sc], [s[1] for s in sc], [s[2] for s in sc], 0)
    P, B, seed, epoch, batch = 64, 96, 21, 1, 2
    rng = np.random.default_rng(8)
    rows = [(i, int(rng.integers(0, sc[i][0].shape[0] + 1)), int(rng.integers(0, sc[i][0].shape[1] + 1)))
            for i in rng.integers(0, 2, size=B)]
    flags = hip_api.AUG_GEOMETRIC | hip_api.AUG_STRONG | (hip_api.AUG_PERTURB if kind == "shapenet" else 0)
    builder = ut.BatchBuilder(mctx, ut.labels_struct(POS_CFG if kind == "posnet" else SHP_CFG, kind), P, 0)
    a = {k: npy(v) for k, v in builder.build(data, desc_of(rows), flags, seed, epoch, batch, fresh=True).items()}
    b = {k: npy(v) for k, v in builder.build(data, desc_of(rows), flags | HM, seed, epoch, batch, fresh=True).items()}
    for k in a:
        if k != "patch":
            assert np.array_equal(a[k], b[k]), k
    n_applied = 0
    for p in range(B):
        apply = hist_draws(seed, epoch, batch, p, 2)[0]
        n_applied += apply
        if not apply:
            assert np.array_equal(a["patch"][p], b["patch"][p]), p
    assert 0 < n_applied < B and not np.array_equal(a["patch"], b["patch"])


def test_histogram_flag_without_a_table_is_an_error(mctx):
    import torch
    img = scene((64, 64), 10, 1)
    data = ut.ResidentSubset.from_arrays([img[0]], [img[1]], [img[2]], 0)
    builder = ut.BatchBuilder(mctx, ut.labels_struct(POS_CFG, "posnet"), 32, 0)
    out = dict(builder.buffers(2))
    out["status"] = builder.status
    mctx.train_set_histograms(None)
    with pytest.raises(hip_api.MppError, match="HISTMATCH"):
        mctx.train_batch(data.struct, builder.labels, desc_of([(0, 10, 10), (0, 30, 30)]), 32, HM, 1, 0, 0, out)
    # a table of another subset's size is refused as well
    mctx.train_set_histograms(torch.zeros((3, 3, 256), dtype=torch.int32, device="cuda"))
    with pytest.raises(hip_api.MppError, match="HISTMATCH"):
        mctx.train_batch(data.struct, builder.labels, desc_of([(0, 10, 10), (0, 30, 30)]), 32, HM, 1, 0, 0, out)
    mctx.train_set_histograms(None)


# ---- error densities -------------------------------------------------------------------------------------------------------
def error_case(H, W, n, seed, saturate=None):
    rng = np.random.default_rng(seed)
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    out = rng.normal(0, 3, size=(3, Hp, Wp)).astype(np.float32)
    if saturate is not None:
        out[2] = saturate
    # (a crowd of more than 1024 objects keeps to one quarter of the image, so that both target values occur)
    hi = (H // 2, W // 2) if n > 1024 else (H, W)
    centers = np.stack([rng.integers(0, hi[0], size=n), rng.integers(0, hi[1], size=n)], 1).astype(np.int32).reshape(-1, 2)
    return out, centers


def cell_formula(out, centers, H, W, md):
    """target, err and the block means in float64"""
    rr, cc = np.mgrid[:H, :W]
    target = np.zeros((H, W))
    if len(centers):
        best = np.full((H, W), np.iinfo(np.int64).max)
        for k in range(0, len(centers), 64):
            c = centers[k:k + 64].astype(np.int64)
            d2 = (c[:, 0][:, None, None] - rr) ** 2 + (c[:, 1][:, None, None] - cc) ** 2
            best = np.minimum(best, d2.min(0))
        target = (~(np.sqrt(best.astype(np.float64)) + 1e-8 > md)).astype(np.float64)
    err = np.abs(target - 1 / (1 + np.exp(-out[2, :H, :W].astype(np.float64))))
    ch, cw = -(-H // 8), -(-W // 8)
    pad = np.full((ch * 8, cw * 8), np.nan)
    pad[:H, :W] = err
    return np.nanmean(pad.reshape(ch, 8, cw, 8), axis=(1, 3)), target


ERROR_CASES = [(100, 130, 60, 1, None), (64, 64, 0, 2, None), (203, 77, 1500, 3, None), (256, 256, 230, 4, None),
               (50, 90, 0, 5, 40.0), (61, 43, 30, 6, -40.0)]


@pytest.mark.parametrize("H,W,n,seed,saturate", ERROR_CASES)
def test_error_map_equals_the_formula_whole_and_in_windows(mctx, H, W, n, seed, saturate):
    import torch
    md = 8.0
    out_h, centers = error_case(H, W, n, seed, saturate)
    want, target = cell_formula(out_h, centers, H, W, md)
    out = torch.from_numpy(out_h).cuda()
    cen = torch.from_numpy(centers).cuda() if n else None
    ch, cw = -(-H // 8), -(-W // 8)
    dens = torch.full((ch, cw), 77, dtype=torch.uint8, device="cuda")
    cell = torch.full((ch, cw), -1, dtype=torch.float32, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    mctx.posnet_error_map(out, (H, W), cen, md, dens, total, cell=cell)
    cell_h, dens_h = npy(cell), npy(dens)
    err = float(np.max(np.abs(cell_h.astype(np.float64) - want)))
    print(f"error map {H}x{W}, {n} objects: max |cell - formula| = {err:.3g}, target share {target.mean():.3f}, sum {int(total)}")
    assert err <= 1e-6                                                   # (a)
    assert cell_h.min() >= 0 and cell_h.max() <= 1
    assert np.array_equal(dens_h, np.minimum(255, np.floor(np.float32(256) * cell_h)).astype(np.uint8))   # (b)
    assert int(total) == int(dens_h.astype(np.int64).sum())              # (c)
    if n:
        assert 0 < target.mean() < 1
    if saturate == 40.0:
        assert (dens_h == 255).all()                                     # err = 1 everywhere: 256 caps at 255
    # (d) the window form over a chunk plan of the same output
    plan = unet.chunk_plan((H, W), 48 * 48, 3, halo=8)                   # (a short halo, so that the small cases split too)
    assert len(plan) > 1
    dens_w = torch.full((ch, cw), 77, dtype=torch.uint8, device="cuda")
    total_w = torch.zeros(1, dtype=torch.int64, device="cuda")
    for core, (cx0, cx1, cy0, cy1) in plan:
        sub = out[:, cx0:-(-cx1 // 8) * 8, cy0:-(-cy1 // 8) * 8].contiguous()
        mctx.posnet_error_map(sub, (H, W), cen, md, dens_w, total_w, crop=(cx0, cy0), core=core)
    assert np.array_equal(npy(dens_w), dens_h)
    assert int(total_w) == int(total)


def test_error_map_refuses_cores_off_the_cell_grid(mctx):
    import torch
    out = torch.zeros((3, 64, 64), device="cuda")
    dens = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    for core in ((4, 64, 0, 64), (0, 60, 0, 64), (0, 64, 0, 72)):
        with pytest.raises(hip_api.MppError):
            mctx.posnet_error_map(out, (64, 64), None, 8.0, dens, total, core=core)
    with pytest.raises(hip_api.MppError):                                # the core must lie inside the crop's output
        mctx.posnet_error_map(out, (128, 128), None, 8.0, torch.zeros((16, 16), dtype=torch.uint8, device="cuda"), total,
                              crop=(0, 0), core=(64, 128, 0, 64))


# ---- anchors ---------------------------------------------------------------------------------------------------------------
def test_density_anchors_equal_searchsorted_on_the_same_words(mctx):
    import torch
    shapes_ = [(37, 50), (64, 64), (16, 2400), (2100, 8), (24, 24)]
    rng = np.random.default_rng(12)
    maps = []
    for H, W in shapes_:
        ch, cw = -(-H // 8), -(-W // 8)
        m = rng.integers(0, 256, size=(ch, cw)).astype(np.uint8)
        m[rng.random((ch, cw)) < 0.5] = 0                                # zero cells
        m[::3] = 0                                                       # zero rows
        m[-1, -1] = 200                                                  # the last (partial) cell can be drawn
        maps.append(m)
    maps[4][:] = 0                                                       # an image without density
    imgs = [np.zeros((H, W, 3), np.uint8) for H, W in shapes_]
    data = ut.ResidentSubset.from_arrays(imgs, [np.zeros((0, 2))] * 5, [np.zeros((0, 3))] * 5, 0)
    ed = ut.ErrorDensities(data, mctx, 8.0)
    for i, m in enumerate(maps):
        ed.map(i).copy_(torch.from_numpy(m))
        ed.totals[i] = int(m.astype(np.int64).sum())
    ed.finish()
    assert np.array_equal(ed.sums, [int(m.astype(np.int64).sum()) for m in maps])
    cellcum, rowcum = npy(ed.cellcum).view(np.uint32), npy(ed.rowcum)
    for i, m in enumerate(maps):
        a, b = ed.cell_off_host[i], ed.cell_off_host[i + 1]
        assert np.array_equal(cellcum[a:b].reshape(m.shape), np.cumsum(m.astype(np.uint32), axis=1))
        assert np.array_equal(rowcum[ed.row_off_host[i]:ed.row_off_host[i + 1]], np.cumsum(m.astype(np.int64).sum(1)))
    n, seed, epoch = 4000, ut.SEED, 16
    rows = np.stack([rng.integers(0, 5, size=n), np.arange(n) * 7 + 3], 1).astype(np.int32)
    got = ed.anchors(rows, seed, epoch)
    assert np.array_equal(got, ed.anchors(rows, seed, epoch))
    assert not np.array_equal(got, ed.anchors(rows, seed, epoch + 1))
    for i, m in enumerate(maps):
        sel = rows[:, 0] == i
        assert sel.sum() > 100
        if i == 4:
            assert (got[sel] == -1).all()
            continue
        want = ut.density_anchors_host(m, shapes_[i], ut.density_words(rows[sel, 1], seed, epoch))
        assert np.array_equal(got[sel], want), i
        assert (m[got[sel, 0] // 8, got[sel, 1] // 8] > 0).all()         # no anchor in a zero cell
        assert (got[sel] >= 0).all() and (got[sel, 0] <= shapes_[i][0]).all() and (got[sel, 1] <= shapes_[i][1]).all()
    sel = rows[:, 0] == 0                                                # the partial last cell is reached
    assert ((got[sel, 0] // 8 == 4) & (got[sel, 1] // 8 == 6)).any()


# ---- the trainer -----------------------------------------------------------------------------------------------------------
def test_plan_draws_half_of_its_anchors_near_objects_when_the_net_predicts_no_mask(mctx):
    import torch
    md = 8.0
    sc = [scene((256, 256), 230, 0), scene((200, 184), 120, 1)]
    noise = np.random.default_rng(2).integers(0, 256, size=(96, 128, 3), dtype=np.uint8)
    data = ut.ResidentSubset.from_arrays([s[0] for s in sc] + [noise], [s[1] for s in sc] + [np.zeros((0, 2))],
                                         [s[2] for s in sc] + [np.zeros((0, 3))], 0)
    torch.manual_seed(0)
    net = unet.PosNet(hidden_dims=(8, 16)).cuda()
    with torch.no_grad():                                                # sigmoid(out[2]) = 0 everywhere
        net.final_layer.weight[2].zero_()
        net.final_layer.bias[2] = -200.0
    ed = ut.ErrorDensities(data, mctx, md)
    ed.update(net)
    whole = npy(ed.dens).copy()
    for i in range(2):                                                   # the density is the target mask
        H, W = sc[i][0].shape[:2]
        _, target = cell_formula(np.zeros((3, H, W), np.float32), sc[i][1], H, W, md)
        pad = np.full((-(-H // 8) * 8, -(-W // 8) * 8), np.nan)
        pad[:H, :W] = target
        mean = np.nanmean(pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8), axis=(1, 3)).astype(np.float32)
        assert np.array_equal(npy(ed.map(i)), np.minimum(255, np.floor(np.float32(256) * mean)).astype(np.uint8))
    assert ed.sums[0] > 0 and ed.sums[1] > 0 and ed.sums[2] == 0
    ed.update(net, max_pixels=128 * 128)                                 # the same maps from crops
    assert np.array_equal(npy(ed.dens), whole)
    pm = {"n_patches": 4096, "unf_sampler_weight": 0.33, "obj_sampler_weight": 0.66, "obj_sampler_sigma": 10}
    plan, which = ut.make_plan(np.random.default_rng(5), data, 4096, pm, ed, epoch=2, return_samplers=True)
    n = len(plan)
    assert n == 4096 and abs(np.mean(which == 2) - 0.5) < 4 * np.sqrt(0.25 / n)
    checked = 0
    for (i, ar, ac), w in zip(plan, which):
        H, W = data.shapes[i]
        assert 0 <= ar <= H and 0 <= ac <= W
        if w != 2 or i == 2:
            continue
        assert ar % 8 == 0 and ac % 8 == 0
        rr, cc = np.mgrid[ar:min(ar + 8, H), ac:min(ac + 8, W)]
        c = sc[i][1]
        d2 = (c[:, 0][:, None, None] - rr) ** 2 + (c[:, 1][:, None, None] - cc) ** 2
        assert np.sqrt(d2.min()) <= md, (i, ar, ac)
        checked += 1
    assert checked > 1000


def test_training_runs_through_an_error_update(tmp_path, monkeypatch, caplog):
    from PIL import Image
    write_dataset(tmp_path)
    monkeypatch.chdir(tmp_path)
    cfg = tiny_config("posnet", n_epochs=4, n_patches=256)
    cfg["data_loader"].update(dataset_update_interval=1, error_update_interval=2)
    with caplog.at_level(logging.WARNING):
        d = ut.train_unet(cfg, "posnet", dataset="SYNTH", model_base=str(tmp_path / "models_storage"))
    log = json.load(open(os.path.join(d, "log.json")))
    assert log["epoch"] == [0, 1, 2, 3] and np.isfinite(log["train_loss"]).all() and os.path.exists(os.path.join(d, "model.pt"))
    maps = tmp_path / "data" / "error_maps" / "SYNTH" / "train" / cfg["model_name"]
    assert sorted(os.listdir(maps)) == ["0000.png", "0001.png", "0002.png"]
    for f in os.listdir(maps):
        with Image.open(maps / f) as im:
            assert im.mode == "L" and im.size == (32, 32)
            assert np.asarray(im).max() > 0
    warned = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]
    assert warned and all("figure_interval" in m for m in warned), warned
    assert not any("error_update_interval" in m or "hist_match" in m for m in warned)
