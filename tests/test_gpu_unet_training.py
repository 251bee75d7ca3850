"""U-Net training on the GPU: the batch builder (mpp_train_batch) against numpy crops and the reference's recorded labels,
the augmentation's D4 / key / perturbation contracts, the fused losses (mpp_posnet_loss, mpp_shapenet_loss) against the
reference's recorded losses and gradients, and ``main.py -p train -m posnet|shapenet`` end to end."""
import glob
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN, REPO
import unet_train_cases as cases
from mpp_cnn_rs_object_detection_amd import hip_api, shapes, synth, unet
from mpp_cnn_rs_object_detection_amd import unet_training as ut

pytestmark = pytest.mark.gpu
POS_CFG = {"loss": {"target_mode": "uvec", "max_distance": 8, "bin_map_dil": 0.6}}
SHP_CFG = {"trainer": {"n_classes": 32}, "mappings": {"size_mapping_min": 0, "size_mapping_max": 32}}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "unet_train_golden.npz"))


@pytest.fixture(scope="module")
def mctx():
    import torch
    c = hip_api.MppContext(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def builder(mctx, kind, P, with_dist=True):
    lab = ut.labels_struct(POS_CFG if kind == "posnet" else SHP_CFG, kind)
    return ut.BatchBuilder(mctx, lab, P, 0, with_dist=with_dist)


def desc_of(rows):
    import torch
    return torch.tensor(np.asarray(rows, dtype=np.int32).reshape(-1, 3), device="cuda")


def npy(t):
    return t.cpu().numpy()


def test_patches_equal_a_zero_padded_crop():
    import torch
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, size=(100, 130, 3), dtype=np.uint8), rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)]
    data = ut.ResidentSubset.from_arrays(imgs, [np.zeros((0, 2))] * 2, [np.zeros((0, 3))] * 2, 0)
    c = hip_api.MppContext(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    P = 48
    rows = [(0, 50, 60), (0, 0, 0), (0, 100, 130), (0, 3, 129), (1, 32, 32), (1, 64, 0), (0, 99, 5)]
    out = builder(c, "posnet", P).build(data, desc_of(rows), 0, 1, 0, 0)
    got = npy(out["patch"])
    for b, (i, ar, ac) in enumerate(rows):
        img = imgs[i].astype(np.float32) / np.float32(255)
        want = np.zeros((P, P, 3), np.float32)
        for r in range(P):
            for cc in range(P):
                gr, gc = ar - P // 2 + r, ac - P // 2 + cc
                if 0 <= gr < img.shape[0] and 0 <= gc < img.shape[1]:
                    want[r, cc] = img[gr, gc]
        assert np.array_equal(got[b], want.transpose(2, 0, 1)), b
    c.close()


def label_batch(mctx, kind, flags=0, seed=1, patches=None, images=None):
    P = cases.LABEL_P
    patches = patches or cases.label_patches()
    rng = np.random.default_rng(5)
    images = images or [rng.integers(0, 256, size=(P, P, 3), dtype=np.uint8) for _ in patches]
    data = ut.ResidentSubset.from_arrays(images, [c for c, _ in patches], [p for _, p in patches], 0)
    rows = [(i, P // 2, P // 2) for i in range(len(patches))]
    out = builder(mctx, kind, P).build(data, desc_of(rows), flags, seed, 0, 0, fresh=True)
    return {k: npy(v) for k, v in out.items()}, images


def test_distance_and_dilated_map_equal_the_fixture(mctx, golden):
    out, _ = label_batch(mctx, "posnet")
    for i in range(3):
        np.testing.assert_allclose(out["dist"][i], golden[f"shape{i}_distance"], rtol=1e-6, atol=0)
        np.testing.assert_allclose(out["dil"][i], golden[f"shape{i}_dil"], rtol=0, atol=1e-6)
    # the empty patch: scipy measures from a virtual point, its dilated map has a blob in the top-left corner
    assert out["dil"][2][0, 0] > 0 and out["mask"][2].sum() == 0 and not out["vec"][2].any()


def test_pointing_vectors_land_on_the_nearest_centre(mctx):
    out, _ = label_batch(mctx, "posnet")
    P = cases.LABEL_P
    for i, (c, _) in enumerate(cases.label_patches()[:2]):
        rr, cc = np.mgrid[:P, :P]
        d2 = (c[:, 0][:, None, None] - rr) ** 2 + (c[:, 1][:, None, None] - cc) ** 2
        dmin = np.sqrt(d2.min(0))
        unique = (d2 == d2.min(0)).sum(0) == 1
        m = out["mask"][i] > 0
        assert np.array_equal(m, dmin + 1e-8 <= 8)
        v = out["vec"][i].transpose(1, 2, 0).astype(np.float64)
        land = np.stack([rr, cc], -1) + v * dmin[..., None]
        for r, q in zip(*np.nonzero(m)):
            hit = np.abs(c - land[r, q]).sum(1)
            k = int(np.argmin(hit))
            assert hit[k] < 1e-4 and abs(np.sqrt(d2[k, r, q]) - dmin[r, q]) < 1e-9
            if unique[r, q]:
                assert k == int(np.argmin(d2[:, r, q]))
        assert not out["vec"][i][:, ~m].any()


def test_shapenet_labels_equal_the_fixture(mctx, golden):
    out, _ = label_batch(mctx, "shapenet")
    for i in range(3):
        assert np.array_equal(out["cls"][:, i], golden[f"shape{i}_cls"]), i
        cov = out["cover"][i].astype(bool)
        lm = np.zeros(cov.shape) if cov.sum() == 0 else cov / np.sum(cov)
        assert np.array_equal(lm, golden[f"shape{i}_loss_mask"]), i
        assert out["sums"][i, :, 0].sum() == cov.sum()


@pytest.mark.parametrize("kind", ["posnet", "shapenet"])
def test_geometric_augmentation_is_the_d4_image_of_the_batch(mctx, kind):
    P = cases.LABEL_P
    patches = cases.label_patches()
    seen = set()
    for seed in range(6):
        aug, images = label_batch(mctx, kind, flags=hip_api.AUG_GEOMETRIC, seed=seed)
        plain, _ = label_batch(mctx, kind, images=images)
        for i, (c, p) in enumerate(patches):
            src = plain["patch"][i].transpose(1, 2, 0)
            hits = [(k, f) for k in range(4) for f in range(3)
                    if np.array_equal(ut.d4_image(src, k, f), aug["patch"][i].transpose(1, 2, 0))]
            assert hits, (seed, i)
            k, f = hits[0]
            seen.add((k, f))
            c2 = ut.d4_points(c, k, f, P).astype(np.int64).reshape(-1, 2)
            p2 = p.copy()
            if len(p2):
                p2[:, 2] = ut.d4_angle(p[:, 2], k, f)
            want, _ = label_batch(mctx, kind, patches=[(c2, p2)], images=[ut.d4_image(images[i], k, f)])
            assert np.array_equal(want["patch"][0], aug["patch"][i])
            keys = ("vec", "mask", "dil", "dist") if kind == "posnet" else ("cover",)
            for key in keys:
                assert np.array_equal(want[key][0], aug[key][i]), (key, seed, i, k, f)
            if kind == "shapenet":
                assert np.array_equal(want["cls"][:, 0], aug["cls"][:, i])
    assert len(seen) > 3


def test_the_key_decides_the_batch(mctx):
    flags = hip_api.AUG_GEOMETRIC | hip_api.AUG_STRONG | hip_api.AUG_PERTURB
    a, images = label_batch(mctx, "shapenet", flags=flags, seed=7)
    b, _ = label_batch(mctx, "shapenet", flags=flags, seed=7, images=images)
    c, _ = label_batch(mctx, "shapenet", flags=flags, seed=8, images=images)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["patch"], c["patch"])
    m = label_batch(mctx, "posnet", flags=hip_api.AUG_MEDIUM, seed=7, images=images)[0]["patch"]
    assert m.min() >= 0 and m.max() <= 1


def test_class_perturbation_frequencies(mctx):
    import torch
    P, B = 128, 1024
    g = np.arange(6, 128, 12)
    centers = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    params = np.tile([[6.0, 10.0, 1.0]], (len(centers), 1))          # classes 8, 19, 10: no clipping
    data = ut.ResidentSubset.from_arrays([np.zeros((P, P, 3), np.uint8)], [centers], [params], 0)
    b = builder(mctx, "shapenet", P)
    desc = desc_of([(0, P // 2, P // 2)] * B)
    r, c = torch.from_numpy(centers[:, 0]).cuda(), torch.from_numpy(centers[:, 1]).cuda()
    plain = b.build(data, desc, 0, 3, 0, 0, fresh=True)["cls"][:, :, r, c]
    pert = b.build(data, desc, hip_api.AUG_PERTURB, 3, 0, 0, fresh=True)["cls"][:, :, r, c]
    d = (pert.to(torch.int64) - plain.to(torch.int64)).cpu().numpy()
    assert np.array_equal(plain.cpu().numpy()[:, 0, 0], [8, 19, 10])
    n = d[0].size
    assert n >= 1e5
    for m in range(3):
        for v, p in ((0, 0.8), (1, 0.1), (-1, 0.1)):
            f = np.mean(d[m] == v)
            assert abs(f - p) < 4 * np.sqrt(p * (1 - p) / n), (m, v, f)


def rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30)


@pytest.mark.parametrize("form", ["train", "val"])
def test_posnet_loss_equals_the_reference(mctx, golden, form):
    import torch
    out, vec, mask, dil = cases.posnet_loss_inputs()
    B, P = out.shape[0], out.shape[-1]
    sums = np.zeros((B, (P + 15) // 16, 2))
    sums[:, 0, 0], sums[:, 0, 1] = mask.sum((1, 2)), dil.sum((1, 2), dtype=np.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    grad = torch.zeros(out.shape, dtype=torch.float32, device="cuda")
    w = torch.tensor([cases.DIV_W], dtype=torch.float32, device="cuda")
    bb = torch.tensor([cases.DIV_B], dtype=torch.float32, device="cuda")
    train = form == "train"
    mctx.posnet_loss(t(out), t(vec), t(mask), t(dil), t(sums), res, grad=grad, w=w if train else None, b=bb if train else None)
    r = npy(res)
    keys = ["vec_loss", "mask_loss"] + (["div_loss"] if train else [])
    for q, k in enumerate(keys):
        assert abs(r[q] - golden[f"pos_{form}_{k}"]) <= 1e-6 * abs(golden[f"pos_{form}_{k}"]), k
    assert abs(r[3] - golden[f"pos_{form}_loss"]) <= 1e-6 * golden[f"pos_{form}_loss"]
    assert rel(npy(grad), golden[f"pos_{form}_grad"]) < 1e-5
    if train:
        assert abs(r[4] - golden["pos_train_dw"]) <= 1e-5 * abs(golden["pos_train_dw"])
        assert abs(r[5] - golden["pos_train_db"]) <= 1e-5 * abs(golden["pos_train_db"])


def test_shapenet_loss_equals_the_reference(mctx, golden):
    import torch
    logits, cls, cover, _ = cases.shapenet_loss_inputs()
    B, P = cover.shape[0], cover.shape[-1]
    sums = np.zeros((B, (P + 15) // 16, 2))
    sums[:, 0, 0] = cover.sum((1, 2))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    grads = [torch.zeros(x.shape, dtype=torch.float32, device="cuda") for x in logits]
    mctx.shapenet_loss([t(x) for x in logits], t(cls.astype(np.uint8)), t(cover.astype(np.uint8)), t(sums), res, grads=grads)
    r = npy(res)
    for h in range(3):
        assert abs(r[h] - golden[f"ce_loss_feat{h}"]) <= 1e-6 * golden[f"ce_loss_feat{h}"]
        assert rel(npy(grads[h]), golden[f"ce_grad{h}"]) < 1e-5
    assert abs(r[3] - golden["ce_loss"]) <= 1e-6 * golden["ce_loss"]
    assert not npy(grads[0])[-1].any()


def torch_posnet_loss(out, vec, mask, dil, w, b):
    """the reference's formulas (pos_loss.py, torch_div.py) in plain torch"""
    import torch
    eps = 1e-5
    s = torch.sigmoid(out[:, 2])
    prod = out[:, :2] * torch.stack([s, s], 1)
    vec_loss = torch.mean(torch.square(prod - vec))
    beta = 1 - torch.sum(mask) / mask.numel()
    mask_loss = torch.mean(-beta * mask * torch.log(s + eps) - (1 - beta) * (1 - mask) * torch.log(1 - s + eps))
    div = torch.gradient(out[:, 0], dim=1)[0] + torch.gradient(out[:, 1], dim=2)[0]
    q = torch.sigmoid(w.reshape(()) * (div * s) + b.reshape(()))
    beta_d = 1 - torch.sum(dil) / dil.numel()
    div_loss = torch.mean(-beta_d * dil * torch.log(q + eps) - (1 - beta_d) * (1 - dil) * torch.log(1 - q + eps))
    return vec_loss + mask_loss + div_loss


def test_autograd_gradients_into_a_posnet_equal_plain_torch(mctx):
    import torch
    torch.manual_seed(0)
    net = unet.PosNet(hidden_dims=(8, 16)).cuda()
    conv = torch.nn.Conv2d(1, 1, 1).cuda()
    with torch.no_grad():
        conv.weight.fill_(cases.DIV_W / 10)
        conv.bias.fill_(cases.DIV_B / 10)
    P = 32
    img, xy, marks = synth.make_scene_image((96, 96), 60, seed=4)
    params = np.stack(shapes.sra_to_wla(marks[:, 0], marks[:, 1], marks[:, 2]), 1)
    data = ut.ResidentSubset.from_arrays([(img * 255).astype(np.uint8)], [xy], [params], 0)
    lab = builder(mctx, "posnet", P, with_dist=False).build(data, desc_of([(0, 30, 30), (0, 60, 50), (0, 90, 90)]), 0, 1, 0, 0)
    grads = []
    for fused in (True, False):
        net.zero_grad()
        conv.zero_grad()
        out = net(lab["patch"])
        if fused:
            loss = ut.posnet_loss(mctx, out, lab, conv)["loss"]
        else:
            loss = torch_posnet_loss(out, lab["vec"], lab["mask"], lab["dil"], conv.weight, conv.bias)
        loss.backward()
        grads.append([p.grad.detach().clone() for p in list(net.parameters()) + list(conv.parameters())])
    # relative to the largest gradient: the conv biases in front of a BatchNorm get rounding noise only (~1e-8)
    scale = max(float(b.abs().max()) for b in grads[1])
    for a, b in zip(*grads):
        assert float((a - b).abs().max()) <= 1e-4 * scale


# ---- end to end ------------------------------------------------------------------------------------------------------------
def write_dataset(root):
    from matplotlib import pyplot as plt
    for subset, ids in (("train", (0, 1, 2)), ("val", (3,))):
        base = root / "data" / "SYNTH" / subset
        for sub in ("images", "annotations", "metadata"):
            os.makedirs(base / sub, exist_ok=True)
        for k in ids:
            img, xy, marks = synth.make_scene_image((256, 256), 230, seed=k)
            plt.imsave(base / "images" / f"{k:04}.png", img)
            params = np.stack(shapes.sra_to_wla(marks[:, 0], marks[:, 1], marks[:, 2]), 1)
            with open(base / "annotations" / f"{k:04}.pkl", "wb") as f:
                pickle.dump({"centers": xy.astype(np.int64), "parameters": params,
                             "categories": np.array(["small-vehicle"] * len(xy), dtype=object),
                             "difficult": np.zeros(len(xy), dtype=np.int64)}, f)
            with open(base / "metadata" / f"{k:04}.json", "w") as f:
                json.dump({"shape": [256, 256], "n_objects": int(len(xy))}, f)
    os.makedirs(root / "models_storage", exist_ok=True)
    with open(root / "paths_config.json", "w") as f:
        json.dump({"dataset_path": ["data/"], "model_path": ["models_storage/"]}, f)


def tiny_config(kind, n_epochs=3, n_patches=256):
    with open(os.path.join(REPO, "model_configs", "posnet/config_pos.json" if kind == "posnet"
                           else "shapenet/config_shape.json")) as f:
        cfg = json.load(f)
    cfg["data_loader"].update(dataset="SYNTH", dataset_update_interval=2)
    cfg["data_loader"]["patch_maker_params"].update(n_patches=n_patches)
    cfg["trainer"].update(n_epochs=n_epochs, batch_size=32)
    return cfg


def run_main(root, args, timeout=300):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, os.path.join(REPO, "main.py")] + args, cwd=root, env=env, capture_output=True,
                       text=True, timeout=timeout)
    return r


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    root = tmp_path_factory.mktemp("unet_train")
    write_dataset(root)
    for kind in ("posnet", "shapenet"):
        path = root / f"cfg_{kind}.json"
        with open(path, "w") as f:
            json.dump(tiny_config(kind), f)
        r = run_main(root, ["-p", "train", "-m", kind, "-c", str(path), "-d", "SYNTH"])
        assert r.returncode == 0, r.stderr[-3000:]
    return root


def test_train_writes_the_reference_model_directory(trained):
    root = trained
    for kind, name, keys in (("posnet", "posvec_dota", ["train_vec_loss", "train_mask_loss", "train_div_loss", "train_loss",
                                                         "val_vec_loss", "val_mask_loss", "val_loss"]),
                             ("shapenet", "shape_dota", ["train_loss_feat0", "train_loss_feat1", "train_loss_feat2",
                                                         "train_loss", "val_loss_feat0", "val_loss_feat1", "val_loss_feat2",
                                                         "val_loss"])):
        d = root / "models_storage" / kind / name
        assert (d / "config.json").exists() and (d / "model.pt").exists()
        assert [os.path.basename(p) for p in glob.glob(str(d / "checkpoint_*.pt"))] == ["checkpoint_0000.pt"]
        log = json.load(open(d / "log.json"))
        assert set(log) == {"epoch", "timestamp", *keys} and log["epoch"] == [0, 1, 2]
        assert all(np.isfinite(log[k]).all() for k in keys)
        if kind == "posnet":
            import torch
            sd = torch.load(d / "model_div_clf.pt", weights_only=True)
            assert set(sd) == {"1.weight", "1.bias"}
            net = unet.PosNet()
            assert unet.load_torch_model(net, str(d))
            assert unet.load_div_clf(str(d)) == (float(sd["1.weight"].flatten()[0]), float(sd["1.bias"].flatten()[0]))
        with pytest.raises(FileExistsError):
            ut.train_unet(tiny_config(kind), kind, model_base=str(root / "models_storage"))


def test_resume_restarts_at_the_last_checkpoint(trained):
    import torch
    root = trained
    d = root / "models_storage" / "posnet" / "posvec_dota"
    ck = torch.load(d / "checkpoint_0000.pt", weights_only=True)
    os.remove(d / "model.pt")
    path = root / "cfg_posnet.json"
    r = run_main(root, ["-p", "train", "-m", "posnet", "-c", str(path), "-d", "SYNTH", "-r"])
    assert r.returncode == 0, r.stderr[-3000:]
    log = json.load(open(d / "log.json"))
    assert log["epoch"] == [0, 1, 2, 0, 1, 2]
    assert "[0000] Train" in r.stdout and (d / "model.pt").exists()
    # with model.pt present nothing is left to train
    r = run_main(root, ["-p", "train", "-m", "posnet", "-c", str(path), "-d", "SYNTH", "-r"])
    assert r.returncode == 0 and "Train" not in r.stdout
    assert json.load(open(d / "log.json"))["epoch"] == [0, 1, 2, 0, 1, 2]
    assert set(ck) == set(torch.load(d / "model.pt", weights_only=True))


def test_infer_runs_on_the_trained_models(trained):
    root = trained
    for kind in ("posnet", "shapenet"):
        cfg = tiny_config(kind)
        path = root / f"cfg_infer_{kind}.json"
        with open(path, "w") as f:
            json.dump(cfg, f)
        r = run_main(root, ["-p", "infer", "-m", kind, "-c", str(path), "-d", "SYNTH", "-o"])
        assert r.returncode == 0, r.stderr[-3000:]
        out = root / "data" / "inference" / "SYNTH" / "val" / cfg["model_name"] / "0003_results.pkl"
        assert out.exists()


def test_posnet_training_lowers_the_val_loss(tmp_path, monkeypatch):
    write_dataset(tmp_path)
    monkeypatch.chdir(tmp_path)
    cfg = tiny_config("posnet", n_epochs=6, n_patches=512)
    d = ut.train_unet(cfg, "posnet", dataset="SYNTH", model_base=str(tmp_path / "models_storage"))
    log = json.load(open(os.path.join(d, "log.json")))
    v = log["val_loss"]
    print("val_loss", v)
    # first MI355X run: 0.484 -> 0.088 after six epochs (0.18 of epoch 0)
    assert v[-1] < 0.5 * v[0], v
