"""The batch builder's labels and the two fused losses (csrc/mpp_train.hip) against the float64 references of
tests/unet_train_ref.py, at the smallest shapes that reach every path of the kernels: several passes of the object
compaction, objects outside the patch, the object cap, the clamps and wraps of the class perturbation, one-row and partial
bands, more than 256 partials, saturated sigmoids, empty and full targets.  tests/test_unet_train_ref_host.py pins the
references and the conditions on these inputs without a GPU."""
import numpy as np
import pytest

import unet_train_ref as R
from mpp_cnn_rs_object_detection_amd import hip_api
from mpp_cnn_rs_object_detection_amd import unet_training as ut

pytestmark = pytest.mark.gpu


def new_ctx():
    import torch
    c = hip_api.MppContext(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    return c


@pytest.fixture(scope="module")
def mctx():
    c = new_ctx()
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def npy(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def build(mctx, dataset, rows, kind, cfg, P, flags=0, seed=R.LABEL_SEED):
    """one launch on a fresh builder -> (the builder, the outputs as numpy arrays)"""
    import torch
    images, centers, params = dataset
    data = ut.ResidentSubset.from_arrays(images, centers, params, 0)
    b = ut.BatchBuilder(mctx, ut.labels_struct(cfg, kind), P, 0, with_dist=True)
    desc = torch.tensor(np.asarray(rows, dtype=np.int32).reshape(-1, 3), device="cuda")
    out = b.build(data, desc, flags, seed, 0, 0, fresh=True)
    return b, {k: npy(v) for k, v in out.items()}


# ---- labels ----------------------------------------------------------------------------------------------------------------
def check_posnet_labels(out, ref, tag):
    worst = 0.0
    for b, r in enumerate(ref):
        for key in ("vec", "mask", "dist"):
            assert np.array_equal(bits(out[key][b]), bits(r[key])), (tag, key, b)
        worst = max(worst, float(np.max(np.abs(out["dil"][b].astype(np.float64) - r["dil"]))))
        np.testing.assert_allclose(out["dil"][b], r["dil"], rtol=0, atol=1e-6)
    want = R.band_sums(out["mask"], out["dil"])
    assert np.array_equal(out["sums"][..., 0], want[..., 0])
    np.testing.assert_allclose(out["sums"][..., 1], want[..., 1], rtol=1e-12, atol=0)
    print(f"posnet labels {tag}: max |dil - reference| = {worst:.3e} (bound 1e-6)")


@pytest.mark.parametrize("variant,geometric", [("uvec8", False), ("vec5.5", False), ("md0", False), ("uvec8", True)])
def test_posnet_labels_equal_the_reference(mctx, variant, geometric):
    flags, seed = (hip_api.AUG_GEOMETRIC, R.GEO_SEED) if geometric else (0, R.LABEL_SEED)
    _, out = build(mctx, R.label_dataset(), R.LABEL_ROWS, "posnet", R.pos_config(variant), R.LABEL_P, flags, seed)
    ref = R.label_reference("posnet", variant, geometric)
    check_posnet_labels(out, ref, f"{variant} geometric={geometric}")
    # no image, no object in reach: the empty-patch rule (distances from the virtual point (-1, 0), no mask, no vector)
    P = R.LABEL_P
    rr, cc = np.mgrid[:P, :P]
    for b in (5, 6, 9):
        assert ref[b]["n"] == 0
        assert np.array_equal(out["dist"][b], np.sqrt(((rr + 1) ** 2 + cc ** 2).astype(np.float64)).astype(np.float32))
        assert not out["mask"][b].any() and not out["vec"][b].any() and out["dil"][b][0, 0] > 0
        assert not out["sums"][b, :, 0].any()
    assert not out["patch"][5].any() and not out["patch"][9].any()


@pytest.mark.parametrize("geometric", [False, True])
def test_shapenet_labels_equal_the_reference(mctx, geometric):
    flags, seed = (hip_api.AUG_GEOMETRIC, R.GEO_SEED) if geometric else (0, R.LABEL_SEED)
    _, out = build(mctx, R.label_dataset(), R.LABEL_ROWS, "shapenet", R.shape_config(), R.LABEL_P, flags, seed)
    ref = R.label_reference("shapenet", "uvec8", geometric)
    for b, r in enumerate(ref):
        assert np.array_equal(out["cover"][b], r["cover"]), b
        assert np.array_equal(out["cls"][:, b], r["cls"]), b
    assert np.array_equal(out["sums"][..., 0], R.band_sums(np.stack([r["cover"] for r in ref]))[..., 0])


@pytest.mark.parametrize("kind", ["posnet", "shapenet"])
def test_object_cap_is_reported_and_the_first_1024_objects_are_labelled(mctx, kind):
    cfg = R.pos_config("uvec8") if kind == "posnet" else R.shape_config()
    P, ref = R.CAP_P, R.cap_reference(kind)
    keys = ("vec", "mask", "dist") if kind == "posnet" else ("cls", "cover")

    def check(out, n):
        for b in range(n):
            for key in keys:
                got = out[key][:, b] if key == "cls" else out[key][b]
                assert np.array_equal(got, ref[key]), (key, b)
            if kind == "posnet":
                np.testing.assert_allclose(out["dil"][b], ref["dil"], rtol=0, atol=1e-6)

    over, out = build(mctx, R.cap_dataset(), [(0, P // 2, P // 2), (1, P // 2, P // 2)], kind, cfg, P)
    assert int(over.status.item()) == R.CAP_N
    with pytest.raises(RuntimeError, match=str(R.CAP_N)):
        over.check()
    check(out, 2)
    full, out = build(mctx, R.cap_dataset(), [(1, P // 2, P // 2)], kind, cfg, P)
    assert int(full.status.item()) == 0
    full.check()
    check(out, 1)


def test_class_perturbation_equals_the_philox_draws(mctx):
    cfg = R.shape_config(R.PERT_N, float(R.PERT_N))
    plain, pert, _ = R.perturb_reference()
    r, c = np.array(R.PERT_GRID).T
    for flags, want in ((0, plain), (hip_api.AUG_PERTURB, pert)):
        _, out = build(mctx, R.perturb_dataset(), R.perturb_rows(), "shapenet", cfg, R.PERT_P, flags, R.PERT_SEED)
        got = out["cls"][:, :, r, c].transpose(1, 2, 0)                    # [B, object, mark]
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        assert out["cover"][:, r, c].all()


# ---- the PosNet loss -------------------------------------------------------------------------------------------------------
def run_posnet_loss(ctx, case, form):
    import torch
    out, vec, mask, dil = R.posnet_loss_case(*case)
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    grad = torch.full(out.shape, float("nan"), dtype=torch.float32, device="cuda")
    train = form == "train"
    w = torch.tensor([R.DIV_W], dtype=torch.float32, device="cuda") if train else None
    b = torch.tensor([R.DIV_B], dtype=torch.float32, device="cuda") if train else None
    ctx.posnet_loss(dev(out), dev(vec), dev(mask), dev(dil), dev(R.band_sums(mask, dil)), res, grad=grad, w=w, b=b)
    return res.cpu(), grad.cpu()


def err(got, want):
    """relative error; against a reference of exactly 0 the absolute one"""
    return abs(got - want) / abs(want) if want != 0 else abs(got - want)


def check_posnet_loss(r, g, ref, train, tag):
    """r: vec, mask, div, total, dw, db; g [B,3,P,P]"""
    e_loss = max(err(float(r[q]), ref[k]) for q, k in enumerate(("vec_loss", "mask_loss", "div_loss", "loss")))
    e_w, e_b = (err(float(r[4]), ref["dw"]), err(float(r[5]), ref["db"])) if train else (0.0, 0.0)
    e_g = [float(np.max(np.abs(g[:, ch] - ref["grad"][:, ch])) / np.max(np.abs(ref["grad"][:, ch]))) for ch in range(3)]
    print(f"posnet loss {tag}: losses {e_loss:.2e} (1e-6), dw {e_w:.2e} db {e_b:.2e} (1e-5), "
          f"grad per channel {e_g[0]:.2e} {e_g[1]:.2e} {e_g[2]:.2e} (1e-5)")
    assert np.isfinite(g).all()
    for q, k in enumerate(("vec_loss", "mask_loss", "div_loss", "loss")):
        assert abs(float(r[q]) - ref[k]) <= 1e-6 * abs(ref[k]), (k, float(r[q]), ref[k])
    if train:
        for q, k in ((4, "dw"), (5, "db")):
            assert abs(float(r[q]) - ref[k]) <= (1e-5 * abs(ref[k]) if ref[k] != 0 else 1e-12), (k, float(r[q]), ref[k])
    for ch in range(3):
        assert e_g[ch] <= 1e-5, (ch, e_g[ch])


@pytest.mark.parametrize("form", ["train", "val"])
@pytest.mark.parametrize("case", R.POSNET_CASES, ids=str)
def test_posnet_loss_equals_the_mixed_reference(mctx, case, form):
    """First MI355X run, the largest error over all cases: see profiles/unet_train.md."""
    res, grad = run_posnet_loss(mctx, case, form)
    check_posnet_loss(res.numpy(), grad.numpy().astype(np.float64), R.posnet_loss_reference(*case, form), form == "train",
                      f"{case} {form}")


# ---- the ShapeNet loss -----------------------------------------------------------------------------------------------------
def run_shapenet_loss(ctx, shape, cover_kind):
    import torch
    logits, cls, cover = R.shapenet_loss_case(*shape, cover_kind)
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    grads = [torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda") for x in logits]
    ctx.shapenet_loss([dev(x) for x in logits], dev(cls), dev(cover), dev(R.band_sums(cover)), res, grads=grads)
    return res.cpu(), [g.cpu() for g in grads]


def check_shapenet_grads(grads, ref, cover, tag):
    worst = 0.0
    for h in range(3):
        want = ref["grads"][h].astype(np.float32)
        ulps = np.abs(grads[h].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        worst = max(worst, float(ulps.max()))
        assert ulps.max() <= 1.0, (tag, h, float(ulps.max()))
        assert not grads[h][np.broadcast_to(cover[:, None] == 0, grads[h].shape)].any()
    return worst


@pytest.mark.parametrize("cover_kind", R.SHAPENET_COVERS)
@pytest.mark.parametrize("shape", R.SHAPENET_SHAPES, ids=str)
def test_shapenet_loss_equals_float64(mctx, shape, cover_kind):
    res, grads = run_shapenet_loss(mctx, shape, cover_kind)
    ref = R.shapenet_loss_reference(*shape, cover_kind)
    r = res.numpy()
    want = ref["feat"] + [ref["loss"]]
    e = max(err(float(r[q]), want[q]) for q in range(4))
    for q in range(4):
        assert abs(float(r[q]) - want[q]) <= 1e-10 * abs(want[q]), (q, float(r[q]), want[q])
    ulps = check_shapenet_grads([g.numpy() for g in grads], ref, R.shapenet_loss_case(*shape, cover_kind)[2], (shape, cover_kind))
    print(f"shapenet loss {shape} {cover_kind}: losses {e:.2e} (1e-10), gradient {ulps:.2f} float32 ulp (1)")


# ---- from the builder into the losses, through autograd -------------------------------------------------------------------
def test_posnet_builder_feeds_the_loss_and_autograd_returns_its_gradients(mctx):
    import torch
    images, centers, params = R.label_dataset()
    data = ut.ResidentSubset.from_arrays(images, centers, params, 0)
    builder = ut.BatchBuilder(mctx, ut.labels_struct(R.pos_config("uvec8"), "posnet"), R.LABEL_P, 0)
    desc = torch.tensor(np.asarray(R.LABEL_ROWS, dtype=np.int32), device="cuda")
    lab = builder.build(data, desc, 0, R.LABEL_SEED, 0, 0)
    out_np = R.builder_posnet_out()
    conv = torch.nn.Conv2d(1, 1, 1).cuda()
    with torch.no_grad():
        conv.weight.fill_(R.DIV_W)
        conv.bias.fill_(R.DIV_B)
    for train in (True, False):
        out = dev(out_np).requires_grad_(True)
        conv.zero_grad()
        d = ut.posnet_loss(mctx, out, lab, conv if train else None)
        d["loss"].backward()
        ref = R.builder_posnet_reference("train" if train else "val")
        d = {k: v.detach() for k, v in d.items()}
        r = [float(d["vec_loss"]), float(d["mask_loss"]), float(d["div_loss"]) if train else 0.0, float(d["loss"]),
             float(conv.weight.grad.reshape(())) if train else 0.0, float(conv.bias.grad.reshape(())) if train else 0.0]
        check_posnet_loss(r, npy(out.grad).astype(np.float64), ref, train, f"builder batch train={train}")


def test_shapenet_builder_feeds_the_loss_and_autograd_returns_its_gradients(mctx):
    import torch
    images, centers, params = R.label_dataset()
    data = ut.ResidentSubset.from_arrays(images, centers, params, 0)
    builder = ut.BatchBuilder(mctx, ut.labels_struct(R.shape_config(), "shapenet"), R.LABEL_P, 0)
    desc = torch.tensor(np.asarray(R.LABEL_ROWS, dtype=np.int32), device="cuda")
    lab = builder.build(data, desc, 0, R.LABEL_SEED, 0, 0)
    ref_lab = R.label_reference("shapenet")
    logits_np = R.builder_logits()
    logits = [dev(x).requires_grad_(True) for x in logits_np]
    d = ut.shapenet_loss(mctx, logits, lab)
    d["loss"].backward()
    cover = np.stack([r["cover"] for r in ref_lab])
    ref = R.shapenet_loss_ref(logits_np, np.stack([r["cls"] for r in ref_lab], 1), cover)
    # the wrapper hands the float64 results on as float32: one float32 rounding of the reference
    for k, want in (("loss_feat0", ref["feat"][0]), ("loss_feat1", ref["feat"][1]), ("loss_feat2", ref["feat"][2]),
                    ("loss", ref["loss"])):
        assert abs(float(d[k].detach()) - float(np.float32(want))) <= float(np.spacing(np.float32(want))), k
    ulps = check_shapenet_grads([npy(x.grad) for x in logits], ref, cover, "builder batch")
    print(f"shapenet loss builder batch: gradient {ulps:.2f} float32 ulp (1)")


# ---- the same inputs give the same bits ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["posnet", "shapenet"])
def test_same_inputs_give_the_same_bits_across_grid_sizes_and_contexts(kind):
    import torch

    def run(c, large):
        if kind == "posnet":
            return run_posnet_loss(c, (129, 32, 1.5, None) if large else (2, 5, 1.5, None), "train")
        return run_shapenet_loss(c, (129, 32, 8) if large else (2, 17, 5), "random")

    one, two = new_ctx(), new_ctx()
    try:
        runs = [run(one, True)]
        run(one, False)
        runs.append(run(one, True))
        runs.append(run(two, True))
    finally:
        one.close()
        two.close()
    flat = [[r] + (list(g) if isinstance(g, list) else [g]) for r, g in runs]
    assert not any(torch.isnan(t).any() for t in flat[0]) and float(flat[0][0][3]) > 0
    for other in flat[1:]:
        for a, b in zip(flat[0], other):
            assert torch.equal(a, b)
