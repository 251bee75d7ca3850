"""The references of tests/unet_conv_ref.py, pinned without a GPU: they are the U-Net's own modules in float64, their bounds
hold for torch's CPU float32 operations at every shape tests/test_gpu_unet_conv_float64.py uses (so the bounds ask nothing
a correct float32 kernel cannot give), and three wrong kernels emulated on the CPU break them at every shape (so they ask
enough)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_conv_ref as R
from test_unet import recipe_state_dict
from mpp_cnn_rs_object_detection_amd import unet


class Folds:
    """ScoreMapNets' folding and packing code without a device context"""
    _folded = unet.ScoreMapNets._folded
    _folded_after_bias = unet.ScoreMapNets._folded_after_bias
    _packed = unet.ScoreMapNets._packed
    _packed_heads = unet.ScoreMapNets._packed_heads

    def __init__(self, shp=None):
        self._fold_cache, self.shp, self.mfma_conv = {}, shp, True


@pytest.fixture(scope="module")
def nets():
    pos, shp = unet.PosNet(), unet.ShapeNet()
    pos.load_state_dict(recipe_state_dict(pos, 1))
    shp.load_state_dict(recipe_state_dict(shp, 2))
    return pos.eval(), shp.eval()


def fold64(conv, bn, x1_bias=None):
    """``_folded`` / ``_folded_after_bias`` restated in float64 (modules already cast)"""
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    shift = bn.bias + (conv.bias - bn.running_mean) * scale
    if x1_bias is not None:
        w = conv.weight
        shift = shift + scale * (w[:, w.shape[1] - x1_bias.numel():].sum(dim=(2, 3)) @ x1_bias)
    return scale.detach(), shift.detach()


# ---- the references are the modules ---------------------------------------------------------------------------------------------
def test_references_equal_the_first_double_conv_in_float64(nets):
    dc32 = nets[0].backbone.descending_path[0]
    seq32 = dc32.double_conv
    f = Folds()
    s1_32, t1_32 = f._folded(seq32[0], seq32[1])
    dc = type(dc32)(3, 32)
    dc.load_state_dict(dc32.state_dict())
    dc = dc.double().eval()
    seq = dc.double_conv
    (s1, t1), (s2, t2) = fold64(seq[0], seq[1]), fold64(seq[3], seq[4])
    np.testing.assert_allclose(s1_32.detach().numpy(), s1.numpy(), rtol=1e-6)            # the float64 fold is unet.py's fold
    np.testing.assert_allclose(t1_32.detach().numpy(), t1.numpy(), rtol=1e-5, atol=1e-7)
    x = torch.rand((1, 3, 13, 21), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    with torch.no_grad():
        want = dc(x)
        # the stem kernel, then the 32 -> 32 convolution with its epilogue
        h, _ = R.stem_ref(x, seq[0].weight, s1, t1)
        got, _ = R.conv3x3_c32_ref(h, seq[3].weight, out_scale=s2, out_shift=t2)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-12)
        # the library's raw first convolution, its BatchNorm + ReLU at the second one's load
        raw = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), seq[0].weight)
        got, _ = R.conv3x3_c32_ref(raw, seq[3].weight, in_scale=s1, in_shift=t1, out_scale=s2, out_shift=t2)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-12)


def test_references_equal_an_up_block_with_its_concat_and_bias_fold(nets):
    up32 = nets[1].backbone.ascending_path[-1]                                      # Up(64, 32)
    f = Folds()
    seq32 = up32.conv.double_conv
    t1_32 = f._folded_after_bias(seq32[0], seq32[1], up32.up.bias.detach())[1]
    up = type(up32)(64, 32)
    up.load_state_dict(up32.state_dict())
    up = up.double().eval()
    seq = up.conv.double_conv
    s1, t1 = fold64(seq[0], seq[1], up.up.bias.detach())
    s2, t2 = fold64(seq[3], seq[4])
    np.testing.assert_allclose(t1_32.detach().numpy(), t1.numpy(), rtol=1e-5, atol=1e-6)
    g = torch.Generator().manual_seed(4)
    x = torch.randn((1, 64, 5, 9), generator=g, dtype=torch.float64)
    skip = torch.relu(torch.randn((1, 32, 10, 18), generator=g, dtype=torch.float64))
    with torch.no_grad():
        want = up(x, skip)
        x1 = F.conv_transpose2d(x, up.up.weight, None, stride=2)                    # without its bias: folded into t1
        h, _ = R.conv3x3_c32_ref(torch.cat([skip, x1], dim=1), seq[0].weight, out_scale=s1, out_shift=t1)
        got, _ = R.conv3x3_c32_ref(h, seq[3].weight, out_scale=s2, out_shift=t2)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-12)


def test_heads_reference_equals_the_module_heads_in_float64(nets):
    shp = nets[1]
    w, b = R.pack_heads([fl[0].weight for fl in shp.final_layers], [fl[0].bias for fl in shp.final_layers])
    g = torch.Generator().manual_seed(5)
    h = torch.relu(torch.randn((1, 32, 8, 16), generator=g, dtype=torch.float64))
    z, p, _ = R.heads_ref(h, w, b, 5, 13)
    for k, fl in enumerate(shp.final_layers):
        conv = torch.nn.Conv2d(32, 32, 1).double()
        conv.load_state_dict(fl[0].state_dict())
        with torch.no_grad():
            logits = conv(h)[0, :, :5, :13]
        np.testing.assert_allclose(z[k].numpy(), logits.permute(1, 2, 0).numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(p[k].numpy(), torch.softmax(logits, dim=0).permute(1, 2, 0).numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(p[k].float().numpy(), unet.marks_torch([logits], 5, 13)[0].numpy(), rtol=0, atol=1e-6)


def test_packing_helpers_are_unet_pys_layouts(nets):
    pos, shp = nets
    f = Folds(shp)
    for conv in (pos.backbone.descending_path[0].double_conv[3], pos.backbone.ascending_path[-1].conv.double_conv[0]):
        wp = R.pack_c32(conv.weight)
        assert torch.equal(wp, f._packed(conv))
        cin = conv.in_channels
        assert tuple(wp.shape) == (cin // 32, 9, 32, 32)
        for (s, tap, ci, co) in ((0, 0, 0, 0), (cin // 32 - 1, 5, 7, 31), (0, 8, 31, 3)):
            assert wp[s, tap, ci, co] == conv.weight[co, 32 * s + ci, tap // 3, tap % 3]
    stem = pos.backbone.descending_path[0].double_conv[0]
    ws = R.pack_stem(stem.weight)
    assert tuple(ws.shape) == (9, 3, 32)
    for (tap, ci, co) in ((0, 0, 0), (5, 2, 31), (7, 1, 4)):
        assert ws[tap, ci, co] == stem.weight[co, ci, tap // 3, tap % 3]
    w, b = R.pack_heads([fl[0].weight for fl in shp.final_layers], [fl[0].bias for fl in shp.final_layers])
    fw, fb = f._packed_heads()
    assert torch.equal(w, fw) and torch.equal(b, fb)


# ---- the work split the GPU tests rely on --------------------------------------------------------------------------------------
def test_the_large_shapes_reach_the_persistent_paths_on_256_compute_units():
    H, W = R.C32_BIG
    tx, ty = R.c32_tiles(H, W)
    assert (tx, ty) == (13, 42)
    n_tiles = tx * ty
    grid = R.c32_grid(n_tiles, 256)
    assert grid == 256 and n_tiles >= 2 * grid + 1
    ranges = R.c32_ranges(n_tiles, grid)
    assert sorted(t for a, b in ranges for t in range(a, b)) == list(range(n_tiles))       # every tile once
    assert {b - a for a, b in ranges} == {2, 3}                                            # uneven shares, up to three tiles
    assert any(a // tx != (b - 1) // tx for a, b in ranges)                                # a range that wraps a tile row
    for cus, n in ((256, 3), (304, 8), (8, 17), (20, 100)):
        r = R.c32_ranges(n, R.c32_grid(n, cus))
        assert sorted(t for a, b in r for t in range(a, b)) == list(range(n))
    H, W, _, _ = R.HEADS_SHAPES[-1]
    assert R.heads_groups(H, W) == 8606 > 4 * R.HEADS_MAX_GRID


# ---- float32 stand-ins and wrong kernels --------------------------------------------------------------------------------------
def c32_float32(inp, kw, pad_mode="reflect", drop=None, affine_on_both=False):
    """conv3x3_c32 from torch's CPU float32 operations; the keyword arguments make it wrong in one way each"""
    x, w = inp[0], inp[1]
    if kw["in_scale"] is not None:
        n = x.shape[1] if affine_on_both else 32
        s, t = kw["in_scale"].repeat(n // 32).view(1, -1, 1, 1), kw["in_shift"].repeat(n // 32).view(1, -1, 1, 1)
        x = x.clone()
        x[:, :n] = torch.relu(x[:, :n] * s + t)
    if drop is not None:
        w = w.clone()
        w[:, drop[0], drop[1], drop[2]] = 0.0
    y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode=pad_mode), w)
    if kw["out_scale"] is not None:
        y = y * kw["out_scale"].view(1, -1, 1, 1) + kw["out_shift"].view(1, -1, 1, 1)
    return torch.relu(y) if kw["relu"] else y


C32_CASES = [(cin, H, W, v) for cin in (32, 64) for (H, W) in R.C32_SHAPES for v in R.C32_VARIANTS]


@pytest.fixture(scope="module", params=C32_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[3]}")
def c32(request):
    cin, H, W, variant = request.param
    inp, ref, bound = R.c32_case(cin, H, W, variant)
    return request.param, inp, R.c32_kwargs(inp, variant), ref, bound


def test_c32_bound_holds_for_torch_float32(c32):
    case, inp, kw, ref, bound = c32
    assert ref.dtype == bound.dtype == torch.float64 and bool((bound > 0).all())
    r = R.worst_ratio(c32_float32(inp, kw), ref, bound)
    print(f"conv3x3_c32 {case}: torch float32 max err / bound = {r:.4f}")
    assert r <= 1.0


def wrong_c32_kernels(case, inp, kw):
    cin, H, W, variant = case
    # the dropped term: one tap of the input channel that carries most (after the in-load affine a channel can be all zero
    # on a 2 x 2 image, and dropping a term that is zero is no error)
    x = inp[0]
    if kw["in_scale"] is not None:
        x = torch.cat([torch.relu(x[:, :32] * kw["in_scale"].view(1, -1, 1, 1) + kw["in_shift"].view(1, -1, 1, 1)), x[:, 32:]], dim=1)
    wrong = {"replicate": dict(pad_mode="replicate"), "dropped term": dict(drop=(int(x.abs().sum(dim=(0, 2, 3)).argmax()), 1, 2))}
    if cin == 64 and R.C32_VARIANTS[variant][0]:
        wrong["affine on the second source"] = dict(affine_on_both=True)
    return wrong


def test_c32_bound_rejects_wrong_kernels(c32):
    case, inp, kw, ref, bound = c32
    for name, how in wrong_c32_kernels(case, inp, kw).items():
        r = R.worst_ratio(c32_float32(inp, kw, **how), ref, bound)
        print(f"conv3x3_c32 {case}: {name}: max err / bound = {r:.1f}")
        assert r >= 10.0, name


def stem_float32(inp, pad_mode="reflect", drop=None):
    x, w, sc, sh = inp
    if drop is not None:
        w = w.clone()
        w[:, drop[0], drop[1], drop[2]] = 0.0
    y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode=pad_mode), w)
    return torch.relu(y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))


@pytest.mark.parametrize("H,W", R.STEM_SHAPES)
def test_stem_bound_holds_for_torch_float32_and_rejects_wrong_kernels(H, W):
    inp, ref, bound = R.stem_case(H, W)
    r = R.worst_ratio(stem_float32(inp), ref, bound)
    print(f"stem {H}x{W}: torch float32 max err / bound = {r:.4f}")
    assert r <= 1.0
    # taps read transposed (tap / 3 and tap % 3 swapped) is a wrong kernel of the stem's own
    x, w, sc, sh = inp
    for name, got in (("replicate", stem_float32(inp, pad_mode="replicate")), ("dropped term", stem_float32(inp, drop=(1, 2, 0))),
                      ("transposed taps", stem_float32((x, w.transpose(2, 3).contiguous(), sc, sh)))):
        r = R.worst_ratio(got, ref, bound)
        print(f"stem {H}x{W}: {name}: max err / bound = {r:.1f}")
        assert r >= 10.0, name


def heads_float32(inp, H, W, half_sum=False):
    h, w, b = inp
    out = []
    for k in range(3):
        z = F.conv2d(h, w[k].reshape(32, 32, 1, 1), b[k])[0, :, :H, :W].permute(1, 2, 0)
        if half_sum:                        # the two half-waves never exchange their sums: classes (r & 3) + 8 (r >> 2) + 4 kh
            e = torch.exp(z - z.max(dim=-1, keepdim=True).values)
            half = ((torch.arange(32) >> 2) & 1).bool()
            s = torch.where(half, e[..., half].sum(-1, keepdim=True), e[..., ~half].sum(-1, keepdim=True))
            out.append(e / s)
        else:
            out.append(torch.softmax(z, dim=-1))
    return torch.stack(out)


@pytest.mark.parametrize("H,W,ldh,ldw", R.HEADS_SHAPES)
def test_heads_bound_holds_for_torch_float32_and_rejects_a_wrong_kernel(H, W, ldh, ldw):
    inp, z, p, bound = R.heads_case(H, W, ldh, ldw)
    assert tuple(p.shape) == (3, H, W, 32)
    np.testing.assert_allclose(p.sum(-1).numpy(), 1.0, rtol=0, atol=1e-14)
    assert float((bound / p).max()) < 1e-3                # a bound that leaves every probability three digits
    r = R.worst_ratio(heads_float32(inp, H, W), p, bound)
    print(f"heads {H}x{W}: torch float32 max err / bound = {r:.4f}")
    assert r <= 1.0
    r = R.worst_ratio(heads_float32(inp, H, W, half_sum=True), p, bound)
    assert r >= 10.0
