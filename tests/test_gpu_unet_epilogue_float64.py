"""The four score-map epilogues (csrc/mpp_maps.hip: ``k_posnet_epilogue``, ``k_shapenet_epilogue``, ``k_posnet_epilogue_nhwc<4|2>``,
``k_shapenet_epilogue_nhwc<4|2>``) against the float64 references and derived bounds of tests/unet_epilogue_ref.py, at the
smallest shapes at which each mechanism of the kernels exists (the switch points between the 16-byte and the scalar paths, the
second x-workgroup of the planar PosNet kernel, partially live waves of the channels-last softmax, axes of length 1) and on
benign, saturated and special inputs.  That a case reaches its mechanism is asserted from the launch arithmetic restated in the
reference module and the pointers at hand, not assumed.  Every output buffer is filled with NaN first: a store that never happens
fails the comparison; windows go into a sentinel frame.  What must be exact is compared bit for bit: a repeated call, the
bfloat16 kernel against the float32 kernel fed the rounded values, the scalar against the 16-byte path, a pixel against the same
pixel of a crop, and every pixel a NaN or an infinity must not reach.  tests/test_unet_epilogue_ref_host.py pins the references
and shows that the bounds are neither too tight for float32 nor loose enough to pass a wrong epilogue."""
import pytest
import torch

import unet_epilogue_ref as R
from mpp_cnn_rs_object_detection_amd import hip_api

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
NAN, INF = float("nan"), float("inf")
F32, BF16 = torch.float32, torch.bfloat16
W_, B_ = R.DIV_W, R.DIV_B


@pytest.fixture(scope="module")
def ctx():
    c = hip_api.MppContext(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture(scope="module")
def worst():
    """worst err / bound per (kernel, family group), printed when the module is done"""
    table = {}
    yield table
    for (kernel, group), r in sorted(table.items()):
        print(f"\nworst err / bound, {kernel}, {group}: {r:.4f}", end="")
    print()


def note(worst, kernel, family, r):
    k = (kernel, R.family_group(family))
    worst[k] = max(worst.get(k, 0.0), r)


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


def nhwc(t):
    """[1,C,H,W] on the device over NHWC memory (explicitly: with H or W of 1 torch calls any strides channels-last)"""
    return t.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def planar(x, off=0):
    """x [C, ldh, ldw] on the device, ``off`` floats into a fresh allocation"""
    store = torch.empty(x.numel() + 4, device="cuda")
    v = store[off:off + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


def nan_det(H, W, ld=None):
    """(storage [H, ld], its [H, W] view) filled with NaN"""
    big = torch.full((H, W if ld is None else ld), NAN, device="cuda")
    return big, big[:, :W]


def assert_within(got, ref, bound, what):
    over = R.count_over(got, ref, bound)
    r = R.worst_ratio(got, ref, bound)
    assert over == 0, f"{what}: {over} of {ref.numel()} outputs over the bound (or never stored), worst err / bound {r:.3g}"
    return r


def run_pos_planar(ctx, x, H, W, ld_dst=None, off=0):
    src = planar(x, off)
    big, det = nan_det(H, W, ld_dst)
    ctx.posnet_epilogue(src, H, W, W_, B_, det)
    torch.cuda.synchronize()
    assert bool(torch.isnan(big[:, W:]).all()), "written behind the rows"
    return det.clone(), src.data_ptr(), det.data_ptr()


def run_pos_nhwc(ctx, x, H, W, dtype):
    src = nhwc(x.unsqueeze(0)).to(dtype)
    _, det = nan_det(H, W)
    ctx.posnet_epilogue_nhwc(src, H, W, W_, B_, det)
    torch.cuda.synchronize()
    return det


def run_shp_planar(ctx, z, H, W, off=0):
    src = planar(z, off)
    marks = torch.full((H, W, 32), NAN, device="cuda")
    ctx.shapenet_epilogue(src, H, W, marks)
    torch.cuda.synchronize()
    return marks, src.data_ptr()


def run_shp_nhwc(ctx, z, H, W, dtype):
    src = nhwc(z.unsqueeze(0)).to(dtype)
    marks = torch.full((H, W, 32), NAN, device="cuda")
    ctx.shapenet_epilogue_nhwc(src, H, W, marks)
    torch.cuda.synchronize()
    return marks


def check_marks(got, z, ref, bound, H, W, what):
    """the bound, the row sums and the exact zeros of a softmax output [H, W, 32] on the device"""
    g = got.cpu()
    r = assert_within(g, ref, bound, what)
    assert bool(torch.isfinite(ref).all())
    rows = (g.double().sum(-1) - 1.0).abs()
    assert float(rows.max()) <= 32 * R.U, f"{what}: a row sums to 1 +- {float(rows.max()):.3g}"
    dead = torch.isinf(z[:, :H, :W]).permute(1, 2, 0)
    assert bool((g[dead] == 0).all()), f"{what}: a class with a logit of -inf is not exactly 0"
    return r


# ---- within the bound of float64, every case x family ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.POS_PLANAR_CASES)), ids=lambda i: "{}x{}-ld{}x{}-dst{}-off{}".format(*R.POS_PLANAR_CASES[i]))
def test_planar_posnet_is_within_the_float32_bound_of_float64_and_repeats(ctx, worst, i):
    c = R.POS_PLANAR_CASES[i]
    assert R.pos_planar_grid(c.H, c.W)[0] == (2 if c.W > 1024 else 1)
    for fam in R.POS_FAMILIES:
        x, ref, bound = R.pos_case(fam, c.H, c.W, c.ldh, c.ldw)
        got, src_addr, dst_addr = run_pos_planar(ctx, x, c.H, c.W, c.ld_dst, c.src_off)
        # a condition, not an assumption: the case takes the 16-byte path with as many threads as it says
        ok = R.pos_planar_vec_ok(c.ldh, c.ldw, 0, c.ld_dst, src_addr, dst_addr)
        assert len(R.pos_planar_vector_threads(c.H, c.W, 0, 0, c.H, c.W, ok)) == R.POS_PLANAR_VECTOR_THREADS[i], (src_addr, dst_addr)
        r = assert_within(got, ref, bound, f"planar posnet {tuple(c)} {fam}")
        print(f"planar posnet {tuple(c)} {fam}: max err / bound = {r:.4f}")
        note(worst, "planar posnet", fam, r)
        if fam == "sat constant":                                   # the divergence is exactly 0: one value everywhere
            assert int(bits(got).unique().numel()) == 1
        again, _, _ = run_pos_planar(ctx, x, c.H, c.W, c.ld_dst, c.src_off)
        assert torch.equal(bits(again), bits(got)), fam


@pytest.mark.parametrize("H,W,ldh,ldw", R.SHP_PLANAR_CASES)
def test_planar_shapenet_is_within_the_float32_bound_of_float64_and_repeats(ctx, worst, H, W, ldh, ldw):
    for fam in R.SHP_FAMILIES:
        z, ref, bound = R.shp_case(fam, H, W, ldh, ldw)
        got, src_addr = run_shp_planar(ctx, z, H, W)
        ok = R.shp_planar_vec_ok(ldh, ldw, 0, src_addr)
        assert ok == (ldw % 4 == 0) and len(R.shp_planar_vector_blocks(W, ok)) == (W // 64 if ok else 0)
        r = check_marks(got, z, ref, bound, H, W, f"planar shapenet {H}x{W} of {ldh}x{ldw} {fam}")
        print(f"planar shapenet {H}x{W} of {ldh}x{ldw} {fam}: max err / bound = {r:.4f}")
        note(worst, "planar shapenet", fam, r)
        assert torch.equal(bits(run_shp_planar(ctx, z, H, W)[0]), bits(got)), fam


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("H,W,ldh,ldw", R.POS_NHWC_CASES)
def test_channels_last_posnet_is_within_the_float32_bound_of_float64_and_repeats(ctx, worst, H, W, ldh, ldw, dtype):
    for fam in R.POS_FAMILIES:
        x, ref, bound = R.pos_case(fam, H, W, ldh, ldw, dtype)
        got = run_pos_nhwc(ctx, x, H, W, dtype)
        r = assert_within(got, ref, bound, f"nhwc posnet {dtype} {H}x{W} of {ldh}x{ldw} {fam}")
        print(f"nhwc posnet {dtype} {H}x{W} of {ldh}x{ldw} {fam}: max err / bound = {r:.4f}")
        note(worst, f"nhwc posnet {str(dtype)[6:]}", fam, r)
        if fam == "sat constant":
            assert int(bits(got).unique().numel()) == 1
        assert torch.equal(bits(run_pos_nhwc(ctx, x, H, W, dtype)), bits(got)), fam
        if dtype == BF16:      # the bfloat16 reads: the float32 kernel fed the rounded values computes the same, bit for bit
            assert torch.equal(bits(run_pos_nhwc(ctx, x, H, W, F32)), bits(got)), fam
        # ... and so does the planar kernel (they share div_at / div_score)
        assert torch.equal(bits(run_pos_planar(ctx, x, H, W)[0]), bits(got)), fam


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("H,W,ldh,ldw", R.SHP_NHWC_CASES)
def test_channels_last_shapenet_is_within_the_float32_bound_of_float64_and_repeats(ctx, worst, H, W, ldh, ldw, dtype):
    live = R.shp_nhwc_live_pixels_per_wave(H, W)
    assert sum(live) == H * W and len(live) == 4 * R.shp_nhwc_grid(H, W)
    for fam in R.SHP_FAMILIES:
        z, ref, bound = R.shp_case(fam, H, W, ldh, ldw, dtype)
        got = run_shp_nhwc(ctx, z, H, W, dtype)
        r = check_marks(got, z, ref, bound, H, W, f"nhwc shapenet {dtype} {H}x{W} of {ldh}x{ldw} {fam}")
        print(f"nhwc shapenet {dtype} {H}x{W} of {ldh}x{ldw} {fam}: max err / bound = {r:.4f}")
        note(worst, f"nhwc shapenet {str(dtype)[6:]}", fam, r)
        assert torch.equal(bits(run_shp_nhwc(ctx, z, H, W, dtype)), bits(got)), fam
        if dtype == BF16:
            assert torch.equal(bits(run_shp_nhwc(ctx, z, H, W, F32)), bits(got)), fam
        assert torch.equal(bits(run_shp_planar(ctx, z, H, W)[0]), bits(got)), fam      # (they share softmax_quad)


# ---- one window with odd wx0, wy0 per kernel, against float64 directly ---------------------------------------------------------
@pytest.mark.parametrize("kernel", ["planar posnet", "planar shapenet", "nhwc posnet float32", "nhwc posnet bfloat16",
                                    "nhwc shapenet float32", "nhwc shapenet bfloat16"])
def test_a_window_is_within_the_bound_of_float64_and_stays_inside_its_frame(ctx, worst, kernel):
    H, W, ldh, ldw, wx0, wy0, wh, ww = R.WINDOW
    dtype = BF16 if kernel.endswith("bfloat16") else F32
    pos = "posnet" in kernel
    ox, oy = 3, 5
    for fam in ("benign", "sat field" if pos else "sat wide"):
        x, ref, bound = (R.pos_case if pos else R.shp_case)(fam, H, W, ldh, ldw, dtype)
        frame = torch.full((wh + 7, ww + 11) + (() if pos else (32,)), SENTINEL, device="cuda")
        view = frame[ox:ox + wh, oy:oy + ww]
        if kernel == "planar posnet":
            ctx.posnet_epilogue(planar(x), H, W, W_, B_, view, wx0=wx0, wy0=wy0)
        elif kernel == "planar shapenet":
            ctx.shapenet_epilogue(planar(x), H, W, view, wx0=wx0, wy0=wy0)
        elif pos:
            ctx.posnet_epilogue_nhwc(nhwc(x.unsqueeze(0)).to(dtype), H, W, W_, B_, view, wx0=wx0, wy0=wy0)
        else:
            ctx.shapenet_epilogue_nhwc(nhwc(x.unsqueeze(0)).to(dtype), H, W, view, wx0=wx0, wy0=wy0)
        torch.cuda.synchronize()
        r = assert_within(view.cpu(), ref[wx0:wx0 + wh, wy0:wy0 + ww], bound[wx0:wx0 + wh, wy0:wy0 + ww], f"{kernel} window {fam}")
        print(f"{kernel} window {fam}: max err / bound = {r:.4f}")
        note(worst, kernel, fam, r)
        frame = frame.clone()
        frame[ox:ox + wh, oy:oy + ww] = SENTINEL
        assert bool((frame == SENTINEL).all()), (kernel, fam, "written outside the window")


# ---- what must be exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,ldh,ldw,ld_dst,n_vec", [(3, 13, 8, 16, 16, 2), (5, 1029, 8, 1032, 1032, 768)])
def test_planar_posnet_scalar_path_equals_the_vector_path_bit_for_bit(ctx, H, W, ldh, ldw, ld_dst, n_vec):
    """the same values through the 16-byte path, through an odd pitch, and from a base 4 bytes off: the shared pixels agree"""
    for fam in R.POS_FAMILIES:
        x = R.pos_inputs(fam, ldh, ldw)
        vec, sa, da = run_pos_planar(ctx, x, H, W, ld_dst)
        ok = R.pos_planar_vec_ok(ldh, ldw, 0, ld_dst, sa, da)
        assert len(R.pos_planar_vector_threads(H, W, 0, 0, H, W, ok)) == n_vec
        odd, sa, da = run_pos_planar(ctx, x[:, :, :W].contiguous(), H, W, ld_dst)
        assert W % 4 and not R.pos_planar_vec_ok(ldh, W, 0, ld_dst, sa, da)
        off, sa, da = run_pos_planar(ctx, x, H, W, ld_dst, off=1)
        assert not R.pos_planar_vec_ok(ldh, ldw, 0, ld_dst, sa, da)
        dense, sa, da = run_pos_planar(ctx, x, H, W)                     # a destination pitch of W, odd: scalar as well
        assert not R.pos_planar_vec_ok(ldh, ldw, 0, W, sa, da)
        assert not bool(torch.isnan(vec).any())
        for name, other in (("odd pitch", odd), ("offset base", off), ("dense destination", dense)):
            assert torch.equal(bits(other), bits(vec)), (fam, name)


def test_planar_shapenet_scalar_loads_equal_the_vector_loads_bit_for_bit(ctx):
    H, W, ldh, ldw = 2, 129, 8, 136
    for fam in R.SHP_FAMILIES:
        z = R.shp_inputs(fam, ldh, ldw)
        vec, sa = run_shp_planar(ctx, z, H, W)
        assert R.shp_planar_vector_blocks(W, R.shp_planar_vec_ok(ldh, ldw, 0, sa)) == [0, 1]
        odd, sa = run_shp_planar(ctx, z[:, :, :W].contiguous(), H, W)
        assert R.shp_planar_vector_blocks(W, R.shp_planar_vec_ok(ldh, W, 0, sa)) == []
        off, sa = run_shp_planar(ctx, z, H, W, off=1)
        assert R.shp_planar_vector_blocks(W, R.shp_planar_vec_ok(ldh, ldw, 0, sa)) == []
        assert not bool(torch.isnan(vec).any())
        assert torch.equal(bits(odd), bits(vec)) and torch.equal(bits(off), bits(vec)), fam


@pytest.mark.parametrize("form", ["planar", "nhwc float32", "nhwc bfloat16"])
def test_a_posnet_pixel_equals_the_same_pixel_of_a_crop_that_holds_its_stencil(ctx, form):
    """crops whose borders are the image's where they touch them; elsewhere the outermost ring of the crop is not compared"""
    H, W, ldh, ldw = 5, 1029, 8, 1032
    dtype = BF16 if form.endswith("bfloat16") else F32

    def run(x, h, w):
        if form == "planar":
            return run_pos_planar(ctx, x, h, w, -(-w // 4) * 4)[0]
        return run_pos_nhwc(ctx, x, h, w, dtype)

    for fam in ("benign", "sat field"):
        x = R.as_dtype(R.pos_inputs(fam, ldh, ldw), dtype)
        full = run(x, H, W)
        assert not bool(torch.isnan(full).any())
        # (rows r0:r1, columns c0:c1) of the image; a side off the image's border loses one ring
        for (r0, r1, c0, c1) in ((0, 4, 1000, 1029), (1, 5, 0, 41), (1, 4, 1016, 1029), (0, 5, 3, 1029)):
            crop = run(x[:, r0:r1, c0:c1].contiguous(), r1 - r0, c1 - c0)
            a0, a1 = (r0 if r0 == 0 else r0 + 1), (r1 if r1 == H else r1 - 1)
            b0, b1 = (c0 if c0 == 0 else c0 + 1), (c1 if c1 == W else c1 - 1)
            assert a1 > a0 and b1 > b0
            assert torch.equal(bits(crop[a0 - r0:a1 - r0, b0 - c0:b1 - c0]), bits(full[a0:a1, b0:b1])), (fam, r0, r1, c0, c1)


def test_a_shapenet_pixel_does_not_depend_on_its_place_in_the_block(ctx):
    H, W, ldh, ldw = 2, 129, 8, 136
    for fam in ("benign", "sat wide"):
        z = R.shp_inputs(fam, ldh, ldw)
        full = run_shp_planar(ctx, z, H, W)[0]
        for (r0, r1, c0, c1) in ((1, 2, 61, 129), (0, 2, 3, 70)):
            crop = z[:, r0:r1, c0:c1].contiguous()
            assert torch.equal(bits(run_shp_planar(ctx, crop, r1 - r0, c1 - c0)[0]), bits(full[r0:r1, c0:c1])), fam
            assert torch.equal(bits(run_shp_nhwc(ctx, crop, r1 - r0, c1 - c0, F32)), bits(full[r0:r1, c0:c1])), fam


# ---- locality of NaN and infinity -----------------------------------------------------------------------------------------------------
#: (form, H, W, ldh, ldw, [(row, col)]): a pixel in the middle of a wave and the last live pixel of a partially live wave
SHP_LOCALITY = [
    ("planar", 2, 63, 8, 64, [(0, 24), (1, 62)]),               # scalar loads; the last quad of the block's last wave is dead
    ("planar", 2, 129, 8, 136, [(1, 88), (1, 128)]),            # 16-byte loads; the third block of a row holds one live pixel
    ("nhwc float32", 7, 9, 8, 12, [(2, 6), (6, 8)]),            # 63 pixels: pixel 24 in the second wave, pixel 62 the last live one
    ("nhwc bfloat16", 7, 9, 8, 12, [(2, 6), (6, 8)]),
    ("nhwc float32", 5, 13, 5, 16, [(0, 7), (4, 12)]),          # 65 pixels: the fifth wave holds one live pixel
]


@pytest.mark.parametrize("form,H,W,ldh,ldw,pixels", SHP_LOCALITY)
def test_a_nan_or_infinite_logit_stays_in_its_pixel(ctx, form, H, W, ldh, ldw, pixels):
    """all 32 outputs of the pixel are NaN (softmax of a NaN; inf - inf), and no other pixel's bits change: what the quad
    shuffles exchange never crosses a pixel"""
    dtype = BF16 if form.endswith("bfloat16") else F32
    run = (lambda z: run_shp_planar(ctx, z, H, W)[0]) if form == "planar" else (lambda z: run_shp_nhwc(ctx, z, H, W, dtype))
    if form != "planar":
        live = R.shp_nhwc_live_pixels_per_wave(H, W)
        last = pixels[1][0] * W + pixels[1][1]
        assert last == H * W - 1 and 0 < live[last // 16] < 16 and live[(pixels[0][0] * W + pixels[0][1]) // 16] == 16
    base_in = R.as_dtype(R.shp_inputs("benign", ldh, ldw), dtype)
    base = run(base_in)
    assert not bool(torch.isnan(base).any())
    for (i, j) in pixels:
        for cls, val in ((13, NAN), (0, INF), (31, NAN)):
            z = base_in.clone()
            z[cls, i, j] = val
            ref, _ = R.shapenet_ref(z, H, W)
            got = run(z)
            assert bool(torch.isnan(ref[i, j]).all()) and int(torch.isnan(ref).sum()) == 32
            assert bool(torch.isnan(got[i, j]).all()), (i, j, cls, val)
            keep = torch.ones((H, W), dtype=torch.bool)
            keep[i, j] = False
            assert torch.equal(bits(got)[keep], bits(base)[keep]), (i, j, cls, val)


POS_LOCALITY = [
    ("planar", 3, 13, 8, 16, 16, [(1, 6), (0, 0), (2, 12), (1, 4), (1, 12)]),
    ("planar", 5, 1029, 8, 1032, 1032, [(2, 1024), (0, 5), (4, 1028), (2, 1027), (3, 1023)]),
    ("planar", 1, 7, 8, 8, 7, [(0, 0), (0, 3)]),
    ("nhwc float32", 3, 257, 4, 260, None, [(1, 255), (0, 256), (2, 0)]),
    ("nhwc bfloat16", 3, 257, 4, 260, None, [(1, 256), (1, 100)]),
    ("nhwc float32", 5, 1, 6, 2, None, [(0, 0), (2, 0)]),
]


@pytest.mark.parametrize("form,H,W,ldh,ldw,ld_dst,places", POS_LOCALITY)
def test_a_nan_reaches_exactly_the_posnet_pixels_whose_stencil_reads_it(ctx, form, H, W, ldh, ldw, ld_dst, places):
    """a NaN in vec0 at (i, j) reaches rows i +- 1 of column j, and (i, j) itself only through a one-sided difference; in vec1
    the same along the row; in the mask (i, j) alone; behind the crop's last column or row nothing.  The expected set is the
    reference's."""
    dtype = BF16 if form.endswith("bfloat16") else F32
    run = (lambda x: run_pos_planar(ctx, x, H, W, ld_dst)[0]) if form == "planar" else (lambda x: run_pos_nhwc(ctx, x, H, W, dtype))
    base_in = R.as_dtype(R.pos_inputs("benign", ldh, ldw), dtype)
    base = run(base_in)
    assert not bool(torch.isnan(base).any())
    outside = ([(0, W)] if ldw > W else []) + ([(H, 0)] if ldh > H else [])
    seen = set()
    for (i, j) in places + outside:
        for ch in range(3):
            x = base_in.clone()
            x[ch, i, j] = NAN
            want = torch.isnan(R.posnet_ref(x, H, W)[0])
            got = run(x)
            assert torch.equal(torch.isnan(got).cpu(), want), (ch, i, j, want.nonzero().tolist(), torch.isnan(got).nonzero().tolist())
            assert torch.equal(bits(got)[~want], bits(base)[~want]), (ch, i, j)
            if (i, j) in outside or (ch == 0 and H == 1) or (ch == 1 and W == 1):
                assert int(want.sum()) == 0                      # behind the crop, or an axis of length 1: never read
            seen.add(int(want.sum()))
    assert 1 in seen and (2 in seen or min(H, W) == 1)
