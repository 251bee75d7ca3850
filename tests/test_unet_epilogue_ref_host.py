"""The references of tests/unet_epilogue_ref.py, pinned without a GPU: they are ``torch.gradient``, ``torch.sigmoid`` and
``torch.softmax`` in float64 (and within their own bounds of unet.py's float32 forms); their bounds hold for a numpy float32
restatement of each epilogue on every case and family tests/test_gpu_unet_epilogue_float64.py uses (so they ask nothing a
correct float32 kernel cannot give), and each of a list of wrong epilogues breaks them on a named case (so they ask enough).  The
case constants reach the mechanisms their comments claim, by the launch arithmetic restated in the reference module."""
import numpy as np
import pytest
import torch

import unet_epilogue_ref as R
from mpp_cnn_rs_object_detection_amd import unet

DTYPES = (torch.float32, torch.bfloat16)
POS_SHAPES = [(c.H, c.W, c.ldh, c.ldw) for c in R.POS_PLANAR_CASES] + R.POS_NHWC_CASES + [R.WINDOW[:4]]
SHP_SHAPES = R.SHP_PLANAR_CASES + R.SHP_NHWC_CASES + [R.WINDOW[:4]]


# ---- the references are torch's operations in float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,ldh,ldw", [(2, 2, 2, 2), (2, 9, 8, 16), (3, 13, 8, 13), (5, 6, 8, 8), (7, 75, 8, 80)])
def test_posnet_reference_equals_torch_gradient_and_sigmoid_in_float64(H, W, ldh, ldw):
    x = R.pos_inputs("benign", ldh, ldw).double()
    c = x[:, :H, :W]
    div = torch.gradient(c[0], dim=0)[0] + torch.gradient(c[1], dim=1)[0]
    want = torch.sigmoid(R.DIV_W * (div * torch.sigmoid(c[2])) + R.DIV_B)
    q, bound = R.posnet_ref(x, H, W)
    assert q.dtype == bound.dtype == torch.float64 and tuple(q.shape) == (H, W) and bool((bound > 0).all())
    np.testing.assert_allclose(q.numpy(), want.numpy(), rtol=0, atol=1e-15)
    # the channels-last layout gives the same reference, bit for bit
    q2, b2 = R.posnet_ref(x.permute(1, 2, 0).contiguous(), H, W, layout="nhwc")
    assert torch.equal(q, q2) and torch.equal(bound, b2)
    # unet.py's own form (float32 inside) is within the bound of it
    got = unet.detection_map_torch(x, H, W, R.DIV_W, R.DIV_B)
    assert R.worst_ratio(got, q, bound) <= 1.0


def test_posnet_reference_on_an_axis_of_length_1_is_grad1s_rule():
    """torch.gradient refuses an axis of length 1; ``grad1`` (csrc/mpp_unet_math.hpp) states the project's rule: gradient 0"""
    x = R.pos_inputs("benign", 8, 8).double()
    with pytest.raises(RuntimeError):
        torch.gradient(x[0, :1, :7], dim=0)
    q, _ = R.posnet_ref(x, 1, 7)                                             # g0 = 0: only d vec1 / d col is left
    want = torch.sigmoid(R.DIV_W * (torch.gradient(x[1, :1, :7], dim=1)[0] * torch.sigmoid(x[2, :1, :7])) + R.DIV_B)
    np.testing.assert_allclose(q.numpy(), want.numpy(), rtol=0, atol=1e-15)
    q, _ = R.posnet_ref(x, 3, 1)                                             # g1 = 0
    want = torch.sigmoid(R.DIV_W * (torch.gradient(x[0, :3, :1], dim=0)[0] * torch.sigmoid(x[2, :3, :1])) + R.DIV_B)
    np.testing.assert_allclose(q.numpy(), want.numpy(), rtol=0, atol=1e-15)
    q, _ = R.posnet_ref(x, 1, 1)                                             # no divergence at all: sigmoid(b)
    assert abs(float(q) - 1.0 / (1.0 + np.exp(-R.DIV_B))) <= 1e-16


@pytest.mark.parametrize("family", ["benign", "sat wide", "neg inf"])
def test_shapenet_reference_equals_torch_softmax_in_float64(family):
    H, W, ldh, ldw = 2, 65, 8, 72
    z = R.shp_inputs(family, ldh, ldw).double()
    p, bound = R.shapenet_ref(z, H, W)
    assert p.dtype == bound.dtype == torch.float64 and tuple(p.shape) == (H, W, 32) and bool((bound > 0).all())
    want = torch.softmax(z[:, :H, :W], dim=0).permute(1, 2, 0)
    np.testing.assert_allclose(p.numpy(), want.numpy(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(p.sum(-1).numpy(), 1.0, rtol=0, atol=1e-14)
    p2, b2 = R.shapenet_ref(z.permute(1, 2, 0).contiguous(), H, W, layout="nhwc")
    assert torch.equal(p, p2) and torch.equal(bound, b2)
    got = unet.marks_torch([z], H, W)[0]                                    # float32 inside
    assert R.worst_ratio(got, p, bound) <= 1.0
    if family == "benign":
        assert float((bound / p).max()) < 1e-4             # a bound that leaves every probability four digits


def test_bf16_round_is_torchs_rounding_and_truncation_is_not():
    x = torch.cat([R.shp_inputs("sat wide", 8, 8).flatten(), torch.tensor([1.00390625, 1.01171875, -1.00390625, 0.0, -0.0])])
    want = x.to(torch.bfloat16).float()
    assert torch.equal(torch.from_numpy(R.bf16_round(x.numpy())), want)       # (two of the values are ties: to even)
    assert not torch.equal(torch.from_numpy(R.bf16_truncate(x.numpy())), want)


# ---- E, and the bounds are not too tight -------------------------------------------------------------------------------------------
def restatement_ratios(exp=R.expf):
    """worst err / bound of the numpy float32 restatements per (kernel, family group, input type), over every shape"""
    worst = {}
    for dt in DTYPES:
        for fam in R.POS_FAMILIES:
            for (H, W, ldh, ldw) in POS_SHAPES:
                x, ref, bound = R.pos_case(fam, H, W, ldh, ldw, dt)
                r = R.worst_ratio(R.posnet_f32(x.numpy(), H, W, exp=exp), ref, bound)
                k = ("posnet", fam, dt)
                worst[k] = max(worst.get(k, 0.0), r)
        for fam in R.SHP_FAMILIES:
            for (H, W, ldh, ldw) in SHP_SHAPES:
                z, ref, bound = R.shp_case(fam, H, W, ldh, ldw, dt)
                r = R.worst_ratio(R.shapenet_f32(z.numpy(), H, W, exp=exp), ref, bound)
                k = ("shapenet", fam, dt)
                worst[k] = max(worst.get(k, 0.0), r)
    return worst


def test_the_float32_restatements_stay_within_the_bounds_and_E_is_twice_their_expf_error():
    args = []

    def recording(a):
        args.append(np.asarray(a, dtype=np.float32).ravel().copy())
        return R.expf(a)

    worst = restatement_ratios(recording)
    for (kernel, fam, dt), r in worst.items():
        print(f"{kernel} {fam} {str(dt)[6:]}: numpy float32 max err / bound = {r:.4f}")
        assert r < 1.0, (kernel, fam, dt)
    # exact results: a dominating class gives exactly 1 and 31 zeros, equal logits give exactly 1/32 -- in float32 as in float64
    assert max(r for (k, fam, _), r in worst.items() if fam not in ("sat dominant", "sat equal", "neg zero", "sat constant")) > 0.05
    a = np.concatenate(args)
    measured = R.exp_ulp_error(a)
    print(f"numpy float32 exp over {a.size} arguments of the cases: worst error {measured:.4f} ulp; E = 2 x {R.E_MEASURED} = {R.E_ULP}")
    assert 0.5 <= measured <= R.E_MEASURED and R.E_ULP == 2 * R.E_MEASURED


# ---- the bounds are not too loose: wrong epilogues ---------------------------------------------------------------------------------
def worst_case_of(run, cases):
    """(worst ratio, its case) of run(case) -> ratio"""
    return max(((run(*c), c) for c in cases), key=lambda t: t[0])


@pytest.mark.parametrize("wrong", R.POS_MUTANTS)
def test_posnet_bound_rejects_a_wrong_epilogue(wrong):
    def ratio(fam, H, W, ldh, ldw):
        x, ref, bound = R.pos_case(fam, H, W, ldh, ldw)
        return R.worst_ratio(R.posnet_f32(x.numpy(), H, W, wrong=wrong), ref, bound)

    r, case = worst_case_of(ratio, [("benign",) + s for s in POS_SHAPES])
    print(f"posnet, {wrong}: max err / bound = {r:.3g} on {case}")
    assert r > 1.0
    # and on the small cases that hold the mechanism: an interior row (3 rows) resp. an interior column
    small = (3, 9, 8, 16)
    assert ratio("benign", *small) > 1.0, small


@pytest.mark.parametrize("wrong", R.SHP_MUTANTS)
def test_shapenet_bound_rejects_a_wrong_epilogue(wrong):
    def ratio(fam, H, W, ldh, ldw):
        z, ref, bound = R.shp_case(fam, H, W, ldh, ldw)
        return R.worst_ratio(R.shapenet_f32(z.numpy(), H, W, wrong=wrong), ref, bound)

    fams = ["sat wide"] if wrong == "no max" else ["benign", "sat wide"]     # without the max only saturation shows
    r, case = worst_case_of(ratio, [(f,) + s for f in fams for s in SHP_SHAPES if s[1] > 1 or wrong != "left neighbour"])
    print(f"shapenet, {wrong}: max err / bound = {r:.3g} on {case}")
    assert r > 1.0
    if wrong == "no max":
        assert ratio("benign", 2, 65, 8, 72) <= 1.0                          # (softmax is shift-invariant: benign logits hide it)
    else:
        assert ratio("benign", 3, 5, 3, 5) > 1.0


@pytest.mark.parametrize("kernel", ["posnet", "shapenet"])
def test_bound_rejects_truncation_to_bfloat16_on_the_input_side(kernel):
    """the reference of a bfloat16 input is of the values rounded to nearest even: an epilogue fed truncated values is wrong"""
    if kernel == "posnet":
        H, W, ldh, ldw = 3, 257, 4, 260
        x, ref, bound = R.pos_case("benign", H, W, ldh, ldw, torch.bfloat16)
        src = R.pos_inputs("benign", ldh, ldw).numpy()
        run = lambda v: R.posnet_f32(v, H, W)                                 # noqa: E731
    else:
        H, W, ldh, ldw = 5, 13, 5, 16
        x, ref, bound = R.shp_case("benign", H, W, ldh, ldw, torch.bfloat16)
        src = R.shp_inputs("benign", ldh, ldw).numpy()
        run = lambda v: R.shapenet_f32(v, H, W)                               # noqa: E731
    assert np.array_equal(R.bf16_round(src), x.numpy())
    assert R.worst_ratio(run(R.bf16_round(src)), ref, bound) < 1.0
    r = R.worst_ratio(run(R.bf16_truncate(src)), ref, bound)
    print(f"{kernel}, bf16 truncation on {H}x{W}: max err / bound = {r:.3g}")
    assert r > 1.0


# ---- saturated inputs: what the bound's floor allows ---------------------------------------------------------------------------------
def test_saturated_references_reach_the_floor_and_both_ends():
    """the saturated families do saturate: references below 2^-126 (a float32 kernel may return exactly 0 there, and the
    bound's floor allows it), references that round to 1, and a constant field whose every output is sigmoid(b)"""
    x, q, bound = R.pos_case("sat field", 5, 1029, 8, 1032)
    assert bool((q < R.FLT_MIN).any()) and bool((q > 1 - R.U / 2).any()) and bool(torch.isfinite(q).all())
    assert bool((bound[q < R.FLT_MIN] >= q[q < R.FLT_MIN]).all())             # 0.0 is within the bound there
    z = R.DIV_W * (torch.gradient(x[0, :5, :1029].double(), dim=0)[0] + torch.gradient(x[1, :5, :1029].double(), dim=1)[0])
    assert float(z.abs().max()) > 200                                          # |w x + b| reaches 200
    x, q, bound = R.pos_case("sat mask", 3, 13, 8, 16)
    assert set(x[2].unique().tolist()) == {-100.0, -20.0, 20.0, 100.0}
    x, q, bound = R.pos_case("sat constant", 3, 13, 8, 16)
    assert bool((q == 1.0 / (1.0 + np.exp(-R.DIV_B))).all())
    assert float(bound.max()) < 8 * R.U                                        # ... to a few ulp: the divergence carries no error
    z, p, bound = R.shp_case("sat wide", 2, 129, 8, 136)
    assert float((p < R.FLT_MIN).double().mean()) > 0.4                       # nearly half of the expf(v - m) underflow
    z, p, bound = R.shp_case("sat dominant", 2, 129, 8, 136)
    assert bool((p.max(-1).values >= 1 - 1e-15).all()) and bool((p.min(-1).values < 1e-35).all())
    z, p, bound = R.shp_case("sat tie", 2, 129, 8, 136)
    top = z[:, :2, :129].max(0).values
    assert bool(((z[:, :2, :129] == top).sum(0) == 2).all())
    for q4 in range(4):
        z, p, _ = R.shp_case(f"sat group {q4}", 2, 129, 8, 136)
        assert bool((p.argmax(-1) // 8 == q4).all())
    z, p, _ = R.shp_case("neg inf", 2, 129, 8, 136)
    dead = torch.isinf(z[:, :2, :129]).permute(1, 2, 0)
    assert bool(dead.any()) and bool((p[dead] == 0).all()) and bool((p[~dead] > 0).all()) and int((~dead[0, 0]).sum()) == 1


# ---- the case constants reach what their comments claim --------------------------------------------------------------------------
def test_planar_posnet_cases_reach_the_vector_path_where_they_say():
    assert len(R.POS_PLANAR_VECTOR_THREADS) == len(R.POS_PLANAR_CASES)
    for c, n in zip(R.POS_PLANAR_CASES, R.POS_PLANAR_VECTOR_THREADS):
        assert c.ldh >= c.H and c.ldw >= c.W and c.ld_dst >= c.W
        ok = R.pos_planar_vec_ok(c.ldh, c.ldw, 0, c.ld_dst, 4 * c.src_off, 0)   # (an allocation's base is 16-byte aligned)
        thr = R.pos_planar_vector_threads(c.H, c.W, 0, 0, c.H, c.W, ok)
        assert len(thr) == n, c
    by = {tuple(c): c for c in R.POS_PLANAR_CASES}
    assert R.pos_planar_vec_ok(8, 8, 0, 8, 0, 0) and R.pos_planar_vector_threads(3, 8, 0, 0, 3, 8, True) == []
    assert R.pos_planar_vector_threads(3, 9, 0, 0, 3, 9, True) == [(1, 4)]
    assert R.pos_planar_vector_threads(3, 12, 0, 0, 3, 12, True) == [(1, 4)]
    assert R.pos_planar_vector_threads(3, 13, 0, 0, 3, 13, True) == [(1, 4), (1, 8)]
    assert not R.pos_planar_vec_ok(8, 13, 0, 16, 0, 0) and not R.pos_planar_vec_ok(8, 16, 0, 16, 4, 0)
    assert (3, 13, 8, 16, 16, 1) in by and (3, 13, 8, 13, 16, 0) in by
    # the second x-workgroup: threads j4 = 1024 (vector, in the interior rows) and 1028 (one pixel)
    assert R.pos_planar_grid(5, 1029) == (2, 5) and R.pos_planar_grid(5, 1024) == (1, 5)
    thr = R.pos_planar_vector_threads(5, 1029, 0, 0, 5, 1029, True)
    assert [(r, j) for r, j in thr if j >= 1024] == [(1, 1024), (2, 1024), (3, 1024)] and 1029 - 1024 == 5
    # the window: odd wy0 leaves the scalar path only
    H, W, ldh, ldw, wx0, wy0, wh, ww = R.WINDOW
    assert wx0 % 2 == 1 and wy0 % 2 == 1 and not R.pos_planar_vec_ok(ldh, ldw, wy0, 96, 0, 0)


def test_planar_shapenet_cases_reach_both_load_paths():
    want = {1: [], 63: [], 64: [0], 65: [0], 128: [0, 1], 129: [0, 1]}
    for (H, W, ldh, ldw) in R.SHP_PLANAR_CASES:
        ok = R.shp_planar_vec_ok(ldh, ldw, 0, 0)
        assert ok == (ldw % 4 == 0) and ldw >= W and ldh >= H
        assert R.shp_planar_vector_blocks(W, ok) == (want[W] if ok else []), (H, W, ldh, ldw)
        assert R.shp_planar_grid(H, W) == (len(want[W]) + (W % 64 != 0), H)
    assert (2, 65, 8, 65) in R.SHP_PLANAR_CASES and (2, 65, 8, 72) in R.SHP_PLANAR_CASES
    assert {(H, W) for H, W, _, _ in R.SHP_PLANAR_CASES} >= {(H, W) for H in (1, 2) for W in (1, 63, 64, 65, 128, 129)}
    H, W, ldh, ldw, wx0, wy0, wh, ww = R.WINDOW
    assert R.shp_planar_grid(wh, ww) == (2, wh) and R.shp_nhwc_grid(wh, ww) == 6 and R.pos_nhwc_grid(wh, ww) == (1, wh)


def test_channels_last_cases_reach_the_workgroup_edges_and_partial_waves():
    assert sorted(R.pos_nhwc_grid(H, W)[0] for H, W, _, _ in R.POS_NHWC_CASES if H == 3) == [1, 1, 1, 1, 2]
    assert {(H, W) for H, W, _, _ in R.POS_NHWC_CASES} == {(3, 1), (3, 2), (3, 255), (3, 256), (3, 257), (1, 5), (5, 1)}
    assert sorted(H * W for H, W, _, _ in R.SHP_NHWC_CASES) == [1, 15, 16, 17, 63, 64, 65]
    live = {H * W: R.shp_nhwc_live_pixels_per_wave(H, W) for H, W, _, _ in R.SHP_NHWC_CASES}
    assert live[1] == [1, 0, 0, 0] and live[15] == [15, 0, 0, 0] and live[16] == [16, 0, 0, 0] and live[17] == [16, 1, 0, 0]
    assert live[63] == [16, 16, 16, 15] and live[64] == [16] * 4 and live[65] == [16] * 4 + [1, 0, 0, 0]
    # a row that ends inside a wave: a wave holds pixels of two rows
    assert sum(1 for H, W, _, _ in R.SHP_NHWC_CASES if H > 1 and W % 16 != 0) >= 1
    for (H, W, ldh, ldw) in R.POS_NHWC_CASES + R.SHP_NHWC_CASES:
        assert ldh >= H and ldw >= W
