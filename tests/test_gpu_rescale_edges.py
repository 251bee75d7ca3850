"""``MppContext.rescale`` (``csrc/mpp_rescale.hip``) at small, misaligned and limit-sized inputs: the cases of
``rescale_cases.py`` against their references, with the source on and off the 16-byte grid and the outputs inside
sentinel-filled buffers; every alignment residue and several row pitches on one picture; bands at the column-group edges;
calls back to back; the refusals.  What each case reaches in the kernels is counted on the CPU (``test_rescale_cases_host.py``)."""
import numpy as np
import pytest

import rescale_cases as RC

pytestmark = pytest.mark.gpu

RUN_CASES = [c for c in RC.ALL_CASES if RC.plan(c.H, c.W, c.tables(), addresses=False).refusal is None]
REFUSED = [c for c in RC.ALL_CASES if c not in RUN_CASES]
PAD = 64                       # sentinel elements on either side of an output
U8_SENTINEL, F64_SENTINEL = 0xA5, -7.25


@pytest.fixture(scope="module")
def ctx():
    from mpp_cnn_rs_object_detection_amd import hip_api
    c = hip_api.MppContext(0)
    yield c
    c.close()


def place(img, base=0, pitch=None):
    """``img`` as a [H,W,3] view, rows ``pitch`` bytes apart, whose first byte lies ``base`` bytes into a flat buffer of random
    bytes that starts on a 16-byte boundary and ends with the picture's last byte"""
    import torch
    H, W = img.shape[:2]
    pitch = 3 * W if pitch is None else pitch
    flat = torch.from_numpy(np.random.default_rng(99).integers(0, 256, base + (H - 1) * pitch + 3 * W, dtype=np.uint8)).cuda()
    assert flat.data_ptr() % 16 == 0
    view = flat.as_strided((H, W, 3), (pitch, 3, 1), base)
    view.copy_(torch.from_numpy(np.array(img)).cuda())             # (a copy: the cases' pictures are read-only)
    assert view.data_ptr() % 16 == base % 16 and base + (H - 1) * pitch + 3 * W == flat.numel()
    return view


class Outputs:
    """``out`` (first byte ``shift`` bytes off a 16-byte boundary) and ``out_f64`` as slices of sentinel-filled buffers"""

    def __init__(self, oh, ow, shift=0, f64=True):
        import torch
        n = oh * ow * 3
        self.n, self.shift = n, shift
        self.u8_buf = torch.full((PAD + shift + n + PAD,), U8_SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.u8_buf.data_ptr() % 16 == 0
        self.out = self.u8_buf[PAD + shift:PAD + shift + n].view(oh, ow, 3)
        self.f64_buf = torch.full((PAD + n + PAD,), F64_SENTINEL, dtype=torch.float64, device="cuda") if f64 else None
        self.out_f64 = self.f64_buf[PAD:PAD + n].view(oh, ow, 3) if f64 else None

    def assert_untouched_around(self):
        b = self.u8_buf.cpu().numpy()
        lo = PAD + self.shift
        assert (b[:lo] == U8_SENTINEL).all() and (b[lo + self.n:] == U8_SENTINEL).all(), "bytes written outside out"
        if self.f64_buf is not None:
            f = self.f64_buf.cpu().numpy()
            assert (f[:PAD] == F64_SENTINEL).all() and (f[PAD + self.n:] == F64_SENTINEL).all(), "values written outside out_f64"

    def assert_untouched(self):
        self.assert_untouched_around()
        assert (self.out.cpu().numpy() == U8_SENTINEL).all()
        assert self.out_f64 is None or (self.out_f64.cpu().numpy() == F64_SENTINEL).all()


def run(ctx, src, tables, o, **kw):
    ctx.rescale(src, tables, out=o.out, out_f64=o.out_f64, **kw)
    ctx.synchronize()
    o.assert_untouched_around()
    return o.out.cpu().numpy(), (None if o.out_f64 is None else o.out_f64.cpu().numpy())


@pytest.mark.parametrize("case", RUN_CASES, ids=repr)
def test_values_and_nothing_outside_the_outputs(case, ctx):
    """float64 within the case's tolerance of its reference (1e-12 for Gaussian tables; the term-count bound against
    longdouble for generic ones); the 8-bit output is the truncation of the device's own float64 and equals the reference's
    level wherever the reference settles it (everywhere for pass-through tables; within one level for the flat blocks);
    values the reference puts outside [-tol, 1 + tol] are exactly 0 or 255.  Run with the source and ``out`` on a 16-byte
    boundary and off it (5 bytes and 1 byte), and once without ``out_f64``: the same bits, the sentinels intact."""
    ref, tol, (oh, ow) = case.reference(), case.tolerance(), case.out
    u8, f64 = run(ctx, place(case.image()), case.tables(), Outputs(oh, ow))
    assert ctx.get_option("rescale_bands") == 1
    assert u8.shape == f64.shape == ref.shape
    err = float(np.abs(f64 - ref).max())
    want = RC.ref_uint8(ref)
    keep = np.ones(ref.shape, bool) if case.pass_through() else ~RC.excluded(ref, tol)
    differ = u8 != want
    print(f"{case.name}: max |device - reference| = {err:.3g} (tolerance {tol:.3g}); {int(differ.sum())} of {differ.size} 8-bit "
          f"values differ, {int((differ & keep).sum())} of them where the reference settles the level; {int((~keep).sum())} left out")
    assert err <= tol
    assert np.array_equal(u8, np.floor(255 * np.clip(f64, 0, 1)).astype(np.uint8))
    assert np.array_equal(u8[keep], want[keep])
    if case.flat:
        assert int(np.abs(u8.astype(int) - want.astype(int)).max()) <= 1
    assert (u8[ref < -tol] == 0).all() and (u8[ref > 1 + tol] == 255).all()
    u8b, f64b = run(ctx, place(case.image(), base=5), case.tables(), Outputs(oh, ow, shift=1))
    assert np.array_equal(u8, u8b) and np.array_equal(f64, f64b)
    u8c, _ = run(ctx, place(case.image(), base=5), case.tables(), Outputs(oh, ow, shift=1, f64=False))
    assert np.array_equal(u8, u8c)


def test_every_alignment_and_pitch_gives_the_same_bits(ctx):
    """the first byte at every residue mod 16, rows 3 W, 3 W + 1, + 8, + 16 bytes apart and at the two pitches that are 0 and
    8 mod 16; every view ends on its buffer's last byte"""
    import torch
    c = RC.ALIGN
    o = Outputs(*c.out)
    u8, f64 = run(ctx, place(c.image()), c.tables(), o)
    assert float(np.abs(f64 - c.reference()).max()) <= c.tolerance()
    first_u8, first_f64 = o.out.clone(), o.out_f64.clone()
    wrong = []
    for pitch in RC.ALIGN_PITCHES:
        for base in range(16):
            if (pitch, base) == (3 * c.W, 0):
                continue
            p = Outputs(*c.out)
            ctx.rescale(place(c.image(), base=base, pitch=pitch), c.tables(), out=p.out, out_f64=p.out_f64)
            ctx.synchronize()
            if not (torch.equal(p.out, first_u8) and torch.equal(p.out_f64, first_f64)):
                wrong.append((pitch, base))
    assert not wrong, f"(pitch, first byte) with other bits than the contiguous picture: {wrong}"


@pytest.mark.parametrize("name", ["17x126@0.5", "31x130@0.5"])
def test_bands_at_the_group_edges(name):
    from mpp_cnn_rs_object_detection_amd import hip_api
    c = RC.BY_NAME[name]
    one = RC.plan(c.H, c.W, c.tables(), addresses=False)
    ctx = hip_api.MppContext(0)
    src = place(c.image())
    u8, f64 = run(ctx, src, c.tables(), Outputs(*c.out))
    assert ctx.get_option("rescale_bands") == 1 and ctx.get_option("rescale_bytes") == one.need
    seen = []
    for limit in (RC.band_limit(c, RC.BAND_ROWS), one.need + one.row_bytes, one.need - 1):
        want = RC.plan(c.H, c.W, c.tables(), ws_limit=limit, addresses=False)
        small = hip_api.MppContext(0)                    # a context of its own: its workspace stays within the limit
        u8b, f64b = run(small, src, c.tables(), Outputs(*c.out), workspace_limit=limit)
        seen.append(small.get_option("rescale_bands"))
        assert seen[-1] == len(want.bands)
        assert small.get_option("rescale_bytes") == want.need <= limit
        assert np.array_equal(u8, u8b) and np.array_equal(f64, f64b)
        small.close()
    print(f"{name}: bands at {RC.BAND_ROWS} rows of workspace / one row of slack / one byte short: {seen}")
    assert seen[0] >= 3 and seen[1:] == [1, 2]
    ctx.close()


def test_calls_back_to_back():
    """a small call, a call that needs a larger workspace and a larger pinned table, the small one again: nothing waits in
    between, and each result is that of the same call on a context of its own"""
    from mpp_cnn_rs_object_detection_amd import hip_api
    small, large = RC.BY_NAME["5x7@0.5"], RC.BY_NAME["64x1400@0.0936"]
    alone = []
    for c in (small, large):
        one = hip_api.MppContext(0)
        alone.append(run(one, place(c.image()), c.tables(), Outputs(*c.out)))
        one.close()
    ps, pl = RC.plan(small.H, small.W, small.tables(), addresses=False), RC.plan(large.H, large.W, large.tables(), addresses=False)
    assert pl.need > ps.need and pl.tab_bytes > ps.tab_bytes
    ctx = hip_api.MppContext(0)
    srcs = [place(c.image()) for c in (small, large)]
    outs = [Outputs(*small.out), Outputs(*large.out), Outputs(*small.out)]
    for k, (i, c) in enumerate(((0, small), (1, large), (0, small))):
        ctx.rescale(srcs[i], c.tables(), out=outs[k].out, out_f64=outs[k].out_f64)
    ctx.synchronize()
    assert ctx.get_option("rescale_bytes") == pl.need
    for k, i in enumerate((0, 1, 0)):
        outs[k].assert_untouched_around()
        assert np.array_equal(outs[k].out.cpu().numpy(), alone[i][0]) and np.array_equal(outs[k].out_f64.cpu().numpy(), alone[i][1])
    ctx.close()


def test_refusals_come_before_any_launch(ctx):
    """each with the message's own words and the output sentinels untouched"""
    import torch
    from mpp_cnn_rs_object_detection_amd import hip_api
    assert [c.name for c in REFUSED] == ["64x1400@0.093"]
    c = REFUSED[0]
    q = RC.plan(c.H, c.W, c.tables(), addresses=False)
    assert q.refusal == "LDS"
    o = Outputs(*c.out)
    with pytest.raises(hip_api.MppError, match=rf"{c.tables()[2].shape[1]} taps over a span of {q.span} source columns.*{q.lds} bytes of LDS"):
        ctx.rescale(place(c.image()), c.tables(), out=o.out, out_f64=o.out_f64)
    ctx.synchronize()
    o.assert_untouched()

    c = RC.ALIGN
    src = torch.from_numpy(c.image().copy()).cuda()
    ri, rw, ci, cw = c.tables()
    T = RC.RS_MAX_TAPS + 1
    many = (np.zeros((c.out[0], T), np.int32), np.full((c.out[0], T), 1.0 / T), ci, cw)
    low = RC.plan(c.H, c.W, c.tables(), addresses=False)
    at_H = ri.copy()
    at_H[-1, -1] = c.H
    for tables, kw, word in ((many, {}, "taps"), (c.tables(), {"workspace_limit": low.tab_bytes + low.row_bytes - 1}, "workspace"),
                             ((at_H, rw, ci, cw), {}, "outside")):
        assert RC.plan(c.H, c.W, tables, addresses=False, **({"ws_limit": kw["workspace_limit"]} if kw else {})).refusal == word
        o = Outputs(*c.out)
        with pytest.raises(hip_api.MppError, match=word):
            ctx.rescale(src, tables, out=o.out, out_f64=o.out_f64, **kw)
        ctx.synchronize()
        o.assert_untouched()


def test_detect_image_on_the_lds_boundary(ctx):
    """``detect.detect_image`` at the ``gsd`` that gives the admitted 1400 -> 131 geometry hands on the picture of the rescale
    alone, and the refused 1400 -> 130 one raises the launcher's sentence.  The model is a stand-in that lends its context and
    detects nothing: the U-Nets and the sampler behind ``detect`` are ``test_gpu_detect.py``'s, a model with nets takes longer
    to set up than a test of the rescale may."""
    from mpp_cnn_rs_object_detection_amd import detect, hip_api

    class RescaleOnly:
        nets, device = object(), 0

        def _figure_ctx(self):
            return ctx

        def infer_image(self, data, seed=None):
            self.seen = data
            return [], []

    c, model = RC.BY_NAME["64x1400@0.0936"], RescaleOnly()
    res = detect.detect_image(model, np.array(c.image()), gsd=c.scale, model_gsd=1.0)
    u8, _ = run(ctx, place(c.image()), c.tables(), Outputs(*c.out))
    assert res.scale == c.scale and res.source_shape == (64, 1400) and res.image.shape == (6, 131, 3)
    assert np.array_equal(res.image, np.divide(u8, 255, dtype=np.float32)) and model.seen.image is res.image
    with pytest.raises(hip_api.MppError, match="42 taps over a span of 720 source columns"):
        detect.detect_image(model, np.array(REFUSED[0].image()), gsd=0.093, model_gsd=1.0)
