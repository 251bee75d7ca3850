"""Float64 references of the four score-map epilogues of csrc/mpp_maps.hip (``k_posnet_epilogue``, ``k_shapenet_epilogue`` and
their channels-last forms ``k_posnet_epilogue_nhwc<4|2>``, ``k_shapenet_epilogue_nhwc<4|2>``) with an error bound per output
that is derived from the float32 format, not measured on the kernels.  Plain torch and numpy on the CPU; nothing of the library is
imported.  tests/test_unet_epilogue_ref_host.py shows that the references are torch's own operations in float64, that the bounds
hold for a numpy float32 restatement of each epilogue and that wrong epilogues break them; tests/test_gpu_unet_epilogue_float64.py
holds the kernels to them.

The references are written from the operations' definitions (``torch.gradient``'s rule per axis, sigmoid, softmax), not from the
kernels.  One rule is the project's own: an axis of length 1 has gradient 0 (``grad1`` in csrc/mpp_unet_math.hpp states it;
``torch.gradient`` refuses such an axis).  Inputs are float32 values widened exactly; a bfloat16 input is the bfloat16 value
widened exactly (the caller rounds, ``bf16_round`` is that rounding).  ``w`` and ``b`` reach the kernels as float32
(csrc/mpp_launch.hpp), so the references round them to float32 first.

The bounds are first-order running errors: the float32 operation sequence of csrc/mpp_unet_math.hpp is followed in float64 and
every operation adds its own rounding error to the errors its operands carry.

  u = 2^-24   each + - * / of float32 errs by at most u relative to its exact result (the build forms no FMA,
              -ffp-contract=off, so each operation rounds on its own);
  E ulp       the error of one ``expf`` result, at most 2 E u relative (an ulp is between u and 2 u of the value);
  2^-126      an absolute floor wherever a product, a quotient or an ``expf`` result can fall below the smallest normal float32:
              such a result may be flushed to zero, which no relative term expresses.  A true value below 2^-126 may come out 0.

E cannot be derived here.  The ROCm installation ships no accuracy table of its device math library (neither its HIP headers nor
its share/doc state an error of ``expf``), so there is no file to cite and E is obtained the other way: the worst ``expf``
error of the CPU float32 restatement below (numpy's float32 ``exp``) against float64 over ALL inputs of all cases and families
of this module (1.7 million arguments, float32 and bfloat16 inputs), doubled.  Measured: 2.3313 ulp
(``E_MEASURED`` rounds it up to 2.34); factor 2; E = 4.68 ulp.  test_unet_epilogue_ref_host.py repeats the measurement and fails
if it exceeds ``E_MEASURED``.  Nothing in it comes from a kernel's behaviour."""
import collections
import functools

import numpy as np
import torch

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
#: worst error of numpy's float32 exp against float64 over the inputs of this module, in ulp, rounded up (see the docstring)
E_MEASURED = 2.34
E_ULP = 2.0 * E_MEASURED
NCLASS = 32
WAVE = 64
#: the "div_clf" scalars the tests use, as the float32 values the kernels receive
DIV_W, DIV_B = float(np.float32(-10.8)), float(np.float32(-2.1))


# ---- references ---------------------------------------------------------------------------------------------------------------------
def _planar64(t, layout, channels, H=None, W=None):
    """the H x W crop of a planar [C][ldh][ldw] or channels-last [ldh][ldw][C] tensor as a dense float64 [C, H, W] (widening is
    exact; dense, so that what torch computes from it does not depend on the layout it came in)"""
    t = torch.as_tensor(t).detach().cpu()
    if t.dim() == 4:
        t = t[0]
    if layout == "nhwc":
        t = t.permute(2, 0, 1)
    elif layout != "planar":
        raise ValueError(layout)
    assert t.dim() == 3 and t.shape[0] == channels, tuple(t.shape)
    return t[:, :H, :W].double().contiguous()


def _gradient(v, dim):
    """``torch.gradient(v, dim=dim)`` with unit spacing -- one-sided at both ends, central inside -- and the running error of
    its float32 form: a one-sided difference is one subtraction (u |g|); a central one is a subtraction and a division by 2
    (u |d| / 2 carried through the division, plus u |g| of the division itself).  An axis of length 1: gradient 0, no error
    (``grad1``, csrc/mpp_unet_math.hpp: nothing is read)."""
    g, e = torch.zeros_like(v), torch.zeros_like(v)
    n = v.shape[dim]
    if n == 1:
        return g, e
    vv, gg, ee = v.movedim(dim, 0), g.movedim(dim, 0), e.movedim(dim, 0)
    gg[0], gg[-1] = vv[1] - vv[0], vv[-1] - vv[-2]
    ee[0], ee[-1] = U * gg[0].abs(), U * gg[-1].abs()
    if n > 2:
        d = vv[2:] - vv[:-2]
        gg[1:-1] = d / 2
        ee[1:-1] = U * d.abs() / 2 + U * (d / 2).abs()
    return g, e


def _sigmoid(x, ex):
    """sigmoid(x) and the running error of 1 / (1 + expf(-x)) for an argument that carries the error ex.

    t = expf(-x) errs relatively by d1 = expm1(ex) + 2 E u (the argument's error sits in the exponent; the negation is exact).
    r = 1 / (1 + t) has dr/dt = -r^2, so t's error moves r by r (1 - r) d1 to first order (the factor 1 + d1 pays the second
    order: |r''| t^2 d1^2 / 2 <= r (1 - r) d1^2); the addition and the division add u r each.  The floor: where t overflows
    float32, r comes out 0 and the true r is below 1 / FLT_MAX < 2^-126; where t is flushed to 0, r moves by less than 2^-126;
    where the quotient is subnormal it may be flushed.  The three exclude each other: one floor."""
    r = torch.sigmoid(x)
    d1 = torch.expm1(ex) + 2 * E_ULP * U
    return r, r * torch.sigmoid(-x) * d1 * (1 + d1) + 2 * U * r + FLT_MIN


def posnet_ref(out3, H, W, w=DIV_W, b=DIV_B, layout="planar"):
    """PosNet's detection map in float64 with a bound on a float32 kernel's error: (q, bound), both [H, W].

    out3: the network output, planar [3][ldh][ldw] or channels-last [ldh][ldw][3] (``layout``), cropped to H x W here; channel 0 /
    1 = the vector field's row / column component, channel 2 = the mask logit.  g0 = d out3[0] / d row and g1 = d out3[1] / d col
    by ``torch.gradient``'s rule on the H x W crop, q = sigmoid(w * (g0 + g1) * sigmoid(mask) + b).
    The bound follows the sequence g0, g1, div = g0 + g1, s = sigmoid(mask), x = div * s, z = w * x + b, q = sigmoid(z):
    sums and differences carry their operands' errors and add u |result|; a product a * c carries |a| e_c + |c| e_a + e_a e_c
    and adds u |result| + 2^-126."""
    x = _planar64(out3, layout, 3, H, W)
    w, b = float(np.float32(w)), float(np.float32(b))
    g0, e0 = _gradient(x[0], 0)
    g1, e1 = _gradient(x[1], 1)
    div = g0 + g1
    e_div = e0 + e1 + U * div.abs()
    s, e_s = _sigmoid(x[2], torch.zeros_like(x[2]))
    xv = div * s
    e_xv = div.abs() * e_s + s * e_div + e_div * e_s + U * xv.abs() + FLT_MIN
    wx = w * xv
    e_wx = abs(w) * e_xv + U * wx.abs() + FLT_MIN
    z = wx + b
    e_z = e_wx + U * z.abs()
    return _sigmoid(z, e_z)


def shapenet_ref(logits32, H=None, W=None, layout="planar"):
    """One ShapeNet head's marks in float64 with a bound on a float32 kernel's error: (p, bound), both [H, W, 32].

    logits32: planar [32][ldh][ldw] or channels-last [ldh][ldw][32], cropped to H x W here.  p = softmax over the 32 classes.
    The bound follows m = max (exact), d_c = z_c - m (u |d_c|; a d_c of -inf is exact), t_c = expf(d_c) (relative
    expm1(e_d) + 2 E u, plus the floor: a small t_c may be flushed), the sum s in the order csrc/mpp_unet_math.hpp states
    (classes 8 q .. 8 q + 7 in sequence in lane q of four, then lanes 0 + 1 and 2 + 3, then the two pairs: every addition adds
    u times its own result), and p_c = t_c / s (|dp| <= e_t / s + t e_s / s^2 (1 + e_s / s), the division's u p_c, the floor).
    Numerator and denominator are taken as independent: their common error would cancel, so this only widens."""
    z = _planar64(logits32, layout, NCLASS, H, W)
    H, W = z.shape[1:]
    z = z.permute(1, 2, 0).contiguous()
    p = torch.softmax(z, dim=-1)
    d = z - z.max(dim=-1, keepdim=True).values
    e_d = torch.where(torch.isinf(d), torch.zeros_like(d), U * d.abs())
    t = torch.exp(d)
    e_t = t * (torch.expm1(e_d) + 2 * E_ULP * U) + FLT_MIN
    part = t.reshape(H, W, 4, 8).cumsum(dim=-1)                             # a lane's partial sums (the first is no addition)
    e_lane = e_t.reshape(H, W, 4, 8).sum(dim=-1) + U * part[..., 1:].sum(dim=-1)
    lane = part[..., -1]
    pair = lane[..., 0::2] + lane[..., 1::2]
    e_pair = e_lane[..., 0::2] + e_lane[..., 1::2] + U * pair
    s = pair.sum(dim=-1, keepdim=True)
    e_s = e_pair.sum(dim=-1, keepdim=True) + U * s
    return p, e_t / s + t * e_s / s ** 2 * (1 + e_s / s) + U * p + FLT_MIN


def worst_ratio(got, ref, bound):
    """max of |got - ref| / bound; NaN (a store that never happened, or a NaN where the reference is finite) counts as infinite"""
    r = (torch.as_tensor(got).detach().cpu().double() - ref).abs() / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


def count_over(got, ref, bound):
    """number of outputs that are not within the bound (NaN included)"""
    return int(((torch.as_tensor(got).detach().cpu().double() - ref).abs() <= bound).logical_not().sum())


def bf16_round(x):
    """float32 array -> the float32 values of its bfloat16 rounding (to nearest, ties to even); finite inputs"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def bf16_truncate(x):
    """the wrong conversion: the low 16 bits dropped"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


# ---- numpy float32 restatements of the epilogues (the float32 stand-ins of the host test, and its wrong kernels) ----------------
def expf(a):
    """numpy's float32 exp"""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(a, dtype=np.float32))


def exp_ulp_error(args):
    """worst error of ``expf`` against float64 over the float32 arguments, in ulp of the true value, over those whose true
    result is a normal float32"""
    a = np.asarray(args, dtype=np.float32)
    a = a[np.isfinite(a)]
    true = np.exp(a.astype(np.float64))
    ok = (true >= FLT_MIN) & (true < 2.0 ** 128)
    a, true = a[ok], true[ok]
    if a.size == 0:
        return 0.0
    ulp = 2.0 ** (np.floor(np.log2(true)) - 23)
    return float((np.abs(expf(a).astype(np.float64) - true) / ulp).max())


F1, F2 = np.float32(1), np.float32(2)


def _sigm32(x, exp):
    with np.errstate(over="ignore", under="ignore"):
        return F1 / (F1 + exp(-x))


def _grad32(v, axis, wrong):
    """torch.gradient's rule along ``axis`` in float32; wrong: "no half" / "one-sided inside" """
    v = np.moveaxis(v, axis, 0)
    n = v.shape[0]
    g = np.zeros_like(v)
    if n > 1:
        g[0], g[-1] = v[1] - v[0], v[-1] - v[-2]
        if n > 2:
            d = v[2:] - v[:-2]
            g[1:-1] = d if wrong == "no half" else d / F2
            if wrong == "one-sided inside":
                g[1] = v[2] - v[1]
                g[-2] = v[-2] - v[-3]
    return np.moveaxis(g, 0, axis)


#: wrong PosNet epilogues
POS_MUTANTS = ["no half", "one-sided inside", "g0 along columns", "vectors swapped", "no mask sigmoid"]
#: wrong ShapeNet epilogues ("no max" has to fail on the saturated families)
SHP_MUTANTS = ["no max", "groups swapped", "sum over 8", "left neighbour"]


def posnet_f32(x, H, W, w=DIV_W, b=DIV_B, wrong=None, exp=expf):
    """the PosNet epilogue in numpy float32, operation by operation; x [3, ldh, ldw] float32; ``wrong`` names a mutant"""
    x = np.asarray(x, dtype=np.float32)[:, :H, :W]
    w, b = np.float32(w), np.float32(b)
    v0, v1, mk = (x[1], x[0], x[2]) if wrong == "vectors swapped" else (x[0], x[1], x[2])
    g0 = _grad32(v0, 1 if wrong == "g0 along columns" else 0, wrong)
    g1 = _grad32(v1, 1, wrong)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        div = g0 + g1
        s = F1 if wrong == "no mask sigmoid" else _sigm32(mk, exp)
        q = _sigm32(w * (div * s) + b, exp)
    assert q.dtype == np.float32
    return q


def shapenet_f32(z, H, W, wrong=None, exp=expf):
    """the ShapeNet epilogue in numpy float32; z [32, ldh, ldw] float32 -> [H, W, 32]; the sum in the order of
    ``softmax_quad`` (csrc/mpp_unet_math.hpp); ``wrong`` names a mutant"""
    v = np.ascontiguousarray(np.asarray(z, dtype=np.float32)[:, :H, :W].transpose(1, 2, 0))
    if wrong == "left neighbour":
        v[:, 1:] = v[:, :-1].copy()
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        m = np.float32(0) if wrong == "no max" else v.max(axis=-1, keepdims=True)
        t = exp(v - m).reshape(H, W, 4, 8)
        lane = t[..., 0]
        for i in range(1, 8):
            lane = lane + t[..., i]
        if wrong == "sum over 8":
            s = lane[..., None]
        else:
            s = ((lane[..., 0] + lane[..., 1]) + (lane[..., 2] + lane[..., 3]))[..., None, None]
        p = (t / s).reshape(H, W, NCLASS)
    if wrong == "groups swapped":
        p = np.concatenate([p[..., 8:16], p[..., 0:8], p[..., 16:]], axis=-1)
    assert p.dtype == np.float32
    return p


# ---- the launchers' work split, restated from csrc/mpp_maps.hip (the tests assert conditions on it) ----------------------------
def pos_planar_grid(wh, ww):
    """k_posnet_epilogue: 256 threads of 4 pixels per workgroup along a window row, one grid row per window row"""
    return -(-ww // 1024), wh


def pos_planar_vec_ok(ldh, ldw, wy0, ld_dst, src_addr, dst_addr):
    """the launcher's condition for 16-byte accesses"""
    return ldw % 4 == 0 and wy0 % 4 == 0 and ld_dst % 4 == 0 and src_addr % 16 == 0 and dst_addr % 16 == 0 and (ldh * ldw) % 4 == 0


def pos_planar_vector_threads(H, W, wx0, wy0, wh, ww, vec_ok):
    """[(r, j4)] of the threads of k_posnet_epilogue that take the 16-byte path: four interior pixels of an interior row"""
    out = []
    for r in range(wh):
        for j4 in range(0, ww, 4):
            x, y4 = wx0 + r, wy0 + j4
            if vec_ok and 0 < x < H - 1 and y4 > 0 and y4 + 4 < W and j4 + 4 <= ww:
                out.append((r, j4))
    return out


def shp_planar_grid(wh, ww):
    """k_shapenet_epilogue: one workgroup per 64 pixels of a window row"""
    return -(-ww // WAVE), wh


def shp_planar_vec_ok(ldh, ldw, wy0, src_addr):
    return ldw % 4 == 0 and wy0 % 4 == 0 and src_addr % 16 == 0 and (ldh * ldw) % 4 == 0


def shp_planar_vector_blocks(ww, vec_ok):
    """x indices of the workgroups of a row that load with 16-byte accesses: whole blocks of 64 pixels"""
    return [bx for bx in range(-(-ww // WAVE)) if vec_ok and bx * WAVE + WAVE <= ww]


def pos_nhwc_grid(wh, ww):
    """k_posnet_epilogue_nhwc: one thread per pixel, 256 per workgroup along a window row"""
    return -(-ww // 256), wh


def shp_nhwc_grid(wh, ww):
    """k_shapenet_epilogue_nhwc: four lanes per pixel over the window's pixels in row-major order, 256 lanes per workgroup"""
    return -(-(wh * ww * 4) // 256)


def shp_nhwc_live_pixels_per_wave(wh, ww):
    """live pixels (of 16) of every wave the launch starts"""
    n = wh * ww
    return [max(0, min(16, n - 16 * k)) for k in range(4 * shp_nhwc_grid(wh, ww))]


# ---- cases: the smallest shapes at which each mechanism exists -------------------------------------------------------------------
#: planar PosNet: the crop, the source's pitch, the destination's row pitch, and floats the source view starts off its storage
PosPlanar = collections.namedtuple("PosPlanar", "H W ldh ldw ld_dst src_off")
POS_PLANAR_CASES = [
    PosPlanar(1, 1, 8, 8, 1, 0),          # both axes of length 1: the divergence is 0 by grad1's n == 1 rule
    PosPlanar(1, 7, 8, 8, 7, 0),          # one row: g0 = 0, g1 one-sided at both ends; two threads, the second with 3 pixels
    PosPlanar(3, 1, 8, 8, 1, 0),          # one column: g1 = 0
    PosPlanar(2, 2, 8, 8, 2, 0),          # no central difference anywhere
    PosPlanar(2, 9, 8, 16, 12, 0),        # aligned and wide enough, but no interior row: scalar
    PosPlanar(3, 8, 8, 8, 8, 0),          # aligned, but no thread qualifies: j4 = 0 has y4 = 0, j4 = 4 has y4 + 4 = W
    PosPlanar(3, 9, 8, 16, 12, 0),        # exactly one vector thread: (r, j4) = (1, 4); its right neighbour is the last column
    PosPlanar(3, 12, 8, 16, 12, 0),       # one vector thread; j4 = 8 holds four pixels but ends on the border: scalar
    PosPlanar(3, 13, 8, 16, 16, 0),       # two vector threads and a one-pixel scalar tail
    PosPlanar(3, 13, 8, 13, 16, 0),       # an odd pitch: the scalar path everywhere
    PosPlanar(5, 1029, 8, 1032, 1032, 0),  # the second x-workgroup (ww > 1024): one vector thread and a one-pixel thread, 5 pixels
    PosPlanar(3, 13, 8, 16, 16, 1),       # the source view starts 4 bytes off a 16-byte boundary: scalar everywhere
]
#: what the comments above claim: vector threads per case (asserted from pos_planar_vector_threads on an aligned base)
POS_PLANAR_VECTOR_THREADS = [0, 0, 0, 0, 0, 0, 1, 1, 2, 0, 3 * 256, 0]

#: planar ShapeNet (H, W, ldh, ldw): below, at and above one and two 64-pixel blocks; the last has an odd pitch (scalar loads)
SHP_PLANAR_CASES = [(H, W, 8, -(-W // 8) * 8) for H in (1, 2) for W in (1, 63, 64, 65, 128, 129)] + [(2, 65, 8, 65)]

#: channels-last PosNet (H, W, ldh, ldw): around the 256-thread workgroup; single row, single column; dense and pitched sources
POS_NHWC_CASES = [(3, 1, 3, 1), (3, 2, 4, 5), (3, 255, 3, 255), (3, 256, 3, 256), (3, 257, 4, 260), (1, 5, 1, 5), (5, 1, 6, 2)]

#: channels-last ShapeNet (H, W, ldh, ldw): 1, 15, 16, 17, 63, 64, 65 pixels -- partially live waves of 16 pixels and the edge of the
#: 64-pixel workgroup; in (3, 5), (7, 9) and (5, 13) a row ends inside a wave
SHP_NHWC_CASES = [(1, 1, 1, 1), (3, 5, 3, 5), (2, 8, 3, 9), (1, 17, 1, 17), (7, 9, 8, 12), (8, 8, 8, 8), (5, 13, 5, 16)]

#: one window with odd wx0, wy0 for all four kernels: (H, W, ldh, ldw, wx0, wy0, wh, ww); two 64-pixel blocks per row
WINDOW = (7, 75, 8, 80, 1, 3, 5, 70)

POS_FAMILIES = ["benign", "sat mask", "sat field", "sat constant", "neg zero"]
SHP_FAMILIES = ["benign", "sat wide", "sat dominant", "sat tie", "sat equal", "sat group 0", "sat group 1", "sat group 2",
                "sat group 3", "neg inf", "neg zero"]


def family_group(name):
    """benign / saturated / special: the issue's three families"""
    return "benign" if name == "benign" else ("saturated" if name.startswith("sat ") else "special")


@functools.lru_cache(maxsize=None)
def pos_inputs(family, ldh, ldw):
    """[3, ldh, ldw] float32 (never modified): the whole pitched buffer holds data of the family"""
    g = torch.Generator().manual_seed(100003 * POS_FAMILIES.index(family) + 1031 * ldh + ldw)
    x = torch.randn((3, ldh, ldw), generator=g)
    if family == "sat mask":                      # mask logits of +-20 and +-100: sigmoid(mask) at both ends, expf(100) overflows
        lv = torch.tensor([20.0, -20.0, 100.0, -100.0])
        x[2] = lv[torch.randint(0, 4, (ldh, ldw), generator=g)]
    elif family == "sat field":                   # |w x + b| reaches about 200 (w = -10.8): the outer expf over- and underflows
        x[:2] *= 8.0
        x[2] += 3.0
    elif family == "sat constant":                # a constant field: the divergence is exactly 0, every output is sigmoid(b)
        x[0], x[1] = 1.25, -3.5
        x[2] *= 2.0
    elif family == "neg zero":                    # -0.0 among the vectors, a mask logit of -0.0 everywhere (sigmoid = 0.5)
        x[:2] = torch.where(torch.rand((2, ldh, ldw), generator=g) < 0.3, torch.tensor(-0.0), x[:2])
        x[2] = -0.0
    return x


@functools.lru_cache(maxsize=None)
def shp_inputs(family, ldh, ldw):
    """[32, ldh, ldw] float32 (never modified)"""
    g = torch.Generator().manual_seed(100003 * SHP_FAMILIES.index(family) + 1031 * ldh + ldw + 7)
    z = 3.0 * torch.randn((NCLASS, ldh, ldw), generator=g)
    pick = torch.randint(0, NCLASS, (1, ldh, ldw), generator=g)
    if family == "sat wide":                      # 40 * randn: nearly half of the expf(v - m) underflow float32
        z = z * (40.0 / 3.0)
    elif family == "sat dominant":                # one class 90 above the rest: expf(-90) is subnormal, p is 1 and 31 zeros
        z = (z / 3.0).scatter_add(0, pick, torch.full((1, ldh, ldw), 90.0))
    elif family == "sat tie":                     # two exactly equal maxima
        top = z.max(dim=0, keepdim=True).values + 2.5
        other = (pick + torch.randint(1, NCLASS, (1, ldh, ldw), generator=g)) % NCLASS
        z = z.scatter(0, pick, top).scatter(0, other, top)
    elif family == "sat equal":                   # all 32 equal: every p is 1/32
        z = (5.0 * torch.randn((1, ldh, ldw), generator=g)).expand(NCLASS, ldh, ldw).contiguous()
    elif family.startswith("sat group"):          # the maximum in lane q's eight classes: the quad's max and sum must travel
        q = int(family[-1])
        z = z.scatter_add(0, 8 * q + pick % 8, torch.full((1, ldh, ldw), 30.0))
    elif family == "neg inf":                     # some classes -inf (never all of a pixel); pixel (0, 0) keeps one class only
        dead = torch.rand((NCLASS, ldh, ldw), generator=g) < 0.4
        dead.scatter_(0, pick, torch.zeros((1, ldh, ldw), dtype=torch.bool))
        dead[:, 0, 0] = True
        dead[5, 0, 0] = False
        z = torch.where(dead, torch.tensor(float("-inf")), z)
    elif family == "neg zero":                    # zeros of both signs: every p is 1/32
        z = torch.where(torch.rand((NCLASS, ldh, ldw), generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    return z


def as_dtype(x, dtype):
    """the values a kernel of that input type sees, as float32: x itself, or its bfloat16 rounding"""
    return x if dtype == torch.float32 else x.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def pos_case(family, H, W, ldh, ldw, dtype=torch.float32):
    """(inputs as float32 values [3, ldh, ldw], reference, bound); computed once per process, never modified"""
    x = as_dtype(pos_inputs(family, ldh, ldw), dtype)
    return (x,) + posnet_ref(x, H, W)


@functools.lru_cache(maxsize=None)
def shp_case(family, H, W, ldh, ldw, dtype=torch.float32):
    z = as_dtype(shp_inputs(family, ldh, ldw), dtype)
    return (z,) + shapenet_ref(z, H, W)
