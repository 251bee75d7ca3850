"""Float64 references of the three kernels of csrc/mpp_conv.hip (``k_conv3x3_c32``, ``k_conv3x3_stem``, ``k_shapenet_heads``,
the whole crop and windows of it) with an error bound per output that is derived from the float32 format, not measured.  Plain torch
on the CPU; nothing of the library is imported.  tests/test_unet_conv_ref_host.py shows that the bounds hold for a
float32 stand-in and that wrong kernels break them; tests/test_gpu_unet_conv_float64.py holds the kernels to them.

Notation: u = 2^-24, the unit roundoff of float32 (a correctly rounded operation errs by at most u / (1 + u) relative to its
exact result); K = the number of products of one output; |.| elementwise; conv(a, b) = F.conv2d(F.pad(a, reflect), b)."""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126

#: grid cap of mpp_launch_shapenet_heads (workgroups of four waves, one group of 32 pixels per wave and iteration)
HEADS_MAX_GRID = 2048
#: output tile of a k_conv3x3_c32 workgroup
CV_ROWS, CV_COLS = 8, 64


# ---- weight layouts: what unet.ScoreMapNets hands the kernels ----------------------------------------------------------
def pack_c32(w):
    """[32, C_in, 3, 3] -> [C_in / 32][kh * 3 + kw][32 in][32 out]: ``ScoreMapNets._packed``"""
    w = w.detach().float()
    cin = w.shape[1]
    return w.permute(2, 3, 1, 0).reshape(9, cin // 32, 32, 32).permute(1, 0, 2, 3).contiguous()


def pack_stem(w):
    """[32, 3, 3, 3] -> [kh * 3 + kw][3 in][32 out]: the stem's block of ``ScoreMapNets._double_conv_nhwc``"""
    return w.detach().float().permute(2, 3, 1, 0).reshape(9, 3, 32).contiguous()


def pack_heads(ws, bs):
    """three [32, 32, 1, 1] weights and three [32] biases -> ([3, 32 class, 32 in], [3, 32]): ``ScoreMapNets._packed_heads``"""
    w = torch.stack([x.detach().float().reshape(32, 32) for x in ws]).contiguous()
    b = torch.stack([x.detach().float() for x in bs]).contiguous()
    return w, b


# ---- the launchers' work split, restated (the tests assert conditions on it) ------------------------------------------------
def c32_tiles(H, W):
    """(tiles_x, tiles_y) of k_conv3x3_c32"""
    return -(-W // CV_COLS), -(-H // CV_ROWS)


def c32_grid(n_tiles, cus):
    """workgroups mpp_launch_conv3x3_c32 starts on a device of ``cus`` compute units"""
    return max(8, min((cus // 8) * 8, -(-n_tiles // 8) * 8))


def c32_ranges(n_tiles, grid):
    """[(t_begin, t_end)] per workgroup id: workgroup (xcd = id % 8, k = id / 8) takes the k-th share of the xcd-th eighth"""
    per = grid // 8
    out = []
    for b in range(grid):
        xcd, k = b % 8, b // 8
        e0, e1 = n_tiles * xcd // 8, n_tiles * (xcd + 1) // 8
        out.append((e0 + (e1 - e0) * k // per, e0 + (e1 - e0) * (k + 1) // per))
    return out


def heads_groups(H, W):
    """groups of 32 pixels of a row: what a wave of k_shapenet_heads takes per iteration"""
    return -(-W // 32) * H


# ---- references -----------------------------------------------------------------------------------------------------------------
def _f64(t):
    return None if t is None else t.detach().cpu().double()


def _conv(x, w):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w)


def _epilogue(acc, acc_err, out_scale, out_shift, relu):
    """value and bound after y = acc * out_scale + out_shift (and ReLU); acc_err = the bound on the accumulator"""
    if out_scale is None:
        y, bound = acc, acc_err                         # (the kernel multiplies by 1.f and adds 0.f: exact)
    else:
        s, t = out_scale.view(1, -1, 1, 1), out_shift.view(1, -1, 1, 1)
        y = acc * s + t
        bound = acc_err * s.abs() + 2 * U * y.abs() + U * t.abs()
    return (torch.relu(y) if relu else y), bound


def conv3x3_c32_ref(x, w, in_scale=None, in_shift=None, out_scale=None, out_shift=None, relu=True):
    """Conv2d(C_in -> 32, 3x3, reflect) as ``mpp_conv3x3_c32`` defines it, in float64, with a bound on a float32 kernel's error.

    x [1, C_in, H, W] and w [32, C_in, 3, 3] hold float32 values.  x_in = x, except that channels 0..31 are
    max(0, x * in_scale + in_shift) when the in-load affine is given (the second source of a concat arrives finished);
    acc = conv(x_in, w); y = acc * out_scale + out_shift when given; ReLU when asked.  Returns (y, bound), both float64
    [1, 32, H, W]; a float32 kernel that rounds every operation correctly satisfies |got - y| <= bound for ANY order of
    the sum, with or without fused multiply-adds.  Derivation, K = 9 * C_in:

    1. Accumulation.  A float32 sum of K products s = sum a_k b_k, products rounded or fused, in any order, has
       |fl(s) - s| <= gamma_K * sum |a_k b_k| with gamma_K = K u / (1 - K u) (Higham, Accuracy and Stability, 3.1 / 3.5).  The
       bound uses (K + 2) u: for K <= 576, K u / (1 - K u) <= K u + 3.5e-5 * K u, so 2 u of slack per output remain, and they
       absorb every second-order term below (each is at most a few K u^2 * conv(|x_in|, |w|), i.e. < 1e-4 of that slack).
       => (K + 2) u * conv(|x_in|, |w|).
    2. The in-load affine on channels 0..31: t = fl(fl(x s) + b) or one fma.  With the u / (1 + u) form of the rounding
       error, |t - (x s + b)| <= 2 u |x s| + u |b| <= 2 u (|x s| + |b|); max(0, .) is 1-Lipschitz and exact.  The
       convolution carries that input error to the output as conv(2 u (|x s| + |b|), |w|) (zero on channels 32..63).
    3. Both are errors of the accumulator; the epilogue multiplies them by |out_scale|.
    4. The epilogue itself, v = fl(fl(acc s) + t) or one fma: |v - (acc s + t)| <= u |acc s| + u |acc s + t|
       <= 2 u |y| + u |t| with y = acc s + t BEFORE the ReLU (a y of -1e-9 may come out as +1e-8: the ReLU cannot shrink the
       bound to 0 there).  Without an epilogue the kernel multiplies by 1 and adds 0, which is exact: no term.
    Subnormals play no part at the magnitudes of the tests (|products| > 1e-30 wherever they matter)."""
    x, w = _f64(x), _f64(w)
    in_scale, in_shift, out_scale, out_shift = _f64(in_scale), _f64(in_shift), _f64(out_scale), _f64(out_shift)
    cin = w.shape[1]
    K = 9 * cin
    x_in, x_err = x, None
    if in_scale is not None:
        s, t = in_scale.view(1, -1, 1, 1), in_shift.view(1, -1, 1, 1)
        x_in, x_err = x.clone(), torch.zeros_like(x)
        x_in[:, :32] = torch.relu(x[:, :32] * s + t)
        x_err[:, :32] = 2 * U * ((x[:, :32] * s).abs() + t.abs())
    acc = _conv(x_in, w)
    acc_err = (K + 2) * U * _conv(x_in.abs(), w.abs())
    if x_err is not None:
        acc_err = acc_err + _conv(x_err, w.abs())
    return _epilogue(acc, acc_err, out_scale, out_shift, relu)


def stem_ref(x, w, scale, shift):
    """Conv2d(3 -> 32, 3x3, reflect) + scale / shift + ReLU as ``mpp_conv3x3_stem`` defines it: the construction of
    ``conv3x3_c32_ref`` with K = 27 and no in-load affine: bound = (K + 2) u * conv(|x|, |w|) * |scale| + 2 u |y| + u |shift|,
    y before the ReLU.  x [1, 3, H, W], w [32, 3, 3, 3]; returns (value, bound) [1, 32, H, W] float64."""
    x, w = _f64(x), _f64(w)
    acc = _conv(x, w)
    acc_err = (27 + 2) * U * _conv(x.abs(), w.abs())
    return _epilogue(acc, acc_err, _f64(scale), _f64(shift), True)


#: the constant of heads_ref's relative bound, in units of u (see there)
HEADS_C = 48


def heads_ref(h, w, b, H, W):
    """ShapeNet's three 1x1 heads + bias + softmax over the 32 classes as ``mpp_shapenet_heads_win`` defines them.

    h [1, 32, ldh, ldw] (cropped to [H, W]), w [3, 32 class, 32 in], b [3, 32], float32 values.  Returns (logits, prob, bound),
    float64 [3, H, W, 32].  Derivation of the bound on a float32 kernel's probabilities:

    1. Logits: z_c = b_c + sum_k w_ck h_k is a sum of 33 terms (32 products and the bias the accumulator starts from), so
       by the accumulation bound of ``conv3x3_c32_ref`` the kernel's logit z'_c has |z'_c - z_c| <= delta_c =
       33 u (|w_c| . |h| + |b_c|)  (gamma_33 <= 33 u (1 + 2e-6); that excess goes into the rounding-up of the constant).
    2. Softmax is invariant under a common shift, so p_c = exp(z_c - m') / sum_j exp(z_j - m') for the kernel's own maximum
       m' as well.  The kernel forms d_c = fl(z'_c - m') = (z'_c - m')(1 + e), |e| <= u, that is d_c = z_c - m' + eta_c with
       eta_c = a_c + r_c, |a_c| <= delta_c (the logit's error) and |r_c| <= rho_c = u |z'_c - m'| (the subtraction's).
       Numerator: exp(d_c) = exp(z_c - m') exp(eta_c).
       Denominator: sum_j exp(z_j - m') exp(eta_j) = exp(e_D) sum_j exp(z_j - m'), where e_D lies between min_j a_j and
       max_j a_j, widened by at most the p-weighted mean of the |r_j|: u sum_j p_j |z_j - m| (m = max z).
       sum_j p_j (m - z_j) = H(p) - log(sum_j exp(z_j - m)) <= H(p) <= log 32 < 3.5: the subtraction costs the denominator
       at most 3.5 u.
       Together the ratio errs relatively by |eta_c - e_D| <= delta_c + max_j delta_j + rho_c + 3.5 u
       <= 2 * max_c delta_c + u |z_c - max| + 3.5 u.
    3. The constant HEADS_C = 48, in units of u:
         12  two expf results (the numerator's and, as a bound on every term, the sum's), 3 ulp = 6 u each: the accuracy
             OpenCL's full profile requires of exp, of which the device library documents 1 ulp;
         31  a 32-term float32 sum of positive terms in any order (gamma_31);
          1  the division;
          3.5 the subtraction's share of the denominator (above);
          0.5 rounding up, which pays for gamma_33 - 33 u and the use of z for z' in rho_c (both < 1e-3 u).
       rel_c = 2 max delta + u |z_c - max z| + 48 u, and the bound is p_c * expm1(rel_c) (the exact form of "relative error
       rel_c" for an error that sits in an exponent) + 2^-126: below the smallest normal float32 a result may be flushed to
       zero, which a relative bound cannot express."""
    hh = _f64(h)[0, :, :H, :W].permute(1, 2, 0)                               # [H, W, 32 in]
    w, b = _f64(w), _f64(b)
    z = torch.einsum("hwk,nck->nhwc", hh, w) + b.view(3, 1, 1, 32)
    delta = 33 * U * (torch.einsum("hwk,nck->nhwc", hh.abs(), w.abs()) + b.abs().view(3, 1, 1, 32))
    p = torch.softmax(z, dim=-1)
    zmax = z.max(dim=-1, keepdim=True).values
    rel = 2 * delta.max(dim=-1, keepdim=True).values + U * (z - zmax).abs() + HEADS_C * U
    return z, p, p * torch.expm1(rel) + FLT_MIN


# ---- shared cases: the same inputs for the host tests and the GPU tests -------------------------------------------------------
C32_EDGE_SHAPES = [(2, 2), (2, 3), (3, 2), (7, 63), (8, 64), (9, 65), (16, 128), (17, 129)]
C32_BIG = (331, 801)                  # 42 x 13 = 546 ragged tiles: more than two per workgroup on 256 compute units
C32_SHAPES = C32_EDGE_SHAPES + [C32_BIG]
#: (in-load affine, epilogue, relu)
C32_VARIANTS = {"epilogue": (False, True, True), "affine+epilogue": (True, True, True), "raw": (False, False, False)}
STEM_SHAPES = [(2, 2), (2, 17), (16, 16), (17, 33), (331, 801)]
HEADS_SHAPES = [(1, 1, 8, 8), (5, 31, 16, 32), (3, 33, 8, 40), (331, 801, 336, 808)]


@functools.lru_cache(maxsize=4)
def c32_inputs(cin, H, W):
    """x [1, cin, H, W], w [32, cin, 3, 3], in_scale, in_shift, out_scale, out_shift: float32 CPU tensors.  Scales of both
    signs (a negative in_scale sends about half of the inputs to the ReLU's zero)."""
    g = torch.Generator().manual_seed(1000 * cin + 7 * H + W)
    x = torch.randn((1, cin, H, W), generator=g)
    w = torch.randn((32, cin, 3, 3), generator=g) / (3.0 * cin ** 0.5)
    isc = (torch.rand(32, generator=g) + 0.5) * torch.where(torch.arange(32) % 5 == 0, -1.0, 1.0)
    ish = torch.randn(32, generator=g) * 0.3
    osc = (torch.rand(32, generator=g) + 0.5) * torch.where(torch.arange(32) % 7 == 3, -1.0, 1.0)
    osh = torch.randn(32, generator=g) * 0.1
    return x, w, isc, ish, osc, osh


def c32_kwargs(inputs, variant):
    """the scale / shift / relu arguments of a variant, by the names conv3x3_c32_ref and MppContext.conv3x3_c32 share"""
    _, _, isc, ish, osc, osh = inputs
    aff, epi, relu = C32_VARIANTS[variant]
    return dict(in_scale=isc if aff else None, in_shift=ish if aff else None, out_scale=osc if epi else None,
                out_shift=osh if epi else None, relu=relu)


@functools.lru_cache(maxsize=2)
def c32_case(cin, H, W, variant):
    """(inputs, reference, bound) of one conv3x3_c32 case; computed once per process, never modified"""
    inp = c32_inputs(cin, H, W)
    ref, bound = conv3x3_c32_ref(inp[0], inp[1], **c32_kwargs(inp, variant))
    return inp, ref, bound


@functools.lru_cache(maxsize=2)
def stem_case(H, W):
    g = torch.Generator().manual_seed(7 * H + W)
    x = torch.rand((1, 3, H, W), generator=g)
    w = torch.randn((32, 3, 3, 3), generator=g) / 5.0
    sc = (torch.rand(32, generator=g) + 0.5) * torch.where(torch.arange(32) % 6 == 1, -1.0, 1.0)
    sh = torch.randn(32, generator=g) * 0.1
    ref, bound = stem_ref(x, w, sc, sh)
    return (x, w, sc, sh), ref, bound


@functools.lru_cache(maxsize=2)
def heads_case(H, W, ldh, ldw):
    """h is a finished activation (after a ReLU) times 2; logits spread over about +-15"""
    g = torch.Generator().manual_seed(1000 * H + W)
    h = torch.relu(torch.randn((1, 32, ldh, ldw), generator=g)) * 2.0
    ws = [torch.randn((32, 32, 1, 1), generator=g) / 2.0 for _ in range(3)]
    bs = [torch.randn(32, generator=g) for _ in range(3)]
    w, b = pack_heads(ws, bs)
    z, p, bound = heads_ref(h, w, b, H, W)
    return (h, w, b), z, p, bound


def worst_ratio(got, ref, bound):
    """max of |got - ref| / bound; NaN (a store that never happened) counts as infinite"""
    r = (torch.as_tensor(got).double() - ref).abs() / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())
