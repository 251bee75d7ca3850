"""Test helper (no test in here): the training labels and the two fused losses restated with numpy and CPU torch, and the
inputs that tests/test_unet_train_ref_host.py (no GPU) and tests/test_gpu_unet_train_float64.py share.

* ``posnet_labels`` / ``shapenet_labels`` / ``value_classes`` / ``perturbed_classes`` / ``patch_objects``: what
  ``mpp_train_batch`` writes for one patch, by brute force in float64 from the formulas of include/mpp_hip.h and DESIGN.md
  section 8 (nothing here calls the library);
* ``posnet_loss_ref`` / ``shapenet_loss_ref``: ``mpp_posnet_loss`` / ``mpp_shapenet_loss`` through CPU torch autograd;
* ``label_dataset`` ... ``shapenet_loss_case``: the seeded inputs; the references of the label batches are computed once
  per process (``label_reference``, ``cap_reference``) and must not be written to.
"""
import functools

import numpy as np

import unet_augment_ref as A
import unet_train_cases as cases
from mpp_cnn_rs_object_detection_amd import hip_api, shapes
from mpp_cnn_rs_object_detection_amd import unet_training as ut

BAND = hip_api.TRAIN_BAND
MAX_OBJ = hip_api.TRAIN_MAX_OBJ


# ---- labels ----------------------------------------------------------------------------------------------------------------
def nearest(centers, P):
    """integer squared distance of every pixel to its nearest centre, that centre's index (ties: the lowest; -1 without
    centres, measured from the virtual point (-1, 0)) and the number of centres at that distance"""
    c = np.asarray(centers, dtype=np.int64).reshape(-1, 2)
    rr, cc = np.mgrid[:P, :P].astype(np.int64)
    if not len(c):
        return (rr + 1) ** 2 + cc ** 2, np.full((P, P), -1, np.int64), np.zeros((P, P), np.int64)
    d2 = (c[:, 0][:, None, None] - rr) ** 2 + (c[:, 1][:, None, None] - cc) ** 2
    best = d2.min(0)
    return best, np.argmax(d2 == best, axis=0), (d2 == best).sum(0)


def posnet_labels(centers, P, uvec, max_distance, sigma_dil):
    """dist, dil, vec [2,P,P], mask of one patch (centres in patch coordinates, annotation order), float32"""
    c = np.asarray(centers, dtype=np.int64).reshape(-1, 2)
    d2, arg, _ = nearest(c, P)
    dist = np.sqrt(d2.astype(np.float64))
    t = dist / float(sigma_dil)
    dil = np.exp(-0.5 * (t * t))
    dil[dil < 1e-5] = 0.0
    vec = np.zeros((2, P, P))
    mask = np.zeros((P, P))
    if len(c):
        rr, cc = np.mgrid[:P, :P]
        v = np.stack([c[arg, 0] - rr, c[arg, 1] - cc]).astype(np.float64)
        norm = np.sqrt(v[0] * v[0] + v[1] * v[1]) + 1e-8
        if uvec:
            v = v / norm
        inside = ~(norm > float(max_distance))
        vec = np.where(inside, v, 0.0)
        mask = inside.astype(np.float64)
    return dist.astype(np.float32), dil.astype(np.float32), vec.astype(np.float32), mask.astype(np.float32)


def shapenet_labels(centers, params, classes, P):
    """cls [3,P,P] uint8, cover [P,P] uint8 of one patch, and the smallest |x - x_crossing| over all (pixel, edge) pairs
    that pass the row test (inf: none).  classes [n,3]: the three classes of every object."""
    c = np.asarray(centers, dtype=np.float64).reshape(-1, 2)
    p = np.asarray(params, dtype=np.float64).reshape(-1, 3)
    cls = np.zeros((3, P, P), np.uint8)
    cover = np.zeros((P, P), np.uint8)
    margin = np.inf
    for k in range(len(c)):
        poly = shapes.rect_to_poly(c[k], short=p[k, 0], long=p[k, 1], angle=p[k, 2])
        pr, pc = poly[:, 0], poly[:, 1]
        r0, r1 = int(max(0.0, pr.min())), min(int(np.ceil(pr.max())), P - 1)
        c0, c1 = int(max(0.0, pc.min())), min(int(np.ceil(pc.max())), P - 1)
        if r0 > r1 or c0 > c1:
            continue
        y, x = np.mgrid[r0:r1 + 1, c0:c1 + 1].astype(np.float64)
        inside = np.zeros(y.shape, bool)
        q = 3
        for e in range(4):
            ye, yq, xe, xj = pr[e], pr[q], pc[e], pc[q]
            rows = ((ye <= y) & (y < yq)) | ((yq <= y) & (y < ye))
            with np.errstate(divide="ignore", invalid="ignore"):
                xc = (xj - xe) * (y - ye) / (yq - ye) + xe
            if rows.any():
                margin = min(margin, float(np.abs(x - xc)[rows].min()))
            inside ^= rows & (x < np.where(rows, xc, -np.inf))
            q = e
        cover[r0:r1 + 1, c0:c1 + 1][inside] = 1
        for m in range(3):
            cls[m, r0:r1 + 1, c0:c1 + 1][inside] = classes[k][m]
    return cls, cover, margin


def value_classes(params, edges):
    """[n,3] plain classes of (a, b, angle) rows: size (a + b) / 2, ratio a / b, angle; the last lower bin edge the value
    reaches (class 0 below the first)"""
    p = np.asarray(params, dtype=np.float64).reshape(-1, 3)
    v = np.stack([(p[:, 0] + p[:, 1]) / 2, p[:, 0] / p[:, 1], p[:, 2]], 1)
    out = np.zeros((len(p), 3), np.int64)
    for m in range(3):
        e = np.asarray(edges[m], dtype=np.float64)
        out[:, m] = np.maximum((e[None, :] <= v[:, m][:, None]).sum(1) - 1, 0)
    return out


def perturbation_draws(rows, seed, epoch, batch, patch):
    """[n,3] in {0, +1, -1}: u < 0.8, u < 0.9, else, from words 0..2 of Philox stream 1 at index = the object's table row"""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    ctr = np.stack([np.full_like(rows, batch), np.full_like(rows, patch), np.ones_like(rows), rows], 1)
    u = A.unif(A.philox_many(ctr, (seed, epoch)))[:, :3]
    return np.where(u < 0.8, 0, np.where(u < 0.9, 1, -1)).astype(np.int64)


def perturbed_classes(params, edges, cyclic, rows, seed, epoch, batch, patch):
    """[n,3] classes under MPP_AUG_PERTURB: plain class + draw, wrapped (cyclic mark) or clamped to 0 .. n_classes - 1"""
    n = len(edges[0])
    cl = value_classes(params, edges) + perturbation_draws(rows, seed, epoch, batch, patch)
    for m in range(3):
        cl[:, m] = (cl[:, m] + n) % n if cyclic[m] else np.clip(cl[:, m], 0, n - 1)
    return cl


def patch_objects(centers_of_image, anchor, P):
    """the rows (indices into the image's annotation list, ascending) with anchor - P/2 <= centre < anchor - P/2 + P"""
    c = np.asarray(centers_of_image, dtype=np.int64).reshape(-1, 2)
    tl = np.asarray(anchor, dtype=np.int64) - P // 2
    keep = np.all((c >= tl) & (c < tl + P), axis=1)
    return np.nonzero(keep)[0]


def band_sums(mask, dil=None):
    """[B, nb, 2] float64 as mpp_train_batch writes them: per band of 16 rows the count of mask (cover) pixels and the sum
    of the float32 dil map"""
    B, P = mask.shape[0], mask.shape[-1]
    nb = (P + BAND - 1) // BAND
    out = np.zeros((B, nb, 2))
    for q in range(nb):
        out[:, q, 0] = np.asarray(mask, dtype=np.float64)[:, q * BAND:(q + 1) * BAND].sum((1, 2))
        if dil is not None:
            out[:, q, 1] = np.asarray(dil, dtype=np.float64)[:, q * BAND:(q + 1) * BAND].sum((1, 2))
    return out


# ---- the PosNet loss --------------------------------------------------------------------------------------------------------
def _mixed_ops():
    """float32 forward, float64 backward: the ops of mode "mixed" that the kernel forms in float32.  Every tensor that
    passes between them is float64 and holds float32 values, so ``.float()`` is exact."""
    import torch

    class Sigmoid(torch.autograd.Function):      # y = sigmoid(x) in float32; dy/dx = y * (1 - y) with 1 - y in float32
        @staticmethod
        def forward(ctx, x):
            y = torch.sigmoid(x.float())
            ctx.save_for_backward(y)
            return y.double()

        @staticmethod
        def backward(ctx, g):
            y, = ctx.saved_tensors
            return g * y.double() * (1.0 - y).double()

    class Div(torch.autograd.Function):          # torch.gradient along rows of a + along columns of b, in float32
        @staticmethod
        def forward(ctx, a, b):
            return (torch.gradient(a.float(), dim=1)[0] + torch.gradient(b.float(), dim=2)[0]).double()

        @staticmethod
        def backward(ctx, g):                    # the stencils are linear: their adjoint, in float64
            with torch.enable_grad():
                a = torch.zeros_like(g, requires_grad=True)
                b = torch.zeros_like(g, requires_grad=True)
                d = torch.gradient(a, dim=1)[0] + torch.gradient(b, dim=2)[0]
                return torch.autograd.grad(d, (a, b), g)

    class Mul(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b):
            ctx.save_for_backward(a, b)
            return (a.float() * b.float()).double()

        @staticmethod
        def backward(ctx, g):
            a, b = ctx.saved_tensors
            return g * b, g * a

    class Affine(torch.autograd.Function):       # z = w x + b, two float32 roundings
        @staticmethod
        def forward(ctx, x, w, b):
            ctx.save_for_backward(x, w)
            return (w.float() * x.float() + b.float()).double()

        @staticmethod
        def backward(ctx, g):
            x, w = ctx.saved_tensors
            return g * w, (g * x).sum().reshape(w.shape), g.sum().reshape(w.shape)

    class PlusEps(torch.autograd.Function):      # y + eps, or (1 - y) + eps, in float32
        @staticmethod
        def forward(ctx, y, complement):
            ctx.sign = -1.0 if complement else 1.0
            y = y.float()
            return (((1.0 - y) if complement else y) + 1e-5).double()

        @staticmethod
        def backward(ctx, g):
            return ctx.sign * g, None

    return Sigmoid.apply, Div.apply, Mul.apply, Affine.apply, PlusEps.apply


def _posnet_loss_f32(out, vec, mask, dil, w, b):
    """the plain float32 statement (PointingVectorLoss with the shipped options + the divergence classifier's term)"""
    import torch
    eps = 1e-5
    s = torch.sigmoid(out[:, 2])
    prod = out[:, :2] * torch.stack([s, s], 1)
    vec_loss = torch.mean(torch.square(prod - vec))
    beta = 1 - torch.sum(mask) / mask.numel()
    mask_loss = torch.mean(-beta * mask * torch.log(s + eps) - (1 - beta) * (1 - mask) * torch.log(1 - s + eps))
    div_loss = torch.zeros((), dtype=out.dtype)
    if w is not None:
        div = torch.gradient(out[:, 0], dim=1)[0] + torch.gradient(out[:, 1], dim=2)[0]
        q = torch.sigmoid(w.reshape(()) * (div * s) + b.reshape(()))
        beta_d = 1 - torch.sum(dil) / dil.numel()
        div_loss = torch.mean(-beta_d * dil * torch.log(q + eps) - (1 - beta_d) * (1 - dil) * torch.log(1 - q + eps))
    return vec_loss, mask_loss, div_loss


def _posnet_loss_mixed(out, vec, mask, dil, w, b):
    """what csrc/mpp_train.hip documents: sigmoid(out[2]), the divergence, x = div * s, z = w x + b, q = sigmoid(z) and the
    + eps arguments of the logs in float32, the rest and every sum in float64, beta = 1 - float32(sum(target)) / N"""
    import torch
    sigmoid, divergence, mul, affine, plus_eps = _mixed_ops()
    o = out.double()
    vec, mask, dil = vec.double(), mask.double(), dil.double()
    N = float(mask.numel())

    def bce(y, t):
        beta = 1.0 - float(np.float32(float(t.sum()))) / N
        return torch.sum(-beta * t * torch.log(plus_eps(y, False)) - (1.0 - beta) * (1.0 - t) * torch.log(plus_eps(y, True))) / N

    s = sigmoid(o[:, 2])
    e = o[:, :2] * s[:, None] - vec
    vec_loss = torch.sum(e * e) / (2.0 * N)
    mask_loss = bce(s, mask)
    div_loss = torch.zeros((), dtype=torch.float64)
    if w is not None:
        x = mul(divergence(o[:, 0], o[:, 1]), s)
        div_loss = bce(sigmoid(affine(x, w.double().reshape(()), b.double().reshape(()))), dil)
    return vec_loss, mask_loss, div_loss


def posnet_loss_ref(out, vec, mask, dil, w, b, mode):
    """``mpp_posnet_loss`` through CPU torch autograd.  out [B,3,P,P], vec [B,2,P,P], mask / dil [B,P,P] float32 arrays; w, b
    floats (None, None: the val form, without the divergence term).  mode "f32": plain float32, what a training framework
    runs; "mixed": the kernel's documented statement.  -> dict: vec_loss, mask_loss, div_loss, loss (float), grad
    [B,3,P,P] float64, dw, db (float; 0 in the val form)"""
    import torch
    fn = {"f32": _posnet_loss_f32, "mixed": _posnet_loss_mixed}[mode]
    leaf = torch.float32 if mode == "f32" else torch.float64          # (float64 leaves hold the float32 values)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
    o = t(out).to(leaf).requires_grad_(True)
    wt = bt = None
    if w is not None:
        wt = torch.tensor([w], dtype=torch.float32).to(leaf).requires_grad_(True)
        bt = torch.tensor([b], dtype=torch.float32).to(leaf).requires_grad_(True)
    vl, ml, dl = fn(o, t(vec), t(mask), t(dil), wt, bt)
    loss = vl + ml + dl
    loss.backward()
    vl, ml, dl, loss = (float(v.detach()) for v in (vl, ml, dl, loss))
    return {"vec_loss": vl, "mask_loss": ml, "div_loss": dl, "loss": loss,
            "grad": o.grad.double().numpy(), "dw": float(wt.grad) if w is not None else 0.0,
            "db": float(bt.grad) if w is not None else 0.0}


# ---- the ShapeNet loss -----------------------------------------------------------------------------------------------------
def shapenet_loss_ref(logits, cls, cover):
    """``mpp_shapenet_loss`` in float64: per head the cross-entropy times cover / count (0 for an empty patch), summed over
    the pixels, divided by B.  logits three [B,n,P,P], cls [3,B,P,P], cover [B,P,P] -> dict: feat [3], loss, grads (three
    float64 arrays)"""
    import torch
    cov = torch.from_numpy(np.asarray(cover).astype(np.float64))
    B = cov.shape[0]
    cnt = cov.sum((1, 2), keepdim=True)
    wgt = torch.where(cnt > 0, cov / torch.clamp(cnt, min=1.0), torch.zeros_like(cov))
    xs = [torch.from_numpy(np.asarray(x).astype(np.float64)).requires_grad_(True) for x in logits]
    feat = []
    for h, x in enumerate(xs):
        y = torch.from_numpy(np.asarray(cls[h]).astype(np.int64))
        ce = torch.logsumexp(x, dim=1) - torch.gather(x, 1, y[:, None])[:, 0]
        feat.append(torch.sum(ce * wgt) / B)
    loss = feat[0] + feat[1] + feat[2]
    loss.backward()
    return {"feat": [float(f.detach()) for f in feat], "loss": float(loss.detach()), "grads": [x.grad.numpy() for x in xs]}


# ---- inputs: the label batches ---------------------------------------------------------------------------------------------
LABEL_P = 48
LABEL_SEED, GEO_SEED = 1, 17
POS_VARIANTS = {"uvec8": (1, 8.0, 0.6), "vec5.5": (0, 5.5, 2.5), "md0": (1, 0.0, 0.6)}   # uvec, max_distance, sigma_dil
SHAPE_N, SHAPE_MAX = 32, 32.0                            # n_classes and size_mapping_max of the label batches
# (image, anchor row, anchor col): interior of A, its four corners, wholly outside A, B (no object), interior and a corner
# of C, no image
LABEL_ROWS = [(0, 80, 100), (0, 0, 0), (0, 160, 200), (0, 3, 199), (0, 157, 2), (0, 300, 300), (1, 32, 32), (2, 48, 50),
              (2, 96, 0), (-1, 10, 10)]


def pos_config(variant):
    uvec, md, sd = POS_VARIANTS[variant]
    return {"loss": {"target_mode": "uvec" if uvec else "vec", "max_distance": md, "bin_map_dil": sd}}


def shape_config(n_classes=SHAPE_N, size_max=SHAPE_MAX):
    return {"trainer": {"n_classes": n_classes}, "mappings": {"size_mapping_min": 0, "size_mapping_max": size_max}}


def shape_edges(n_classes=SHAPE_N, size_max=SHAPE_MAX):
    """lower bin edges and the cyclic flags of the three marks (ValueMapping's linspace)"""
    maps = ut.shape_mappings(shape_config(n_classes, size_max))
    return [np.asarray(m.feature_mapping, dtype=np.float64) for m in maps], [bool(m.is_cyclic) for m in maps]


def _distinct_pixels(rng, H, W, n, taken=()):
    taken = {tuple(t) for t in taken}
    free = np.array([(r, c) for r in range(H) for c in range(W) if (r, c) not in taken], dtype=np.int64)
    return free[rng.permutation(len(free))[:n]]


def _object_params(rng, n):
    return np.stack([rng.uniform(3, 8, n), rng.uniform(6, 14, n), rng.uniform(0, np.pi, n)], 1)


@functools.lru_cache(maxsize=None)
def label_dataset():
    """images, centres, params of the three images: A 160 x 200 with 700 objects on distinct pixels in shuffled order, 12
    pairs of them placed left and right (or above and below) of a pixel; B 64 x 64 without objects; C 96 x 96 with 300, so
    that C's rows in the object table start at 700"""
    rng = np.random.default_rng(2024)
    pairs = []
    for k in range(12):
        r, c = 10 + 12 * k, 20 + 14 * k
        d = 1 + k % 3
        pairs += [(r, c - d), (r, c + d)] if k % 2 else [(r - d, c), (r + d, c)]
    ca = np.concatenate([np.array(pairs, dtype=np.int64), _distinct_pixels(rng, 160, 200, 700 - len(pairs), pairs)])
    ca = ca[rng.permutation(700)]
    cc = _distinct_pixels(rng, 96, 96, 300)
    centers = [ca, np.zeros((0, 2), np.int64), cc]
    params = [_object_params(rng, 700), np.zeros((0, 3)), _object_params(rng, 300)]
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((160, 200), (64, 64), (96, 96))]
    return images, centers, params


def _patch_scene(images_centers_params, row, P, d4=None):
    """the objects of one patch: centres in patch coordinates, params, table rows; d4 = (k, flip) moves them"""
    _, centers, params, starts = images_centers_params
    img, ar, ac = row
    if img < 0:
        return np.zeros((0, 2), np.int64), np.zeros((0, 3)), np.zeros(0, np.int64)
    keep = patch_objects(centers[img], (ar, ac), P)[:MAX_OBJ]
    c = centers[img][keep] - (np.array([ar, ac]) - P // 2)
    p = params[img][keep].copy()
    if d4 is not None and len(keep):
        c = ut.d4_points(c, d4[0], d4[1], P).astype(np.int64)
        p[:, 2] = ut.d4_angle(p[:, 2], d4[0], d4[1])
    return c, p, keep + starts[img]


def _reference(dataset, rows, P, kind, variant, d4s):
    images, centers, params = dataset
    starts = np.concatenate([[0], np.cumsum([len(c) for c in centers])])
    ds = (images, centers, params, starts)
    out = []
    for b, row in enumerate(rows):
        c, p, _ = _patch_scene(ds, row, P, None if d4s is None else d4s[b])
        if kind == "posnet":
            dist, dil, vec, mask = posnet_labels(c, P, *POS_VARIANTS[variant])
            d2, _, ties = nearest(c, P)
            out.append({"dist": dist, "dil": dil, "vec": vec, "mask": mask, "d2": d2, "ties": ties, "n": len(c)})
        else:
            edges, _ = shape_edges()
            cls, cover, margin = shapenet_labels(c, p, value_classes(p, edges), P)
            out.append({"cls": cls, "cover": cover, "margin": margin, "n": len(c)})
    for o in out:
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


def label_d4():
    """the D4 element (k, flip) of every patch of the AUG_GEOMETRIC batch, from the host restatement of the draws"""
    rec = A.aug_params_host(hip_api.AUG_GEOMETRIC, GEO_SEED, 0, 0, len(LABEL_ROWS), LABEL_P, 3)
    return [(int(r["rot"]), int(r["flip"])) for r in rec]


@functools.lru_cache(maxsize=None)
def label_reference(kind, variant="uvec8", geometric=False):
    """per patch of LABEL_ROWS a dict of read-only arrays; posnet: dist, dil, vec, mask (+ d2, ties); shapenet: cls, cover
    (+ margin)"""
    return _reference(label_dataset(), LABEL_ROWS, LABEL_P, kind, variant, label_d4() if geometric else None)


# ---- inputs: the object cap ------------------------------------------------------------------------------------------------
CAP_P, CAP_N = 40, 1100


@functools.lru_cache(maxsize=None)
def cap_dataset():
    """image 0: 40 x 40 with 1100 objects on distinct pixels; image 1: the same with the first 1024 of them"""
    rng = np.random.default_rng(77)
    c = _distinct_pixels(rng, CAP_P, CAP_P, CAP_N)
    p = _object_params(rng, CAP_N)
    images = [rng.integers(0, 256, size=(CAP_P, CAP_P, 3), dtype=np.uint8) for _ in range(2)]
    return images, [c, c[:MAX_OBJ].copy()], [p, p[:MAX_OBJ].copy()]


@functools.lru_cache(maxsize=None)
def cap_reference(kind):
    """the labels of the patch that holds the whole image, from its first 1024 objects in annotation order"""
    return _reference(cap_dataset(), [(1, CAP_P // 2, CAP_P // 2)], CAP_P, kind, "uvec8", None)[0]


# ---- inputs: the exact class perturbation ----------------------------------------------------------------------------------
PERT_P, PERT_B, PERT_N, PERT_SEED = 16, 256, 8, 9
PERT_GRID = [(4, 4), (4, 12), (12, 4), (12, 12)]
# (a, b): size class 0 | 7 and ratio class 7 | ratio class 0 | both in the middle; under size_mapping_max = 8 a bin is 1 wide
PERT_SIZES = [(0.5, 0.9), (7.0, 7.5), (0.5, 4.4), (3.0, 5.0)]
PERT_ANGLES = [0.1, 3.0, 1.3, 2.2]                       # angle class 0, 7, 3, 5 of 8


@functools.lru_cache(maxsize=None)
def perturb_dataset():
    """eight 16 x 16 images of four objects each, 8 px apart: no polygon reaches another object's centre (the largest
    half-diagonal is 5.2 px), so the class at a centre is that object's own"""
    centers, params = [], []
    for i in range(8):
        centers.append(np.array(PERT_GRID, dtype=np.int64))
        params.append(np.array([[*PERT_SIZES[(i + k) % 4], PERT_ANGLES[(i // 2 + k) % 4]]
                                for k in range(4)]))
    images = [np.zeros((PERT_P, PERT_P, 3), np.uint8) for _ in range(8)]
    return images, centers, params


def perturb_rows():
    return [(b % 8, PERT_P // 2, PERT_P // 2) for b in range(PERT_B)]


@functools.lru_cache(maxsize=None)
def perturb_reference():
    """plain [B,4,3] and perturbed [B,4,3] classes of the four objects of every patch, and the draws [B,4,3]"""
    _, _, params = perturb_dataset()
    edges, cyclic = shape_edges(PERT_N, float(PERT_N))
    plain, pert, draws = [], [], []
    for b, (img, _, _) in enumerate(perturb_rows()):
        rows = 4 * img + np.arange(4)
        plain.append(value_classes(params[img], edges))
        pert.append(perturbed_classes(params[img], edges, cyclic, rows, PERT_SEED, 0, 0, b))
        draws.append(perturbation_draws(rows, PERT_SEED, 0, 0, b))
    return np.stack(plain), np.stack(pert), np.stack(draws)


# ---- inputs: the losses ----------------------------------------------------------------------------------------------------
DIV_W, DIV_B = cases.DIV_W, cases.DIV_B
# (B, P, input scale, special): the smallest shapes, a one-row second band, an odd partial band, 258 partials; scale 6 is
# the saturated regime; "zero": mask and dil all zero, "ones": mask all one, "full": mask and dil all one, "dilzero": dil
# all zero
POSNET_CASES = [(1, 3, 1.5, None), (2, 4, 1.5, None), (2, 5, 1.5, None), (2, 17, 1.5, None), (3, 33, 1.5, None),
                (129, 32, 1.5, None), (2, 17, 6.0, None), (129, 32, 6.0, None), (2, 17, 1.5, "zero"), (2, 17, 1.5, "ones"),
                (2, 17, 1.5, "full"), (2, 5, 1.5, "zero"), (2, 5, 1.5, "ones"), (1, 3, 1.5, "dilzero")]


def posnet_loss_case(B, P, scale, special=None):
    """out, vec, mask, dil float32 (the recipe of unet_train_cases.posnet_loss_inputs at any shape)"""
    rng = np.random.default_rng([17, B, P, int(10 * scale)])
    out = rng.normal(0, scale, size=(B, 3, P, P)).astype(np.float32)
    mask = (rng.random((B, P, P)) < 0.3).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, size=(B, P, P))
    dil = (rng.random((B, P, P)) * (rng.random((B, P, P)) < 0.1)).astype(np.float32)
    if special == "zero":
        mask[:], dil[:] = 0, 0
    elif special == "ones":
        mask[:] = 1
    elif special == "full":
        mask[:], dil[:] = 1, 1
    elif special == "dilzero":
        dil[:] = 0
    vec = (np.stack([np.cos(ang), np.sin(ang)], axis=1) * mask[:, None]).astype(np.float32)
    return out, vec, mask, dil


@functools.lru_cache(maxsize=None)
def posnet_loss_reference(B, P, scale, special, form, mode="mixed"):
    out, vec, mask, dil = posnet_loss_case(B, P, scale, special)
    train = form == "train"
    return posnet_loss_ref(out, vec, mask, dil, DIV_W if train else None, DIV_B if train else None, mode)


def builder_posnet_out():
    """the network output that the builder-to-loss test puts against the labels of LABEL_ROWS"""
    return np.random.default_rng(41).normal(0, 1.5, size=(len(LABEL_ROWS), 3, LABEL_P, LABEL_P)).astype(np.float32)


def builder_logits():
    rng = np.random.default_rng(43)
    return [rng.normal(0, 2.0, size=(len(LABEL_ROWS), SHAPE_N, LABEL_P, LABEL_P)).astype(np.float32) for _ in range(3)]


@functools.lru_cache(maxsize=None)
def builder_posnet_reference(form, mode="mixed"):
    """the PosNet loss of builder_posnet_out() against the reference labels of the plain label batch"""
    lab = label_reference("posnet")
    train = form == "train"
    return posnet_loss_ref(builder_posnet_out(), *(np.stack([r[k] for r in lab]) for k in ("vec", "mask", "dil")),
                           DIV_W if train else None, DIV_B if train else None, mode)


SHAPENET_SHAPES = [(1, 1, 1), (2, 17, 5), (3, 16, 32), (129, 32, 8)]
SHAPENET_COVERS = ["random", "empty", "full", "lastband"]


def shapenet_loss_case(B, P, n, cover_kind):
    """three logits [B,n,P,P] float32, cls [3,B,P,P] uint8, cover [B,P,P] uint8; "lastband": patch 0's only covered pixel is
    the last one of its last band, the other patches as "random" """
    rng = np.random.default_rng([23, B, P, n])
    logits = [rng.normal(0, 2.0, size=(B, n, P, P)).astype(np.float32) for _ in range(3)]
    cls = rng.integers(0, n, size=(3, B, P, P)).astype(np.uint8)
    cover = (rng.random((B, P, P)) < 0.25).astype(np.uint8)
    if cover_kind == "empty":
        cover[:] = 0
    elif cover_kind == "full":
        cover[:] = 1
    elif cover_kind == "lastband":
        cover[0] = 0
        cover[0, P - 1, P - 1] = 1
    return logits, cls, cover


@functools.lru_cache(maxsize=None)
def shapenet_loss_reference(B, P, n, cover_kind):
    return shapenet_loss_ref(*shapenet_loss_case(B, P, n, cover_kind))
