"""Test helper (no test in here): the spatial ops of the augmentation recipe restated in NumPy.

* ``aug_params_host``: the record ``mpp_train_aug_params`` writes, from ``hip_api.philox`` alone (the draw table is in the
  header of csrc/mpp_train.hip);
* ``restate_patch``: the whole image pipeline of one patch in float64, given its record: D4, histogram matching, shadow,
  fog, channel shuffle / dropout, brightness-contrast, CLAHE / RGB shift / to-gray, downscale, median / box blur, Gauss
  noise, / 255.  The definitions are those of DESIGN.md section 8; nothing here calls the library but ``philox``.
"""
import numpy as np

from mpp_cnn_rs_object_detection_amd import hip_api
from mpp_cnn_rs_object_detection_amd import unet_training as ut

GEO, MED, STRONG, HM, SPATIAL = (hip_api.AUG_GEOMETRIC, hip_api.AUG_MEDIUM, hip_api.AUG_STRONG, hip_api.AUG_HISTMATCH,
                                 getattr(hip_api, "AUG_SPATIAL", 32))
MAX_HAZE = 64
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
SIX = ("shadow", "fog", "clahe", "downscale", "blur")          # the record's fields of the six ops (blur: median | box)


# ---- Philox ----------------------------------------------------------------------------------------------------------------
def philox_many(ctr: np.ndarray, key) -> np.ndarray:
    """Philox4x32-10 of counters [n, 4] under one key, in NumPy (the CPU tests compare it with ``hip_api.philox``)"""
    c = [np.asarray(ctr)[:, k].astype(np.uint64) for k in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xffffffff), np.uint64(int(key[1]) & 0xffffffff)
    mask, s32 = np.uint64(0xffffffff), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & mask, (p0 >> s32) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(c, 1).astype(np.uint32)


def unif(words) -> np.ndarray:
    return (np.asarray(words).astype(np.float64) + 0.5) / 4294967296.0


def _draw(seed, epoch, batch, patch, stream, index) -> np.ndarray:
    return unif(hip_api.philox([batch, patch, stream, index], [seed, epoch]))


def rand_int(u: float, lo: int, hi: int) -> int:
    """randint(lo, hi), both ends included, from one uniform"""
    return min(hi, lo + int(u * (hi - lo + 1)))


# ---- the record ------------------------------------------------------------------------------------------------------------
def haze_plan(P: int, fog_coef: float):
    """the rounds of albumentations' haze loop: [(number of points, midx, midy)], and hw"""
    hw = max(1, int(P // 3 * fog_coef))
    midx, midy, index, rounds = P // 2 - 2 * hw, P // 2 - hw, 1, []
    while midx > -hw or midy > -hw:
        rounds.append((hw // 10 * index, midx, midy))
        midx -= 3 * hw * P // (2 * P)
        midy -= 3 * hw * P // (2 * P)
        index += 1
    return rounds, hw


def haze_count(P: int, hw: int) -> int:
    """the number of haze points as a function of (P, hw) alone"""
    midx, midy, index, n = P // 2 - 2 * hw, P // 2 - hw, 1, 0
    while midx > -hw or midy > -hw:
        n += hw // 10 * index
        midx -= 3 * hw * P // (2 * P)
        midy -= 3 * hw * P // (2 * P)
        index += 1
    return n


def aug_params_host(flags: int, seed: int, epoch: int, batch: int, B: int, P: int, n_images: int) -> np.ndarray:
    out = np.zeros(B, hip_api.AUG_RECORD_DTYPE)
    for b in range(B):
        r = out[b]
        d = lambda stream, index: _draw(seed, epoch, batch, b, stream, index)   # noqa: E731
        if flags & HM:
            u = d(0, 5)
            r["hm"], r["tmpl"], r["blend"] = u[0] < 0.5, min(n_images - 1, int(u[1] * n_images)), 0.1 + u[2] * 0.65
        if flags & GEO:
            u = d(0, 0)
            r["rot"] = int(u[1] * 4.0) if u[0] < 0.5 else 0
            r["flip"] = 1 + int(u[3] * 3.0) if u[2] < 0.5 else 0
        r["alpha"] = 1.0                                                         # (PatchAug's defaults)
        if not flags & (MED | STRONG):
            continue
        strong = bool(flags & STRONG)
        u = d(0, 1)
        if strong and u[0] < 0.5:
            r["chan_op"] = 1 if u[1] < 0.5 else 2
            r["chan_arg"] = int(u[2] * (6.0 if r["chan_op"] == 1 else 3.0))
        if strong and u[3] < 0.5:
            r["bc"] = 1
        u = d(0, 2)
        r["alpha"] = np.float32(1.0 + (u[0] * 0.4 - 0.2))
        r["beta"] = np.float32((u[1] * 0.4 - 0.2) * 255.0)
        fired = u[2] < 0.5
        if fired:
            w = u[3] * (1.1 if strong else 1.0)
            r["color"] = 0 if w < 0.5 else (1 if w < 1.0 else 2)
            r["clahe"] = bool(flags & SPATIAL) and r["color"] == 0
        u = d(0, 3)
        r["shift"] = (u[:3] * 40.0 - 20.0).astype(np.float32)
        r["noise"] = u[3] < 0.5
        r["sigma"] = np.sqrt(10.0 + d(0, 4)[0] * 40.0)
        if not flags & SPATIAL:
            continue
        u = d(0, 6)
        if strong:
            r["shadow"] = u[0] < 0.5
            r["n_poly"] = (1 + (u[1] < 0.5)) if r["shadow"] else 0
            r["fog"] = u[2] < 0.5
            r["fog_coef"] = 0.3 + u[3] * 0.7
        u = d(0, 7)
        r["clip"] = 1.0 + u[0] * 3.0
        if strong:
            r["downscale"] = u[1] < 0.5
        if u[2] < 0.2:
            r["blur"] = 1 if u[3] < 0.5 else 2
        for v in range(5 * int(r["n_poly"])):
            u = d(3, v)
            r["poly"][v // 5, v % 5] = (rand_int(u[0], 0, P), rand_int(u[1], P // 2, P))
        if r["fog"]:
            rounds, hw = haze_plan(P, float(r["fog_coef"]))
            k = 0
            for count, midx, midy in rounds:
                for _ in range(count):
                    assert k < MAX_HAZE
                    u = d(3, 16 + k)
                    r["haze"][k] = (rand_int(u[0], midx, P - midx - hw), rand_int(u[1], midy, P - midy - hw))
                    k += 1
            r["n_haze"] = k
    return out


def selects(rec) -> tuple:
    """which of the six ops a record selects, as a tuple of names"""
    names = []
    if rec["shadow"]:
        names.append("shadow")
    if rec["fog"]:
        names.append("fog")
    if rec["clahe"]:
        names.append("clahe")
    if rec["downscale"]:
        names.append("downscale")
    if rec["blur"] == 1:
        names.append("median")
    if rec["blur"] == 2:
        names.append("blur")
    return tuple(names)


# ---- the ops, float64 ------------------------------------------------------------------------------------------------------
def clip255(x):
    return np.clip(x, 0.0, 255.0)


def polygon_mask(P: int, verts) -> np.ndarray:
    """even-odd crossing rule on pixel centres (the statement of csrc/mpp_classics.hpp); verts (x, y) = (column, row)"""
    yy, xx = np.mgrid[:P, :P].astype(np.float64)
    inside = np.zeros((P, P), bool)
    q = len(verts) - 1
    for e in range(len(verts)):
        xe, ye = float(verts[e][0]), float(verts[e][1])
        xj, yq = float(verts[q][0]), float(verts[q][1])
        cond = ((ye <= yy) & (yy < yq)) | ((yq <= yy) & (yy < ye))
        if yq != ye:
            inside ^= cond & (xx < (xj - xe) * (yy - ye) / (yq - ye) + xe)
        q = e
    return inside


def shadow_rgb(x: np.ndarray) -> np.ndarray:
    """RGB -> HLS, L *= 0.5, HLS -> RGB on [..., 3] values in 0..255"""
    c = x / 255.0
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    mx, mn = c.max(-1), c.min(-1)
    d = mx - mn
    L = (mx + mn) / 2
    safe = np.where(d == 0, 1.0, d)
    S = np.where(L < 0.5, d / np.where(d == 0, 1.0, mx + mn), d / np.where(d == 0, 1.0, 2.0 - mx - mn))
    h = np.where(mx == r, (g - b) / safe, np.where(mx == g, 2.0 + (b - r) / safe, 4.0 + (r - g) / safe)) / 6.0
    h = np.where(h < 0, h + 1.0, h)
    L2 = L * 0.5
    q = np.where(L2 <= 0.5, L2 * (1.0 + S), L2 + S - L2 * S)
    p = 2.0 * L2 - q
    out = np.empty_like(c)
    for ch, off in enumerate((1.0 / 3.0, 0.0, -1.0 / 3.0)):
        t = h + off
        t = np.where(t < 0, t + 1.0, t)
        t = np.where(t >= 1.0, t - 1.0, t)
        v = np.where(t < 1.0 / 6.0, p + (q - p) * 6.0 * t,
                     np.where(t < 0.5, q, np.where(t < 2.0 / 3.0, p + (q - p) * (2.0 / 3.0 - t) * 6.0, p)))
        out[..., ch] = np.where(d == 0, L2, v)
    return clip255(out * 255.0)


def fog_counts(P: int, haze, hw2: int) -> np.ndarray:
    """k: how many of the discs (radius hw2 // 2, centre point + hw2 // 2) cover each pixel"""
    yy, xx = np.mgrid[:P, :P]
    rad = hw2 // 2
    k = np.zeros((P, P), np.int64)
    for x, y in haze:
        k += ((xx - (int(x) + rad)) ** 2 + (yy - (int(y) + rad)) ** 2 <= rad * rad)
    return k


def box_mean(x: np.ndarray, s: int) -> np.ndarray:
    """box mean of side s, anchor s // 2, BORDER_REFLECT_101, per channel of [P, P, 3]"""
    a = s // 2
    pad = np.pad(x, ((a, s - 1 - a), (a, s - 1 - a), (0, 0)), mode="reflect")
    P = x.shape[0]
    acc = np.zeros_like(x)
    for di in range(s):
        for dj in range(s):
            acc += pad[di:di + P, dj:dj + P]
    return acc / (s * s)


def fog(x: np.ndarray, P: int, fog_coef: float, haze) -> np.ndarray:
    hw2 = max(int(P // 3 * fog_coef), 10)
    k = fog_counts(P, haze, hw2)
    alpha = 0.08 * fog_coef
    x = clip255(255.0 - (255.0 - x) * ((1.0 - alpha) ** k)[..., None])
    s = hw2 // 10
    return clip255(box_mean(x, s)) if s > 1 else x


def rgb_to_lab(x: np.ndarray) -> np.ndarray:
    c = x / 255.0
    lin = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    X = (0.412453 * lin[..., 0] + 0.357580 * lin[..., 1] + 0.180423 * lin[..., 2]) / 0.950456
    Y = 0.212671 * lin[..., 0] + 0.715160 * lin[..., 1] + 0.072169 * lin[..., 2]
    Z = (0.019334 * lin[..., 0] + 0.119193 * lin[..., 1] + 0.950227 * lin[..., 2]) / 1.088754
    f = lambda t: np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)   # noqa: E731
    fx, fy, fz = f(X), f(Y), f(Z)
    L = np.where(Y > 0.008856, 116.0 * fy - 16.0, 903.3 * Y)
    return np.stack([L, 500.0 * (fx - fy), 200.0 * (fy - fz)], -1)


def lab_to_rgb(lab: np.ndarray) -> np.ndarray:
    L, a, b = lab[..., 0], lab[..., 1], lab[..., 2]
    fy = (L + 16.0) / 116.0
    Y = np.where(L > 903.3 * 0.008856, fy ** 3, L / 903.3)
    fy2 = np.where(Y > 0.008856, np.cbrt(Y), 7.787 * Y + 16.0 / 116.0)
    finv = lambda f: np.where(f > 6.0 / 29.0, f ** 3, (f - 16.0 / 116.0) / 7.787)   # noqa: E731
    X, Z = finv(a / 500.0 + fy2) * 0.950456, finv(fy2 - b / 200.0) * 1.088754
    lin = np.stack([3.240479 * X - 1.537150 * Y - 0.498535 * Z, -0.969256 * X + 1.875991 * Y + 0.041556 * Z,
                    0.055648 * X - 0.204043 * Y + 1.057311 * Z], -1)
    c = np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * np.maximum(lin, 0.0031308) ** (1.0 / 2.4) - 0.055)
    return clip255(c * 255.0)


def clahe_clip(hist: np.ndarray, limit: int) -> np.ndarray:
    """OpenCV's clip and redistribute of one 256-bin tile histogram"""
    h = hist.astype(np.int64).copy()
    excess = int(np.maximum(h - limit, 0).sum())
    h = np.minimum(h, limit)
    h += excess // 256
    rest = excess % 256
    if rest:
        step = max(256 // rest, 1)
        bins = np.arange(256)
        h += ((bins % step == 0) & (bins // step < rest)).astype(np.int64)
    return h


def clahe_lut(hist: np.ndarray, clip: float, area: int) -> np.ndarray:
    limit = max(1, int(clip * area / 256))
    return np.minimum(255, np.rint(np.cumsum(clahe_clip(hist, limit)) * 255.0 / area)).astype(np.int64)


def clahe_l8(L8: np.ndarray, clip: float) -> np.ndarray:
    """CLAHE of an 8-bit [P, P] plane on an 8 x 8 grid: the float bilinear blend of the four tiles' lut[L8]"""
    P = L8.shape[0]
    ts = P // 8
    luts = np.empty((8, 8, 256), np.int64)
    for ty in range(8):
        for tx in range(8):
            tile = L8[ty * ts:(ty + 1) * ts, tx * ts:(tx + 1) * ts]
            luts[ty, tx] = clahe_lut(np.bincount(tile.ravel(), minlength=256), clip, ts * ts)
    f = np.arange(P) / ts - 0.5
    t1 = np.floor(f).astype(np.int64)
    w = f - t1
    lo, hi = np.clip(t1, 0, 7), np.clip(t1 + 1, 0, 7)
    ya, xa = w[:, None], w[None, :]
    g = lambda ty, tx: luts[ty[:, None], tx[None, :], L8].astype(np.float64)   # noqa: E731
    return (g(lo, lo) * (1 - xa) + g(lo, hi) * xa) * (1 - ya) + (g(hi, lo) * (1 - xa) + g(hi, hi) * xa) * ya


def clahe(x: np.ndarray, clip: float, window: float = 1e-3):
    """returns (image, pre: the pre-rounding L* 255 / 100 of every pixel)"""
    lab = rgb_to_lab(x)
    pre = lab[..., 0] * 255.0 / 100.0
    L8 = np.clip(np.rint(pre), 0, 255).astype(np.int64)
    lab[..., 0] = clahe_l8(L8, clip) * 100.0 / 255.0
    return lab_to_rgb(lab), pre


def down_map(P: int) -> np.ndarray:
    """m(t): the source index of Downscale(0.9), nearest both ways"""
    d = int(np.rint(0.9 * P))
    t = np.arange(P)
    return np.minimum(P - 1, np.floor((t * d // P) / 0.9).astype(np.int64))


def median3(x: np.ndarray) -> np.ndarray:
    P = x.shape[0]
    pad = np.pad(x, ((1, 1), (1, 1), (0, 0)), mode="edge")
    return np.median(np.stack([pad[di:di + P, dj:dj + P] for di in range(3) for dj in range(3)]), axis=0)


def blur3(x: np.ndarray) -> np.ndarray:
    return clip255(box_mean(x, 3))


def noise_normals(seed, epoch, batch, patch, P) -> np.ndarray:
    """[P, P, 3] standard normals of the Gauss noise: Philox stream 2, index = pixel, Box-Muller on its four words"""
    pix = np.arange(P * P, dtype=np.uint64)
    ctr = np.stack([np.full_like(pix, batch), np.full_like(pix, patch), np.full_like(pix, 2), pix], 1)
    u = unif(philox_many(ctr, (seed, epoch)))
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    t0, t1 = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], 1).reshape(P, P, 3)


def match_lut(src: np.ndarray, tmpl_counts: np.ndarray) -> np.ndarray:
    """skimage's match_histograms for one channel as a table over the 256 values (as tests/test_unet_resampling_host.py)"""
    src_q = np.cumsum(np.bincount(src.ravel(), minlength=256)) / src.size
    values = np.nonzero(tmpl_counts)[0]
    return np.interp(src_q, np.cumsum(tmpl_counts[values]) / tmpl_counts.sum(), values)


def restate_patch(crop: np.ndarray, rec, key, tmpl_counts=None, window: float = 1e-3):
    """crop: the zero-padded P x P x 3 uint8 read of the patch (before D4); rec: its record; key (seed, epoch, batch, patch);
    tmpl_counts [3][256]: the bincounts of the record's template image.  Returns (patch [3, P, P] float64 in [0, 1],
    exempt [P, P] bool: the pixels CLAHE's bin-flip exemption covers, n_flip: the pixels within ``window`` of a bin edge)."""
    P = crop.shape[0]
    x = ut.d4_image(crop, int(rec["rot"]), int(rec["flip"])).astype(np.float64)
    if rec["hm"]:
        s = ut.d4_image(crop, int(rec["rot"]), int(rec["flip"]))
        for ch in range(3):
            lut = match_lut(s[..., ch], np.asarray(tmpl_counts[ch]))
            x[..., ch] = clip255(rec["blend"] * lut[s[..., ch]] + (1.0 - rec["blend"]) * s[..., ch])
    if rec["shadow"]:
        m = np.zeros((P, P), bool)
        for k in range(int(rec["n_poly"])):
            m |= polygon_mask(P, rec["poly"][k])
        x[m] = shadow_rgb(x[m])
    if rec["fog"]:
        x = fog(x, P, float(rec["fog_coef"]), rec["haze"][:int(rec["n_haze"])])
    if rec["chan_op"] == 1:
        x = x[..., list(PERMS[int(rec["chan_arg"])])]
    elif rec["chan_op"] == 2:
        x = x.copy()
        x[..., int(rec["chan_arg"])] = 0.0
    if rec["bc"]:
        x = clip255(float(rec["alpha"]) * x + float(rec["beta"]))
    exempt, n_flip = np.zeros((P, P), bool), 0
    if rec["clahe"]:
        x, pre = clahe(x, float(rec["clip"]))
        near = np.abs(pre - np.floor(pre) - 0.5) < window
        n_flip = int(near.sum())
        ts = P // 8
        tiles = near.reshape(8, ts, 8, ts).any(axis=(1, 3))
        grown = np.pad(tiles, 1)
        tiles = np.any([grown[di:di + 8, dj:dj + 8] for di in range(3) for dj in range(3)], axis=0)
        exempt = np.repeat(np.repeat(tiles, ts, 0), ts, 1)
    elif rec["color"] == 1:
        x = clip255(x + rec["shift"].astype(np.float64))
    elif rec["color"] == 2:
        x = np.repeat(clip255(0.299 * x[..., :1] + 0.587 * x[..., 1:2] + 0.114 * x[..., 2:]), 3, -1)
    if rec["downscale"]:
        m = down_map(P)
        x = x[m][:, m]
        exempt = exempt[m][:, m]
    if rec["blur"]:
        x = median3(x) if rec["blur"] == 1 else blur3(x)
        grown = np.pad(exempt, 1, mode="edge")
        exempt = np.any([grown[di:di + P, dj:dj + P] for di in range(3) for dj in range(3)], axis=0)
    if rec["noise"]:
        seed, epoch, batch, patch = key
        x = clip255(x + float(rec["sigma"]) * noise_normals(seed, epoch, batch, patch, P))
    return (x / 255.0).transpose(2, 0, 1), exempt, n_flip


# ---- the inputs both test modules use ---------------------------------------------------------------------------------------
SEED, EPOCH, B = 11, 2, 64
#: (level, P, batches): the pools of patches compared with the restatement
POOLS = [("strong", 128, 8), ("medium", 128, 4), ("strong", 64, 4), ("medium", 64, 2)]
CLAHE_FLIP_CAP = 4               # pixels of a patch within the window of a bin edge; a patch above it is left out
LEFT_OUT_SHARE = 1 / 8


def posterize(img: np.ndarray, levels: int = 3) -> np.ndarray:
    """a float image in [0, 1] -> uint8 with ``levels`` values per channel: CLAHE's bin-flip cap (4 pixels of a patch within
    1e-3 of a bin edge) can only hold for images of few colours; 16 384 pixels of free colours put ~33 there"""
    q = np.clip(np.floor(img * levels), 0, levels - 1)
    return ((q + 0.5) / levels * 255).astype(np.uint8)


def test_images():
    """three synthetic scenes (``synth.make_scene_image``, posterized) and one image of uniform random bytes"""
    from mpp_cnn_rs_object_detection_amd import synth
    imgs = []
    for k, (shape, n) in enumerate([((256, 256), 230), ((200, 184), 120), ((160, 240), 150)]):
        imgs.append(posterize(synth.make_scene_image(shape, n, seed=k)[0]))
    imgs.append(np.random.default_rng(9).integers(0, 256, size=(96, 128, 3), dtype=np.uint8))
    return imgs


test_images.__test__ = False


def pool_flags(level: str, spatial: bool = True) -> int:
    return GEO | HM | (STRONG if level == "strong" else MED) | (SPATIAL if spatial else 0)


def pool_rows(level: str, P: int, batch: int, imgs):
    """desc rows (image, anchor row, anchor col) of one batch: every 16th patch from the random-bytes image, anchors
    anywhere in [0, shape] so that crops hang over the border"""
    rng = np.random.default_rng([P, batch, len(level)])
    rows = []
    for b in range(B):
        i = len(imgs) - 1 if b % 16 == 0 else int(rng.integers(0, len(imgs) - 1))
        H, W = imgs[i].shape[:2]
        rows.append((i, int(rng.integers(0, H + 1)), int(rng.integers(0, W + 1))))
    return rows


def crop(img: np.ndarray, ar: int, ac: int, P: int) -> np.ndarray:
    """the zero-padded P x P read at anchor - P/2 (uint8)"""
    out = np.zeros((P, P, 3), np.uint8)
    r0, c0 = ar - P // 2, ac - P // 2
    ra, rb, ca, cb = max(0, r0), min(img.shape[0], r0 + P), max(0, c0), min(img.shape[1], c0 + P)
    if rb > ra and cb > ca:
        out[ra - r0:rb - r0, ca - c0:cb - c0] = img[ra:rb, ca:cb]
    return out


def restate_pool(level: str, P: int, batches: int, imgs, records=None):
    """[(batch, patch, record, restated patch, exempt, n_flip)] of a pool; records: per batch, default the host's"""
    counts = [[np.bincount(im[..., ch].ravel(), minlength=256) for ch in range(3)] for im in imgs]
    out = []
    for batch in range(batches):
        rec = aug_params_host(pool_flags(level), SEED, EPOCH, batch, B, P, len(imgs)) if records is None else records[batch]
        for b, (i, ar, ac) in enumerate(pool_rows(level, P, batch, imgs)):
            x, exempt, n_flip = restate_patch(crop(imgs[i], ar, ac, P), rec[b], (SEED, EPOCH, batch, b), counts[int(rec[b]["tmpl"])])
            out.append((batch, b, rec[b], x, exempt, n_flip))
    return out
