"""The edge cases of the rescale tests (host and GPU): small, misaligned and limit-sized inputs of ``MppContext.rescale``, their
references (``rescale_ref.py``), and ``plan``: a plain Python restatement of what ``mpp_rescale_run`` refuses, of its bands
and of every address ``k_rescale_rows`` forms, which counts per case the branches of the kernels that the case reaches.

A case is Gaussian (the project's tables: ``rescale_tables`` per axis; reference: the scipy restatement) or generic (seeded
random tables; reference: ``apply_tables`` in ``np.longdouble``).  Images are seeded uint8 noise; one case alone keeps the
flat blocks of ``translation_cases.make_image``.
"""
import functools

import numpy as np

import rescale_ref as R
from mpp_cnn_rs_object_detection_amd import dataset_translation as dt
from translation_cases import make_image

# the constants of csrc/mpp_rescale.hip
RS_COLS, RS_WAVES, RS_RPT = 64, 4, 4
RS_ROWS = RS_WAVES * RS_RPT
RS_LDS_MAX = 64 * 1024
RS_MAX_TAPS = 4096
DEFAULT_WORKSPACE = 512 << 20

GAUSS_TOL = 1e-12


def noise_image(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


class Case:
    """kind 'scale': both axes through ``rescale_image_tables(H, W, scale)``; 'shape': the output size given per axis;
    'generic': random tables (``taps`` = (Tr, Tc), ``out`` = (oh, ow))"""

    def __init__(self, name, H, W, kind, scale=None, out=None, taps=None, seed=1, flat=False, why=""):
        self.name, self.H, self.W, self.kind, self.scale, self.taps, self.seed, self.flat, self.why = \
            name, H, W, kind, scale, taps, seed, flat, why
        self.out = dt.rescale_output_shape(H, W, scale) if kind == "scale" else tuple(out)

    def __repr__(self):
        return self.name

    @property
    def gaussian(self):
        return self.kind != "generic"

    def image(self):
        return _image(self)

    def tables(self):
        return _tables(self)

    def reference(self):
        """float64 [oh,ow,3], not to be written to: the scipy restatement, or the longdouble evaluation rounded to float64"""
        return _reference(self)

    def tolerance(self):
        """on |device float64 - reference|: 1e-12 for Gaussian tables; for generic ones the term-count bound
        2 Tr Tc 2^-53 max_i sum|wr| max_j sum|wc| (factor 2: the division by 255 and the other summation order)"""
        if self.gaussian:
            return GAUSS_TOL
        _, rw, _, cw = self.tables()
        return 2 * rw.shape[1] * cw.shape[1] * 2.0 ** -53 * float(np.abs(rw).sum(axis=1).max()) * float(np.abs(cw).sum(axis=1).max())

    def pass_through(self):
        """every weight is exactly 0 or 1 (both factors 1): each output is one source byte / 255, on the device as in the
        restatement, so 255 v sits on an integer everywhere and no seed can keep it away from one"""
        _, rw, _, cw = self.tables()
        return bool(np.isin(rw, (0.0, 1.0)).all() and np.isin(cw, (0.0, 1.0)).all())


@functools.lru_cache(maxsize=None)
def _image(c):
    img = make_image(c.H, c.W, seed=c.seed) if c.flat else noise_image(c.H, c.W, c.seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _tables(c):
    if c.kind == "scale":
        shape, t = dt.rescale_image_tables(c.H, c.W, c.scale)
        assert shape == c.out
    elif c.kind == "shape":
        t = dt.rescale_tables(c.H, c.out[0]) + dt.rescale_tables(c.W, c.out[1])
    else:
        rng = np.random.default_rng([c.seed, 77])
        (oh, ow), (Tr, Tc) = c.out, c.taps
        t = (rng.integers(0, c.H, (oh, Tr)).astype(np.int32), rng.uniform(-0.5, 1.0, (oh, Tr)),
             rng.integers(0, c.W, (ow, Tc)).astype(np.int32), rng.uniform(-0.5, 1.0, (ow, Tc)))
        for idx, n in ((t[0], c.H), (t[2], c.W)):         # the first and the last byte of the image are among those read
            idx[0, 0], idx[-1, -1] = 0, n - 1
    for a in t:
        a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _reference(c):
    if c.kind == "scale":
        ref = R.rescale_ref(c.image(), c.scale)
    elif c.kind == "shape":
        ref = R.resize_ref(c.image(), *c.out)
    else:
        ref = R.apply_tables(c.image(), *c.tables(), dtype=np.longdouble).astype(np.float64)
    assert ref.shape == c.out + (3,)
    ref.setflags(write=False)
    return ref


def S(H, W, scale, why, **kw):
    return Case(f"{H}x{W}@{scale:g}", H, W, "scale", scale=scale, why=why, **kw)


TINY = [
    S(1, 1, 1.0, "n_in = 1: all indices 0, a 3-byte source"),
    S(2, 2, 0.5, "one output pixel, the mean of the four (255 v a multiple of 1/4: the seed keeps it off the integers)", seed=2),
    S(5, 7, 0.5, "a 105-byte image of 21-byte rows: a row is one chunk or two, the last one runs past the end"),
    S(3, 40, 0.34, "radius 4 > n_in - 1: the mirror folds more than once"),
    S(16, 5, 1.0, "T = 2, the tap at index n_in folded back with weight 0; 16 source rows"),
    S(50, 50, 0.99, "rounds to the source's own size"),
    S(7, 300, 0.2119, "one output row, ow = 64, Tr 26 / Tc 16"),
    S(300, 7, 0.2119, "one output column, Tr 16 / Tc 26"),
]
GROUPS = [
    S(17, 126, 0.5, "ow = 63: one partly filled group, 3 ow odd; rows mod 16 = 1"),
    S(33, 128, 0.5, "ow = 64: one exactly full group, 3 ow even; rows mod 16 = 1"),
    S(31, 130, 0.5, "ow = 65: a full group and one column, 3 ow odd; rows mod 16 = 15"),
]
ROW_TAILS = [
    S(15, 70, 0.5, "15 source rows: the fourth wave's threads hold 3 live rows"),
    S(22, 66, 0.5, "22 source rows: in the second block a thread holds 2 live rows, two waves none"),
]
LDS = [
    S(64, 1400, 0.0936, "ow = 131: the largest admitted reduction of this width"),
    S(64, 1400, 0.093, "ow = 130: refused at the LDS limit"),
    S(40, 1300, 0.095, "4 x 124, just under the limit through rescale_image_tables"),
]
COLS_BLOCKS = [
    S(9, 342, 0.5, "ow = 171: 257 pairs of values, so k_rescale_cols' second block holds one thread, whose second value is padding"),
]
FLAT = S(40, 48, 0.5, "the flat white and black blocks: 255 v on integers, where truncation bites", flat=True)
TWO_FACTORS = [
    Case("24x400->24x50", 24, 400, "shape", out=(24, 50), why="rows kept (Tr 2), columns by 8 (Tc 30)"),
    Case("400x24->50x24", 400, 24, "shape", out=(50, 24), why="rows by 8 (Tr 30), columns kept (Tc 2)"),
    Case("1x200->1x100", 1, 200, "shape", out=(1, 100), why="one source row, columns halved"),
]
GENERIC = Case("generic 37x150->21x71", 37, 150, "generic", out=(21, 71), taps=(3, 5), seed=5,
               why="random indices anywhere, weights of both signs: the clip acts")
ALIGN = S(37, 150, 0.5, "the alignment sweep's picture")
#: row pitches of the sweep: 3 W, + 1, + 8, + 16; 3 W = 450 = 2 mod 16, so none of those keeps (address & 15) fixed from row to
#: row or lets it alternate: 464 (0 mod 16) and 456 (8 mod 16) do
ALIGN_PITCHES = (450, 451, 458, 466, 464, 456)
#: source rows of workspace in the banded runs of the group-edge cases (an output row of theirs reads 6)
BAND_ROWS = 7

ALL_CASES = TINY + GROUPS + ROW_TAILS + COLS_BLOCKS + LDS + [FLAT] + TWO_FACTORS + [GENERIC, ALIGN]
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


# ---- what the comparison of the 8-bit values leaves out --------------------------------------------------------------------
def excluded(ref, tol):
    """values whose 8-bit level the reference cannot settle: ref inside [-tol, 1 + tol] with 255 clip(ref) within 255 tol of
    an integer.  (Outside that interval the device value is clipped for certain: the level is 0 or 255.)"""
    v = 255 * np.clip(ref, 0, 1)
    return (ref >= -tol) & (ref <= 1 + tol) & (np.abs(v - np.round(v)) <= 255 * tol)


def ref_uint8(ref):
    return np.floor(255 * np.clip(ref, 0, 1)).astype(np.uint8)


# ---- folds of the mirror ---------------------------------------------------------------------------------------------------
def taps_folded_twice(n_in, n_out):
    """taps of ``rescale_tables(n_in, n_out)`` whose position before the mirror lies beyond one reflection of the image"""
    f = n_in / n_out
    radius = int(4.0 * max(0.0, (f - 1) / 2) + 0.5)
    i0 = np.floor(f * (np.arange(n_out) + 0.5) - 0.5).astype(np.int64)
    raw = i0[:, None] - radius + np.arange(2 * radius + 2)[None, :]
    if n_in == 1:
        return int((raw != 0).sum())
    return int(((raw < -(n_in - 1)) | (raw > 2 * (n_in - 1))).sum())


# ---- the launcher and the kernels' addressing, restated --------------------------------------------------------------------
def up256(v):
    return (v + 255) & ~255


class Plan:
    """see ``plan``"""


def plan(H, W, tables, pitch=None, base=0, ws_limit=DEFAULT_WORKSPACE, addresses=True):
    """``mpp_rescale_run`` and the addresses of ``k_rescale_rows`` for a source whose first byte sits at ``base`` (only
    ``base & 15`` matters) with rows ``pitch`` bytes apart.  -> Plan with ``refusal`` (None, or a word of the message:
    'taps', 'outside', 'LDS', 'workspace'), ``span``, ``row_stride``, ``lds``, ``tab_bytes``, ``row_bytes``, ``need``,
    ``bands`` [(i0, i1, r0, r1)] and ``counts``."""
    ri, rw, ci, cw = tables
    (oh, Tr), (ow, Tc) = ri.shape, ci.shape
    pitch = 3 * W if pitch is None else pitch
    p = Plan()
    p.refusal, p.bands, p.counts = None, [], {}
    p.shape = (oh, ow, Tr, Tc)
    if Tr > RS_MAX_TAPS or Tc > RS_MAX_TAPS or pitch < 3 * W:
        p.refusal = "taps"
        return p
    if ri.min() < 0 or ri.max() >= H or ci.min() < 0 or ci.max() >= W:
        p.refusal = "outside"
        return p
    groups = []                                        # (j0, columns in the image, cmin, cmax) per workgroup along x
    for j0 in range(0, ow, RS_COLS):
        lanes = np.minimum(j0 + np.arange(RS_COLS), ow - 1)     # lanes past the image repeat the last column
        groups.append((j0, min(RS_COLS, ow - j0), int(ci[lanes].min()), int(ci[lanes].max())))
    p.groups = groups
    p.span = max(g[3] - g[2] + 1 for g in groups)
    p.row_stride = (p.span * 3 + 15 + 15) // 16 * 16
    p.lds = Tc * RS_COLS * 8 + Tc * RS_COLS * 4 + 16 + RS_ROWS * p.row_stride     # weights | indices | min, max | the rows
    if p.lds > RS_LDS_MAX:
        p.refusal = "LDS"
        return p
    ow3 = 3 * ow
    tpitch = (ow3 + 1) & ~1
    p.row_bytes = tpitch * 8
    p.tab_bytes = up256(oh * Tr * 8) + up256(ow * Tc * 8) + up256(oh * Tr * 4) + up256(ow * Tc * 4)
    if ws_limit < p.tab_bytes + p.row_bytes:
        p.refusal = "workspace"
        return p
    max_rows = min((ws_limit - p.tab_bytes) // p.row_bytes, 65535 * RS_ROWS)
    rlo, rhi = ri.min(axis=1), ri.max(axis=1)
    i0 = 0
    while i0 < oh:
        lo, hi, i1 = int(rlo[i0]), int(rhi[i0]), i0 + 1
        if hi - lo + 1 > max_rows:
            p.refusal = "workspace"
            return p
        while i1 < oh and i1 - i0 < 65535:
            l2, h2 = min(lo, int(rlo[i1])), max(hi, int(rhi[i1]))
            if h2 - l2 + 1 > max_rows:
                break
            lo, hi, i1 = l2, h2, i1 + 1
        p.bands.append((i0, i1, lo, hi + 1))
        i0 = i1
    p.need = p.tab_bytes + max(b[3] - b[2] for b in p.bands) * p.row_bytes
    if not addresses:
        return p

    end = base + (H - 1) * pitch + 3 * W               # src_end
    nch = p.row_stride // 16
    n = dict(groups=len(groups), partial_groups=sum(g[1] < RS_COLS for g in groups),
             lanes_past_ow=sum(RS_COLS - g[1] for g in groups), odd_ow3=ow3 & 1,
             cols_blocks=((ow3 + 1) // 2 + 255) // 256, cols_threads_in_last_block=((ow3 + 1) // 2 - 1) % 256 + 1, chunks_inside=0, chunks_low=0, chunks_high=0,
             row_blocks=0, row_blocks_with_tail=0, threads_live_1=0, threads_live_2=0, threads_live_3=0, threads_live_0=0,
             band_rows=[b[3] - b[2] for b in p.bands])
    residues = set()
    for (_, _, r0, r1) in p.bands:
        for rb0 in range(r0, r1, RS_ROWS):
            n["row_blocks"] += 1
            n["row_blocks_with_tail"] += rb0 + RS_ROWS > r1
            for ty in range(RS_WAVES):
                live = min(RS_RPT, max(0, r1 - (rb0 + ty * RS_RPT)))
                if live < RS_RPT:
                    n[f"threads_live_{live}"] += RS_COLS
            for r in range(rb0, min(rb0 + RS_ROWS, r1)):
                for (_, _, cmin, cmax) in groups:
                    a = base + r * pitch + 3 * cmin
                    res = a & 15
                    residues.add(res)
                    first = a - res
                    # the bytes the taps name lie inside the image and inside what is staged; the farthest byte read back
                    assert base <= a and a + 3 * (cmax - cmin + 1) <= end
                    assert a + 3 * (cmax - cmin + 1) <= first + p.row_stride
                    assert res + 3 * (cmax - cmin) + 2 < p.row_stride
                    k = np.arange(nch)
                    lo_cut, hi_cut = first + 16 * k < base, first + 16 * k + 16 > end
                    n["chunks_low"] += int(lo_cut.sum())
                    n["chunks_high"] += int(hi_cut.sum())
                    n["chunks_inside"] += int((~lo_cut & ~hi_cut).sum())
    n["residues"] = sorted(residues)
    p.counts = n
    return p


def band_limit(case, rows):
    """the workspace limit that leaves room for ``rows`` source rows of ``case`` beside its tables"""
    q = plan(case.H, case.W, case.tables(), addresses=False)
    return q.tab_bytes + rows * q.row_bytes
