"""The per-tile naive initialisation (k_naive_init, csrc/mpp_maps.hip) at the edges of the reference's rule (host side: no
GPU import).

Every chain starts from `naive_detection` (sample_rjmcmc.py:23-35 with utils/nms.py:68-110): `detection_map >= threshold`
compared as NumPy compares a float32 map with a Python float, i.e. in float32; a greedy walk over the candidates in
descending value that keeps a candidate iff every centre kept before it lies at `d > nms_distance`; the argmax class
(first maximum) of the three mark maps at each centre, turned into a value by the mapping table.

A case is a detection map, three mark maps, a mapping, a threshold and an NMS distance.  Its expectation does not come
from the C oracle (which restates the same reading of the reference as the kernel, and is itself held to these cases by
tests/test_naive_init_cases_host.py) but from `host_greedy` of tests/test_cnn_detection_host.py, which is pinned to the
reference's recorded output, and from `np.argmax` over the mark rows:

* fixture    the reference's recorded 256 x 320 map at 0.2 (float32 rounds the threshold up), 0.7 and the shipped
             0.6464646464646465 (float32 rounds both down): a pixel equal to float32(thr) is a candidate; the recorded tie
             pixels of the mark maps pin "first of tied maxima";
* plateau    saturated 1.0 blobs on 48 x 80, one over pixel (0, 0) and one over the last pixel: every tie goes to the larger
             index, and H != W catches a swapped idx / W;
* ramp       a strictly monotone 40 x 56 map at thr 0.0 (distance 6.5) and at the value of pixel (0, 1) (distance 2.5): every
             pick depends on the one before; pixel (0, 0) has value 0.0 (rank key 0 if the key is the raw float bits) and is
             the last pick of the first, pixel (0, 1) equals the threshold and is the last pick of the second;
* nms        a 96 x 96 synthetic tile at distances 0.0, 1.0, 4.5, 5.0, 6.0, and three equal peaks at mutual distances 5, 5 and
             sqrt(10) at distance 5.0: the rule keeps only d > distance, so one survives;
* zeros      16 x 24 of +0.0 at thr 0.0, distance 0.0: every pixel is kept, (0, 0) the last;
* negatives  0.3 * standard normal on 40 x 56 with a -0.0 and a +0.0 two pixels apart among negative neighbours, thr -0.5,
             distance 2.5: negative values and -0.0 rank as numbers (-0.0 ties with +0.0, the larger index is kept);
* stack      five 48 x 80 tiles for one context: synthetic, empty (all below the threshold), the plateau, dense noise, a ramp.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from helpers import GOLDEN
from kernel_param_cases import make_mappings
from mpp_cnn_rs_object_detection_amd import synth
from test_cnn_detection_host import host_greedy, mark_maps

SHIPPED_THR = 0.6464646464646465            # model_configs/mpp/mpp_hrcM.json: rounds down in float32
STACK_SHAPE, STACK_THR, STACK_NMS = (48, 80), 0.5, 6.0


@dataclass
class Case:
    name: str
    det: np.ndarray                     # [H, W] float32
    marks: List[np.ndarray]             # 3 x [H, W, 32] float32
    thr: float
    nms: float
    mapping: str = "default"            # kernel_param_cases.make_mappings()
    min_kept: int = 5                   # the fewest centres the case must keep to be worth running
    golden_key: str = ""                # fixture cases: the recorded result "ge_2" / "ge_7" of the same threshold, if any

    @property
    def shape(self) -> Tuple[int, int]:
        return tuple(self.det.shape)

    def __str__(self):
        return self.name


@dataclass
class Expected:
    centers: np.ndarray                 # [K, 2] int32 (row, col) in pick order
    marks: np.ndarray                   # [K, 3] float64: the mapping table's values
    classes: np.ndarray                 # [K, 3] argmax classes
    n_cand: int


def golden():
    return np.load(os.path.join(GOLDEN, "cnn_baseline_golden.npz"))


def _marks_for(shape, seed):
    """seeded random classes through mark_maps (multiples of 1/128 below 0.5, 0.75 at the class); every fifth pixel of map
    (r + c) % 3 holds a second 0.75 at class 31, so that a 'last maximum' or '>=' argmax reads another value there"""
    H, W = shape
    rng = np.random.default_rng([911, seed, H, W])
    cls = rng.integers(0, 32, size=(3, H, W)).astype(np.uint8)
    r, c = np.nonzero((np.arange(H)[:, None] * W + np.arange(W)[None, :]) % 5 == 0)
    k = (r + c) % 3
    ok = cls[k, r, c] < 31
    rc = np.stack([r[ok], c[ok]], axis=1)
    return mark_maps(cls, rc, k[ok], np.full(int(ok.sum()), 31))


def _case(name, det, thr, nms, seed, **kw):
    det = np.ascontiguousarray(det, dtype=np.float32)
    return Case(name, det, _marks_for(det.shape, seed), float(thr), float(nms), **kw)


def ramp(H, W):
    return (np.arange(H * W, dtype=np.float64).reshape(H, W) / (H * W)).astype(np.float32)


def plateau_map(shape=STACK_SHAPE, floor=0.0):
    H, W = shape
    det = np.full(shape, floor, np.float32)
    for r, c in [(0, 0), (H - 1, W - 1), (20, 20), (25, 24), (12, 63), (15, 64), (40, 40), (30, 79), (47, 8)]:
        det[max(0, r - 5):r + 6, max(0, c - 5):c + 6] = 1.0
    return det


def lattice_map():
    det = np.full((32, 32), 0.1, np.float32)
    for r, c in [(10, 12), (13, 16), (10, 17)]:       # offsets (3, 4) and (0, 5): distances 5, 5 and sqrt(10)
        det[r, c] = 0.9
    return det


def negatives_map():
    rng = np.random.default_rng(3)
    neg = (rng.standard_normal((40, 56)) * 0.3).astype(np.float32)
    # the two zeros are the largest values within reach of each other (everything up to 3 px around them is negative), so which
    # of them is kept is decided by their rank alone
    neg[2:9, 2:11] = -np.abs(neg[2:9, 2:11]) - np.float32(0.01)
    neg[5, 5], neg[5, 7] = -0.0, 0.0
    return neg


def _fixture_cases():
    g = golden()
    marks = mark_maps(g["mark_cls"], g["tie_rc"], g["tie_k"], g["tie_j"])
    return [Case(f"fixture-{name}", g["det"], marks, thr, float(g["nms_distance"]), golden_key=key)
            for name, thr, key in (("0.2", 0.2, "ge_2"), ("0.7", 0.7, "ge_7"), ("shipped", SHIPPED_THR, ""))]


def stack_cases() -> List[Case]:
    """the five tiles of the stack case, each also a case of its own (one threshold and distance per context)"""
    H, W = STACK_SHAPE
    rng = np.random.default_rng(20)
    gt_xy = np.stack([rng.integers(4, H - 4, 9), rng.integers(4, W - 4, 9)], axis=1).astype(np.int32)
    gt_mk = np.stack([rng.uniform(6, 12, 9), rng.uniform(0.35, 0.7, 9), rng.uniform(0, np.pi, 9)], axis=1)
    synth_det, _ = synth.render_maps(STACK_SHAPE, gt_xy, gt_mk, noise=0.2, noise_seed=5)
    empty = np.full(STACK_SHAPE, 0.25, np.float32)
    empty[7, 9] = np.nextafter(np.float32(STACK_THR), np.float32(0))        # the largest float32 below the threshold
    noise = rng.random(STACK_SHAPE, dtype=np.float32)
    dets = [("synth", synth_det, 3), ("empty", empty, 0), ("plateau", plateau_map(floor=0.125), 5), ("noise", noise, 5),
            ("ramp", ramp(H, W), 5)]
    return [_case(f"stack-{n}", d, STACK_THR, STACK_NMS, 40 + i, mapping="warped", min_kept=k) for i, (n, d, k) in enumerate(dets)]


def _build() -> List[Case]:
    cases = _fixture_cases()
    cases.append(_case("plateau", plateau_map(), 0.5, 6.0, 1, mapping="warped"))
    r = ramp(40, 56)
    # (distances at which the walk, which starts at the last pixel, ends on the pixel in question: at 6.0 it stops at (1, 7))
    cases.append(_case("ramp-thr0", r, 0.0, 6.5, 2))                                    # keeps (0, 0), value 0.0
    cases.append(_case("ramp-thr-px01", r, float(r[0, 1]), 2.5, 2, mapping="offset"))   # keeps (0, 1), value == thr
    tile = synth.make_tile(96, 30, tile_id=5, noise=0.0)
    for d in (0.0, 1.0, 4.5, 5.0, 6.0):
        cases.append(Case(f"nms-d{d}", tile.det, tile.marks, 0.2, d))
    cases.append(_case("nms-lattice-d5", lattice_map(), 0.5, 5.0, 3, min_kept=1))
    cases.append(_case("zeros", np.zeros((16, 24), np.float32), 0.0, 0.0, 4))
    cases.append(_case("negatives", negatives_map(), -0.5, 2.5, 5, mapping="flags"))
    return cases + stack_cases()


_cases: List[Case] = []
_expected: Dict[Tuple[str, float], Expected] = {}


def cases() -> List[Case]:
    if not _cases:
        _cases.extend(_build())
    return _cases


CASE_NAMES = ["fixture-0.2", "fixture-0.7", "fixture-shipped", "plateau", "ramp-thr0", "ramp-thr-px01", "nms-d0.0", "nms-d1.0",
              "nms-d4.5", "nms-d5.0", "nms-d6.0", "nms-lattice-d5", "zeros", "negatives", "stack-synth", "stack-empty",
              "stack-plateau", "stack-noise", "stack-ramp"]
STACK_NAMES = [n for n in CASE_NAMES if n.startswith("stack-")]


def by_name(name: str) -> Case:
    return {c.name: c for c in cases()}[name]


def edges_of(case: Case) -> np.ndarray:
    return np.stack([m.feature_mapping for m in make_mappings(case.mapping)])


def expected(case: Case, thr: float = None) -> Expected:
    """host_greedy's centres in pick order and the table values at the first maximum of each mark row (computed once)"""
    thr = case.thr if thr is None else float(thr)
    key = (case.name, thr)
    if key not in _expected:
        centers, _, n_cand = host_greedy(case.det, thr, False, case.nms)
        rows = [m[centers[:, 0], centers[:, 1]] for m in case.marks]
        cls = np.stack([np.argmax(r, axis=1) for r in rows], axis=1).reshape(-1, 3)
        edges = edges_of(case)
        marks = np.stack([edges[k][cls[:, k]] for k in range(3)], axis=1).astype(np.float64).reshape(-1, 3)
        centers = centers.astype(np.int32)
        for a in (centers, marks, cls):
            a.setflags(write=False)
        _expected[key] = Expected(centers, marks, cls, n_cand)
    return _expected[key]
