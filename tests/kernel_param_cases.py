"""Chains at kernel parameters and mark mappings other than the defaults (host side: no GPU import).

Every other chain test runs `mappings.default_mappings()` and the defaults of `kernels.make_kernels` (max_delta 8, sigmas
2.0 / 0.1).  The cases here move each of them -- translation windows of 1 x 1 up to 31 x 31 pixels, bin edges that are no
linspace, ranges that do not start at 0, other cyclic flags, other sigmas, split radius and mixtures -- on tiles that are
thinner than the window, longer than one 512-entry chunk of the birth searches, or higher than the 1 024 rows of the
row level kept in LDS.  The CPU oracle is generic in all of them and is the reference.

`CASES` lists the cases, `build(case)` makes a case's maps, mappings, kernels, model and start, `walk(case)` steps the
oracle one step at a time, `count(case, walk)` counts what the walk exercised (tests/test_kernel_param_cases_host.py
holds every case to floors on these counts, so that a lopsided case cannot hide a branch).

The schedules are hot (T0 = 5, alpha = 0.9995: T stays above 0.6): under the default cold schedule the population of a
small tile collapses to about one point and nothing is exercised.  The split / merge case runs at a constant T = 0.6
with a smaller split / merge weight: at T = 5 every split is accepted, the population passes 90 and no merge ever is."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np

from helpers import model_for
from mpp_cnn_rs_object_detection_amd import kernels, synth
from mpp_cnn_rs_object_detection_amd.mappings import ValueMapping, default_mappings

PI = float(np.pi)


def warped(m: ValueMapping) -> ValueMapping:
    """the mapping's lower bin edges moved to vmin + range * (i/32)**1.5: strictly increasing, far from a linspace"""
    i = np.arange(m.n_classes, dtype=float)
    m.feature_mapping = m.v_min + m.range * (i / m.n_classes) ** 1.5
    return m


def make_mappings(name: str):
    if name == "default":
        return default_mappings()
    if name == "offset":        # M1: ranges that do not start at 0
        return [ValueMapping(32, 4, 28), ValueMapping(32, 0.2, 1.0), ValueMapping(32, 0, PI, is_cyclic=True)]
    if name == "warped":        # M2: no linspace (and a range that does not start at 0 under the binary search)
        return [warped(ValueMapping(32, 2, 30)), warped(ValueMapping(32, 0.1, 1.0)), warped(ValueMapping(32, 0, PI, is_cyclic=True))]
    if name == "flags":         # M3: the ratio wraps, the angle is clamped
        return [ValueMapping(32, 0, 32), ValueMapping(32, 0, 1, is_cyclic=True), ValueMapping(32, 0, PI, is_cyclic=False)]
    raise KeyError(name)


@dataclass(frozen=True)
class Case:
    name: str
    shape: Tuple[int, int]
    mapping: str                        # make_mappings()
    setup: str                          # helpers.model_for(): "legacy" or "no-calibration"
    kernel: Dict[str, float]            # fields of the KernelDesc set after make_kernels
    intensity: float
    seed: int
    steps: int = 4000
    T0: float = 5.0
    alpha: float = 0.9995
    chain: int = 0
    split_merge: bool = False
    weights: Optional[Dict[str, float]] = None      # overrides of kernels.BASE_KERNEL_WEIGHTS
    ends: float = 0.0                   # share of the ground truth and of the start placed within 12 px of the long side's ends
    map_seed: int = 0

    @property
    def max_delta(self) -> int:
        return int(self.kernel.get("max_delta", 8))

    def __str__(self):
        return self.name


CASES = [
    Case("wide-default-md12", (48, 80), "default", "legacy", dict(max_delta=12, sigma_trans=3.5, sigma_transform=0.25), 30.0, seed=101),
    Case("thin5x70-offset-md15", (5, 70), "offset", "no-calibration", dict(max_delta=15, sigma_trans=0.5, sigma_transform=0.02), 12.0, seed=102),
    Case("thin70x5-warped-md9", (70, 5), "warped", "legacy", dict(max_delta=9, sigma_transform=0.25), 12.0, seed=103),
    Case("line1x90-flags-md15", (1, 90), "flags", "no-calibration", dict(max_delta=15, sigma_transform=0.25), 8.0, seed=104, steps=3000),
    Case("split40x56-offset-md3", (40, 56), "offset", "legacy", dict(max_delta=3, split_radius=9.0, split_sigma=0.2), 30.0, seed=218,
         split_merge=True, weights=dict(ms_weight=0.4), T0=0.6, alpha=1.0),
    Case("mix48x80-warped-md9", (48, 80), "warped", "no-calibration", dict(max_delta=9, sigma_trans=3.5), 30.0, seed=106,
         weights=dict(uniform_bd_weight=0, gaussian_translation_weight=0)),
    Case("still48x80-flags-md0", (48, 80), "flags", "legacy", dict(max_delta=0, sigma_trans=0.5, sigma_transform=0.02), 30.0, seed=107),
    Case("tall1040x24-default-md3", (1040, 24), "default", "no-calibration", dict(max_delta=3, sigma_trans=3.5), 100.0, seed=108),
    Case("long24x1040-warped-md15", (24, 1040), "warped", "legacy", dict(max_delta=15, sigma_transform=0.02), 100.0, seed=109, ends=0.25),
]
BY_NAME = {c.name: c for c in CASES}


def _positions(rng, shape, n, ends):
    H, W = shape
    xy = np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], axis=1)
    k = int(round(ends * n))
    if k:                                # the first k near the two ends of the long side
        ax, L = (0, H) if H >= W else (1, W)
        near = rng.integers(0, 12, k)
        xy[:k, ax] = np.where(rng.random(k) < 0.5, near, L - 1 - near)
    return xy.astype(np.int32)


@dataclass
class Built:
    case: Case
    det: np.ndarray
    marks: list
    maps: list
    kd: kernels.KernelDesc
    setup: object
    model: object
    xy: np.ndarray
    mk: np.ndarray


def build(case: Case, **kernel_overrides) -> Built:
    """maps rendered on seeded random ground truth (about one rectangle per 250 px), the case's mappings and kernels, and
    a start of as many random rectangles (size 8..14, ratio 0.35..0.6, any angle)"""
    H, W = case.shape
    rng = np.random.default_rng([77, case.map_seed, H, W])
    n = max(3, (H * W) // 250)
    gt_xy = _positions(rng, case.shape, n, case.ends)
    gt_marks = np.stack([rng.uniform(6, 12, n), rng.uniform(0.35, 0.7, n), rng.uniform(0, PI, n)], axis=1)
    det, marks = synth.render_maps(case.shape, gt_xy, gt_marks, noise=0.2, noise_seed=case.seed)
    maps = make_mappings(case.mapping)
    w = dict(kernels.BASE_KERNEL_WEIGHTS, **(case.weights or {}))
    kd = kernels.make_kernels(maps, case.intensity, use_split_merge=case.split_merge, kernel_weights=w)
    kd = dataclasses.replace(kd, **dict(case.kernel, **kernel_overrides))
    setup, _, model = model_for(case.setup)
    xy = _positions(rng, case.shape, n, case.ends)
    mk = np.stack([rng.uniform(8, 14, n), rng.uniform(0.35, 0.6, n), rng.uniform(0, PI, n)], axis=1)
    return Built(case, det, marks, maps, kd, setup, model, xy, mk)


def make_oracle(b: Built):
    import oracle
    o = oracle.Oracle(b.case.shape, b.det, b.marks, b.model, b.kd)
    o.set_points(b.xy, b.mk)
    o.set_temperature(b.case.T0, b.case.alpha, 0.0)
    return o


@dataclass
class Walk:
    built: Built
    props: np.ndarray                   # oracle.PROPOSAL_DTYPE [steps]
    out: np.ndarray                     # oracle.STEPOUT_DTYPE [steps]
    before: list                        # (xy, marks) before each step
    n_before: np.ndarray = field(default=None)
    final: tuple = None                 # (xy, marks) after the last step


_walks: Dict[str, Walk] = {}


def walk(case: Case) -> Walk:
    """the oracle's own chain, one step at a time: the state before every step, its proposal, its outcome (cached)"""
    if case.name in _walks:
        return _walks[case.name]
    b = build(case)
    o = make_oracle(b)
    props, out, before = [], [], []
    for _ in range(case.steps):
        before.append(o.get_points())
        so, pr = o.run(1, case.seed, chain=case.chain, trace=True)
        props.append(pr); out.append(so)
    w = Walk(b, np.concatenate(props), np.concatenate(out), before, np.array([len(s[0]) for s in before]), o.get_points())
    _walks[case.name] = w
    return w


def linspace_class(m: ValueMapping, v):
    """the class a linspace over the mapping's range would give (the device's guess before it looks at the table)"""
    g = np.floor((np.asarray(v, dtype=float) - m.v_min) * (m.n_classes / m.range)).astype(int)
    return np.clip(g, 0, m.n_classes - 1)


def table_class(m: ValueMapping, v):
    return np.maximum(np.searchsorted(m.feature_mapping, np.asarray(v, dtype=float), side="right") - 1, 0)


def count(case: Case, w: Walk) -> dict:
    """what the walk exercised; keys are the conditions of tests/test_kernel_param_cases_host.py"""
    K = kernels
    H, W = case.shape
    md = case.max_delta
    p, out, kd, maps = w.props, w.out, w.built.kd, w.built.maps
    k, acc, has_t = p["kernel"], out["accepted"] > 0, p["target"] >= 0
    c = dict(pop_min=int(w.n_before.min()), pop_median=float(np.median(w.n_before)), nan_dE=int(np.isnan(out["dE"]).sum()))
    run = best = 0
    for n in w.n_before:
        run = run + 1 if n == 0 else 0
        best = max(best, run)
    c["longest_empty_run"] = best
    for i in range(10):
        if kd.p_kernel[i] <= 0:
            assert not (k == i).any()
            continue
        sel = (k == i) if i in (K.K_UBIRTH, K.K_DBIRTH) else (k == i) & has_t
        if i == K.K_MERGE:
            sel = sel & (p["param_id"] >= 0)
        c[f"proposed_{K.KERNEL_NAMES[i]}"] = int(sel.sum())
        c[f"accepted_{K.KERNEL_NAMES[i]}"] = int((sel & acc).sum())
    # data-driven translations: the clipped window around the target's pixel
    dt = np.nonzero((k == K.K_DTRANS) & has_t)[0]
    long_side = corner = spans = own = 0
    for i in dt:
        x, y = w.before[i][0][p["target"][i]]
        x0, x1, y0, y1 = max(0, x - md), min(x + md + 1, H), max(0, y - md), min(y + md + 1, W)
        long_side += max(x1 - x0, y1 - y0) > 17
        corner += (x0 == 0 or x1 == H) and (y0 == 0 or y1 == W)
        spans += (x1 - x0 == H) if H <= W else (y1 - y0 == W)
        own += (p["ax"][i] == x and p["ay"][i] == y)
    c.update(dtrans=len(dt), dtrans_window_over_17=int(long_side), dtrans_corner=int(corner), dtrans_spans_short_side=int(spans),
             dtrans_own_pixel=int(own))
    db = k == K.K_DBIRTH
    c["dbirth_beyond_512"] = int((db & ((p["ax"] if H >= W else p["ay"]) >= 512)).sum())
    # Gaussian transforms: the range ends of clamped marks, the wraps of cyclic ones
    gt = np.nonzero((k == K.K_GTRANSF) & has_t)[0]
    new = np.stack([p["as"], p["ar"], p["aa"]], axis=1)
    for j, m in enumerate(maps):
        idx = gt[p["param_id"][gt] == j]
        if m.is_cyclic:
            old = np.array([w.before[i][1][p["target"][i], j] for i in idx]).reshape(-1)
            moved = old + p["aux0"][idx]
            c[f"gtransf_wraps_{j}"] = int(((moved < m.v_min) | (moved >= m.v_max)).sum())
        else:
            c[f"gtransf_at_range_end_{j}"] = int(((new[idx, j] == m.v_min) | (new[idx, j] == m.v_max)).sum())
    # proposals with a mark in a class that a linspace over the range gets wrong
    has_add = ~np.isin(k, (K.K_UDEATH, K.K_DDEATH, K.K_SPLIT, K.K_MERGE)) & (has_t | np.isin(k, (K.K_UBIRTH, K.K_DBIRTH)))
    differs = np.zeros(len(k), bool)
    for j, m in enumerate(maps):
        differs |= linspace_class(m, new[:, j]) != table_class(m, new[:, j])
    c["proposals_off_the_linspace_class"] = int((differs & has_add).sum())
    return c
