"""Dataset translation: a raw DOTA or COWC download -> ``<dataset_path>/<name>/<subset>/{raw_images,images,raw_annotations,
annotations,metadata,images_w_annotations}``, the layout every other step reads (``paths.fetch_data_paths``).

Mirrors the reference's ``data/translation/translate_DOTA.py`` and ``translate_COWC.py`` (same config keys, same files, names
``f"{id:04}"``), with the image work -- skimage 0.18.1 ``rescale(image, scale, anti_aliasing=True, multichannel=True)`` to the
target ground sampling distance, then ``plt.imsave`` -- done by ``MppContext.rescale`` on the GPU (``csrc/mpp_rescale.hip``).
The host part here is numpy only: selection, annotations, and the two tap tables into which the Gaussian blur and the
bilinear interpolation of each axis are folded.  There is no CPU path for the pixels.
"""
from __future__ import annotations

import glob
import json
import os
import pickle
import re
import shutil
import time
import warnings
from concurrent.futures import ThreadPoolExecutor
from datetime import datetime
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .paths import find_existing_path, get_dataset_base_path, make_if_not_exist
from .shapes import polygon_to_abw

SCALE_ACCEPTABLE_DELTA = 1e-2

ALL_CATEGORIES = ['large-vehicle', 'roundabout', 'plane', 'tennis-court', 'helipad', 'airport', 'small-vehicle',
                  'baseball-diamond', 'harbor', 'bridge', 'swimming-pool', 'storage-tank', 'helicopter',
                  'container-crane', 'soccer-ball-field', 'basketball-court', 'ship', 'ground-track-field']
SUB_FOLDERS = ['raw_images', 'images', 'raw_annotations', 'annotations', 'metadata', 'images_w_annotations']
COWC_GSD = 0.15

_DATE = re.compile(r'acquisition dates?:([^\n]*)')
_SOURCE = re.compile(r'imagesource:([^\n]*)')
_GSD = re.compile(r'gsd:([^\n]*)')


# ---- the rescale: output shape and tap tables ------------------------------------------------------------------------------
def rescale_output_shape(H: int, W: int, scale: float) -> Tuple[int, int]:
    """``np.round(scale * (H, W))``, half to even, as skimage's ``rescale`` sizes its output"""
    oh, ow = np.round(scale * np.array([H, W], dtype=np.float64)).astype(int)
    return int(oh), int(ow)


def gaussian_weights(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """the weights of ``scipy.ndimage.gaussian_filter1d``: radius ``int(truncate * sigma + 0.5)``, normalised by their sum"""
    radius = int(truncate * float(sigma) + 0.5)
    if radius == 0 or sigma <= 0:
        return np.ones(1)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def rescale_tables(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """One axis of the anti-aliased rescale as (index [n_out,T] int32, weight [n_out,T] float64), T = 2 radius + 2:
    output i = sum_t weight[i,t] * input[index[i,t]] is the bilinear sample at f (i + 0.5) - 0.5, f = n_in / n_out, of the
    input blurred with sigma = (f - 1) / 2 (``mode='mirror'``, ``truncate=4``).  Needs n_out <= n_in (scale <= 1): the
    sample points then lie inside the input and the interpolation needs no boundary rule."""
    if not 0 < n_out <= n_in:
        raise ValueError(f"rescale_tables: {n_in} -> {n_out} is not a reduction")
    f = n_in / n_out
    g = gaussian_weights(max(0.0, (f - 1) / 2))
    radius = (len(g) - 1) // 2
    x = f * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5
    i0 = np.floor(x).astype(np.int64)
    a = x - i0
    T = 2 * radius + 2
    w = np.zeros((n_out, T), dtype=np.float64)
    w[:, :T - 1] += (1.0 - a)[:, None] * g[None, :]       # the blurred sample at i0 ...
    w[:, 1:] += a[:, None] * g[None, :]                   # ... and the one at i0 + 1
    idx = i0[:, None] - radius + np.arange(T)[None, :]
    if n_in > 1:                                          # scipy's 'mirror': d c b | a b c d | c b a
        period = 2 * (n_in - 1)
        idx = np.mod(idx, period)
        idx = np.where(idx >= n_in, period - idx, idx)
    else:
        idx = np.zeros_like(idx)
    return np.ascontiguousarray(idx, dtype=np.int32), w


def rescale_image_tables(H: int, W: int, scale: float):
    """(oh, ow) and the (row_idx, row_w, col_idx, col_w) of ``MppContext.rescale`` for an H x W image"""
    oh, ow = rescale_output_shape(H, W, scale)
    if not (0 < oh <= H and 0 < ow <= W):
        raise ValueError(f"rescale: a {H} x {W} picture at scale {scale:.6g} would become {oh} x {ow}: "
                         + ("it is too small for that scale" if oh <= 0 or ow <= 0 else "only reductions are built"))
    return (oh, ow), rescale_tables(H, oh) + rescale_tables(W, ow)


# ---- annotations -----------------------------------------------------------------------------------------------------------
def parse_label_text(text: str):
    """rows ``x1 y1 x2 y2 x3 y3 x4 y4 category difficult`` -> (coords [n,8] float64, categories [n] object, difficult [n]
    int64); lines of another form (the two header lines of DOTA-v1 label files) are skipped"""
    coords, cats, diff = [], [], []
    for line in text.splitlines():
        p = line.split(' ')
        if len(p) != 10:
            continue
        try:
            c, d = [float(v) for v in p[:8]], int(p[9])
        except ValueError:
            continue
        coords.append(c)
        cats.append(p[8])
        diff.append(d)
    cat = np.empty(len(cats), dtype=object)
    cat[:] = cats
    return np.array(coords, dtype=np.float64).reshape(-1, 8), cat, np.array(diff, dtype=np.int64)


def count_objects(text: str, categories: Sequence[str]) -> Dict[str, int]:
    _, cat, _ = parse_label_text(text)
    return {c: int(np.sum(cat == c)) for c in categories}


def dota_annotations(text: str, categories: Sequence[str], scale: float) -> Dict[str, np.ndarray]:
    """The annotation pickle of one image (``translate_DOTA.py:136-192``): corners as (y, x), truncated mean centres,
    both scaled if the image is, (a, b, angle) per object."""
    coords, cat, diff = parse_label_text(text)
    keep = np.isin(cat, list(categories))
    coords, cat, diff = coords[keep], cat[keep], diff[keep]
    polygons = np.stack((coords[:, 1::2], coords[:, 0::2]), axis=-1)          # [n,4,(y,x)]
    centers = np.mean(polygons, axis=1).astype(int)
    if abs(1 - scale) > SCALE_ACCEPTABLE_DELTA:
        assert scale <= 1
        polygons = polygons * scale
        centers = (centers * scale).astype(int)
    if len(centers) == 0:
        e = np.array([])
        return {'centers': e, 'parameters': e.copy(), 'categories': e.copy(), 'difficult': e.copy()}
    return {'centers': centers, 'parameters': polygon_to_abw(polygons), 'categories': cat, 'difficult': diff}


def cowc_annotations(annotation: np.ndarray, scale: float) -> Dict[str, np.ndarray]:
    """``translate_COWC.py:45-62``: one 4 x 4 'vehicle' per non-zero pixel of the annotation image"""
    centers = np.array(np.where(np.any(annotation > 0, axis=-1))).T
    centers = (centers * scale).astype(int)
    n = len(centers)
    cat = np.empty(n, dtype=object)
    cat[:] = 'vehicle'
    if n == 0:
        return {'centers': np.array([]), 'parameters': np.array([]), 'categories': np.array([]), 'difficult': np.zeros(0)}
    return {'centers': centers, 'parameters': np.tile(np.array([4.0, 4.0, 0.0]), (n, 1)), 'categories': cat.astype(str),
            'difficult': np.zeros(n)}


# ---- selection -------------------------------------------------------------------------------------------------------------
def parse_meta_text(text: str, where: str = "meta"):
    """(date string, source or None, gsd or None) from the first three lines of a DOTA meta file"""
    lines = text.splitlines()
    m = [p.match(lines[i]) if i < len(lines) else None for i, p in enumerate((_DATE, _SOURCE, _GSD))]
    if any(v is None for v in m):
        raise ValueError(f"{where}: expected 'acquisition dates:', 'imagesource:' and 'gsd:' lines")
    date, source, gsd = (v.group(1) for v in m)
    try:
        gsd = float(gsd)
    except ValueError:
        gsd = None
    try:
        from dateutil import parser as date_parser
        date = str(date_parser.parse(date, default=datetime(1, 1, 1))) if date.strip() else "NaT"
    except (ValueError, OverflowError):
        date = "NaT"
    return date, (None if source == 'None' else source), gsd


def _by_id(pattern: str, ext: str) -> Dict[int, str]:
    out = {}
    for p in glob.glob(pattern):
        m = re.search(r'P([0-9]+)\.' + ext + '$', os.path.basename(p))
        if m:
            out[int(m.group(1))] = p
    return out


def fetch_dota_paths(base_path: str, subset: str) -> List[Dict[str, Any]]:
    """images/P*.png, DOTA-v2.0_<subset>/P*.txt and meta/P*.txt paired by id, sorted by id, with the parsed meta"""
    assert subset in ['train', 'val']
    images = _by_id(os.path.join(base_path, subset, 'images', 'P*.png'), 'png')
    labels = _by_id(os.path.join(base_path, subset, f'DOTA-v2.0_{subset}', 'P*.txt'), 'txt')
    metas = _by_id(os.path.join(base_path, subset, 'meta', 'P*.txt'), 'txt')
    rows = []
    for i in sorted(set(images) & set(labels) & set(metas)):
        with open(metas[i], 'r') as f:
            date, source, gsd = parse_meta_text(f.read(), metas[i])
        rows.append({'id': i, 'path_image': images[i], 'path_label': labels[i], 'path_meta': metas[i], 'date': date,
                     'source': source, 'gsd': gsd})
    return rows


def drop_images(rows: List, drop_rate: float, rng_seed: int = 0) -> List:
    """the reference's draw: ``default_rng(seed).choice(range(n), size=int(n * (1 - drop_rate)), replace=False)``, sorted"""
    if not drop_rate > 0:
        return rows
    assert drop_rate < 1.0
    n = len(rows)
    kept = np.random.default_rng(rng_seed).choice(range(n), size=int(n * (1 - drop_rate)), replace=False)
    kept.sort()
    return [rows[i] for i in kept]


def select_dota(rows: List[Dict[str, Any]], categories: Sequence[str], target_gsd: float, prune_empty: bool, drop_rate: float = 0.0,
                banned_sources: Optional[Sequence[str]] = None, rng_seed: int = 0) -> List[Dict[str, Any]]:
    """``translate_DOTA.py:213-264`` on rows sorted by id; a row needs 'counts' {category: n} besides what
    ``fetch_dota_paths`` gives.  Adds scale, n_objects and sample_density."""
    for c in categories:
        assert c in ALL_CATEGORIES, c
    rows = sorted(rows, key=lambda r: r['id'])
    if banned_sources is not None:
        sources = {r['source'] for r in rows}
        for s in banned_sources:
            if s not in sources:
                warnings.warn(f"source {s} does not exist ({sorted(str(v) for v in sources)})")
        rows = [r for r in rows if r['source'] not in banned_sources]
    rows = [dict(r, scale=r['gsd'] / target_gsd) for r in rows if r['gsd'] is not None and r['gsd'] <= target_gsd]
    for r in rows:
        r['n_objects'] = int(sum(r['counts'][c] for c in categories))
    total = sum(r['n_objects'] for r in rows)
    for r in rows:
        r['sample_density'] = r['n_objects'] / total if total else 0.0
    if prune_empty:
        rows = [r for r in rows if r['n_objects'] > 0]
    return drop_images(rows, drop_rate, rng_seed)


def fetch_cowc_paths(data_path: str) -> List[Dict[str, Any]]:
    png = glob.glob(os.path.join(data_path, '*/*.png'))
    annotations = sorted(s for s in png if re.match(r'(.*)_Annotated_Cars.png', s))
    images = sorted(s for s in png if not re.match(r'(.*)((?:_Annotated_Cars)|(?:_Annotated_Negatives)).png', s))
    if len(images) != len(annotations):
        raise ValueError(f"{data_path}: {len(images)} images but {len(annotations)} *_Annotated_Cars.png files")
    return [{'id': i, 'path_image': im, 'path_label': an, 'gsd': COWC_GSD} for i, (im, an) in enumerate(zip(images, annotations))]


# ---- images ----------------------------------------------------------------------------------------------------------------
def read_rgb(path: str) -> np.ndarray:
    """a PNG as uint8 [H,W,3]; alpha is dropped, anything that is not 3-channel 8-bit after that raises"""
    from PIL import Image
    with Image.open(path) as im:
        a = np.array(im)
    if a.ndim == 3 and a.shape[2] == 4:
        a = a[:, :, :3]
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError(f"{path}: expected an 8-bit image of 3 channels, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def write_rgb(path: str, a: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(a, mode="RGB").save(path, format="PNG")


def _read_annotation_image(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    return a if a.ndim == 3 else a[:, :, None]


class _Translator:
    """Decode and encode in a thread pool (PIL releases the GIL), the device work on the calling thread: decode, kernel and
    encode of different images overlap.  ``timings`` gets one dict of seconds per image."""

    def __init__(self, device: int, workspace_limit: Optional[int] = None):
        import torch
        from . import hip_api
        self.torch, self.hip_api = torch, hip_api
        self.ctx = hip_api.MppContext(device)                      # no GPU: MppError, there is no CPU path for the pixels
        self.dev = torch.device("cuda", device)
        self.ctx.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
        self.workspace_limit = workspace_limit or hip_api.RESCALE_WORKSPACE
        self.workers = min(16, os.cpu_count() or 1)
        self.timings: List[Dict[str, float]] = []

    def rescale(self, raw: np.ndarray, scale: float, t: Dict[str, float]) -> np.ndarray:
        torch = self.torch
        if abs(1 - scale) <= SCALE_ACCEPTABLE_DELTA:
            return raw                                              # copied through, as in the reference
        if scale > 1:
            raise ValueError(f"scale {scale} > 1: only reductions are built")
        _, tables = rescale_image_tables(raw.shape[0], raw.shape[1], scale)
        c0 = time.perf_counter()
        src = torch.from_numpy(raw).to(self.dev)
        torch.cuda.synchronize(self.dev)
        c1 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = self.ctx.rescale(src, tables, workspace_limit=self.workspace_limit)
        e1.record()
        torch.cuda.synchronize(self.dev)
        c2 = time.perf_counter()
        res = out.cpu().numpy()
        t.update(upload=c1 - c0, kernel=e0.elapsed_time(e1) * 1e-3, download=time.perf_counter() - c2)
        return res

    def run(self, jobs: List[Dict[str, Any]], save_dir: str, annotate) -> None:
        """jobs: rows with id, path_image, path_label, scale, n_objects, info; annotate(row) -> the annotation dict"""
        def decode(row):
            c = time.perf_counter()
            a = read_rgb(row['path_image'])
            return a, time.perf_counter() - c

        def finish(row, image, t):
            c = time.perf_counter()
            name = f"{row['id']:04}"
            write_rgb(os.path.join(save_dir, 'images', name + '.png'), image)
            t['encode'] = time.perf_counter() - c
            shutil.copy(row['path_image'], os.path.join(save_dir, 'raw_images', name + '.png'))
            with open(os.path.join(save_dir, 'annotations', name + '.pkl'), 'wb') as f:
                pickle.dump(annotate(row), f)
            with open(os.path.join(save_dir, 'metadata', name + '.json'), 'w') as f:
                json.dump({'shape': list(image.shape), 'n_objects': int(row['n_objects']), 'scale': row['scale'], **row['info']},
                          f, indent=1)
            return t

        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            ahead = self.workers                                   # images decoded (or being encoded) besides the current one
            decoding = [pool.submit(decode, r) for r in jobs[:ahead]]
            finishing = []
            for k, row in enumerate(jobs):
                raw, dt = decoding[k].result()
                decoding[k] = None
                if k + ahead < len(jobs):
                    decoding.append(pool.submit(decode, jobs[k + ahead]))
                t = {'id': row['id'], 'decode': dt, 'upload': 0.0, 'kernel': 0.0, 'download': 0.0}
                image = self.rescale(raw, row['scale'], t)
                finishing.append(pool.submit(finish, row, image, t))
                if len(finishing) > ahead:
                    self.timings.append(finishing.pop(0).result())
            self.timings.extend(f.result() for f in finishing)


def _write_json(path: str, obj) -> None:
    with open(path, 'w') as f:
        json.dump(obj, f, indent=1)


def _prepare_dirs(name: str, config: Dict[str, Any], subsets: Sequence[str]) -> str:
    save_dir = os.path.join(get_dataset_base_path(), name)
    make_if_not_exist(save_dir)
    _write_json(os.path.join(save_dir, 'config.json'), config)
    for ss in subsets:
        make_if_not_exist(os.path.join(save_dir, ss))
        make_if_not_exist([os.path.join(save_dir, ss, s) for s in SUB_FOLDERS])
    return save_dir


def translate_dota(config: Dict[str, Any], device: int = 0, workspace_limit: Optional[int] = None) -> List[Dict[str, float]]:
    """``translate_DOTA.translate_dota`` with the reference's config keys; returns the per-image timings (seconds)."""
    subsets, categories = config["subsets"], config["categories"]
    drop_rate = config.get('drop_rate') or {ss: 0.0 for ss in subsets}
    for ss in subsets:
        assert ss in ['train', 'val'], ss                          # 'test' has no labels: not built, as in the reference
    tr = _Translator(device, workspace_limit)
    source_base = find_existing_path(config["dota_base_path"])
    save_dir = _prepare_dirs(config["name"], config, subsets)
    for ss in subsets:
        print(f'making {ss} patches')
        rows = fetch_dota_paths(source_base, ss)
        texts = {}
        for r in rows:
            with open(r['path_label'], 'r') as f:
                texts[r['id']] = f.read()
            r['counts'] = count_objects(texts[r['id']], categories)
        n_prev = len(rows)
        rows = select_dota(rows, categories, config["target_gsd"], bool(config["prune_empty"]), drop_rate[ss],
                           config["banned_sources"])
        print(f'{len(rows)} of {n_prev} images kept (gsd <= {config["target_gsd"]}, banned sources, '
              f'{"" if config["prune_empty"] else "not "}pruning empty images, drop rate {drop_rate[ss]:.2%})')
        sub_dir = os.path.join(save_dir, ss)
        _write_json(os.path.join(sub_dir, 'paths_and_meta.json'), rows)
        for r in rows:
            r['info'] = {'original_gsd': r['gsd'], 'source': r['source'], 'date': r['date']}
            shutil.copy(r['path_label'], os.path.join(sub_dir, 'raw_annotations', f"{r['id']:04}.txt"))
            if r['n_objects'] == 0:
                print(f"[warning] {categories} not in image {r['path_image']}")
        tr.run(rows, sub_dir, lambda r: dota_annotations(texts[r['id']], categories, r['scale']))
    return tr.timings


def translate_cowc(config: Dict[str, Any], device: int = 0, workspace_limit: Optional[int] = None) -> List[Dict[str, float]]:
    """``translate_COWC.translate_cowc`` with the reference's config keys (subset 'val' only, every image rescaled)."""
    tr = _Translator(device, workspace_limit)
    source_base = find_existing_path(config["cowc_base_path"])
    save_dir = _prepare_dirs(config["name"], config, ['val'])
    rows = fetch_cowc_paths(source_base)
    print(f"found {len(rows)} images")
    scale = COWC_GSD / config["target_gsd"]
    if abs(1 - scale) <= SCALE_ACCEPTABLE_DELTA:
        # the reference rescales every COWC image; at a scale this close to 1 that is a resampling of its own, not built
        raise ValueError(f"target_gsd {config['target_gsd']} is the COWC gsd {COWC_GSD}: nothing to translate")
    with ThreadPoolExecutor(max_workers=tr.workers) as pool:
        annotations = list(pool.map(lambda r: cowc_annotations(_read_annotation_image(r['path_label']), scale), rows))
    for r, a in zip(rows, annotations):
        r.update(scale=scale, n_objects=int(len(a['centers'])), info={'original_gsd': r['gsd']})
    total = sum(r['n_objects'] for r in rows)
    for r in rows:
        r['sample_density'] = r['n_objects'] / total if total else 0.0
    by_id = {r['id']: a for r, a in zip(rows, annotations)}
    if bool(config["prune_empty"]):
        rows = [r for r in rows if r['n_objects'] > 0]
    rows = drop_images(rows, config['drop_rate'])
    sub_dir = os.path.join(save_dir, 'val')
    _write_json(os.path.join(sub_dir, 'paths_and_meta.json'), [{k: v for k, v in r.items() if k != 'info'} for r in rows])
    tr.run(rows, sub_dir, lambda r: by_id[r['id']])
    return tr.timings
