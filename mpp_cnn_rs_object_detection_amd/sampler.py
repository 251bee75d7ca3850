"""RJMCMC sampling driver: ``sample_rjmcmc`` and its batched, GPU-native form.

Mirrors the reference's ``models/mpp/rjmcmc_sampler/sample_rjmcmc.py:23-102`` (same signature,
same schedule arithmetic, same "which state is returned" rule) while running the chain of every
tile in ONE kernel launch, one workgroup per tile (``libmppgpu.so``: ``mpp_run``).

Differences a caller can observe (both documented in DESIGN.md):

* the proposal stream is Philox4x32-10 keyed by a seed drawn from the given ``rng`` (the reference
  consumes the NumPy generator directly and is not reproducible run to run);
* with ``use_split_merge`` the kernel needs ``spec_waves`` 1 or 8 (split / merge steps run alone on the live state).
"""
from __future__ import annotations

import logging
import time
from typing import List, Optional, Sequence, Union

import numpy as np

from . import energies as E
from .custom_types import ImageWMaps
from .hip_api import MppContext
from .kernels import make_kernels
from .shapes import Rectangle

NMS_DISTANCE = 6.0      # reference sample_rjmcmc.py:27


def _to_rectangles(xy: np.ndarray, marks: np.ndarray) -> List[Rectangle]:
    # (.tolist() first: building 5 000 rectangles from NumPy scalars took 54 ms of a 0.26 s scene, from Python numbers 8 ms)
    return [Rectangle(x, y, size=s, ratio=r, angle=a) for (x, y), (s, r, a) in zip(xy.tolist(), marks.tolist())]


def resolve_schedule(num_samples: int, init_temperature: float, alpha_t, burn_in, samples_interval,
                     target_temperature: float, iter_multiplier=None):
    """The reference's schedule arithmetic (``sample_rjmcmc.py:58-66,78`` and ``stopping.py:41-42``).

    Returns (alpha, T_target, total_steps, snapshot_step): the chain runs ``max_iter + 1`` steps and the
    configuration handed back is the one after the last step t with t >= burn_in and
    t % samples_interval == 0 (``rjmcmc.py:138-141``), or the final one if no such step exists."""
    if iter_multiplier is not None:
        burn_in = burn_in * iter_multiplier
        samples_interval = samples_interval * iter_multiplier
        alpha_t = np.power(alpha_t, 1 / iter_multiplier)
    if isinstance(alpha_t, str):
        if alpha_t != "auto":
            raise ValueError("alpha_t must be a number or 'auto'")
        alpha_t = float(np.power(target_temperature / init_temperature, 1 / burn_in))
        target_temperature = 0
    burn_in, samples_interval = int(burn_in), int(samples_interval)
    max_iter = burn_in + (num_samples + 1) * samples_interval
    total = max_iter + 1
    snaps = [t for t in range(burn_in, total) if samples_interval > 0 and t % samples_interval == 0]
    return float(alpha_t), float(target_temperature), total, snaps


#: relative speed of ONE chain with 8 / 4 / 2 / 1 waves in deep rounds (csrc/mpp_deep.hip; the 512-px bench tile: 117 / 131 /
#: 177 / 218 ms per 100 001 steps, gpurun_out of round 3; one wave per step, round 1: 1.0 / 0.74 / 0.47 / 0.30)
SPEC_SPEED = {8: 1.0, 4: 0.89, 2: 0.66, 1: 0.54}
#: ... and with one wave per step (the kernels chains with the split / merge kernels run on): profiles/r01_batched_sweep.json
SPEC_SPEED_WAVE = {8: 1.0, 4: 0.74, 2: 0.47, 1: 0.30}
LDS_PER_CU, WAVES_PER_CU, N_CU = 160 * 1024, 8, 256      # MI355X; 8 waves of 256 VGPRs fill a CU


def choose_spec_waves(ctx: MppContext, n_tiles: int, use_split_merge: bool = False) -> int:
    """Speculative waves per chain for a launch of ``n_tiles`` chains: fewer waves per chain let more chains share a
    CU -- if their LDS footprint (set by the point capacity) allows it.  Minimises rounds-of-workgroups / chain speed.
    With the default capacity of 1024 slots one chain fills a CU's LDS and 8 waves are always best; with 128 slots the
    measured optimum is 8 waves up to 256 tiles, 4 up to 512, 2 up to 1024, 1 beyond (same sweep)."""
    best, best_t = 8, None
    for spec in ((8, 1) if use_split_merge else (8, 4, 2, 1)):
        ctx.set_option("spec_waves", spec)
        lds = max(1, ctx.get_option("lds_bytes"))
        resident = N_CU * max(1, min(LDS_PER_CU // lds, WAVES_PER_CU // spec))
        t = -(-n_tiles // resident) / (SPEC_SPEED_WAVE if use_split_merge else SPEC_SPEED)[spec]
        if best_t is None or t < best_t - 1e-12:
            best, best_t = spec, t
    return best


def replica_chain_ids(n_tiles: int, restarts: int, chain0: int = 0) -> np.ndarray:
    """Chain ids of the ``restarts`` replicas of an image's ``n_tiles`` tiles, uint32 ``[restarts * n_tiles]`` in the
    context's chain order (chain ``r * n_tiles + i``): replica ``r`` of tile ``i`` draws from ``chain0 + i + r * n_tiles``.
    ``n_tiles`` is the tile count of the whole image, so no two chains of an image share an id and replica 0 keeps the id
    the tile has without restarts."""
    n_tiles, restarts, chain0 = int(n_tiles), int(restarts), int(chain0)
    if n_tiles < 0 or restarts < 1 or chain0 < 0:
        raise ValueError(f"replica_chain_ids: n_tiles {n_tiles}, restarts {restarts}, chain0 {chain0}")
    if n_tiles and chain0 + restarts * n_tiles - 1 > 2 ** 32 - 1:
        raise ValueError(f"replica_chain_ids: chain id {chain0 + restarts * n_tiles - 1} does not fit 32 bits "
                         f"({restarts} restarts of {n_tiles} tiles from chain {chain0})")
    return (chain0 + np.arange(restarts * n_tiles, dtype=np.int64)).astype(np.uint32)


def select_replicas(energy, n_tiles: int) -> np.ndarray:
    """The winning replica of every tile, int64 ``[n_tiles]``, from the chains' energies ``[restarts * n_tiles]`` (chain
    ``r * n_tiles + i``) or ``[restarts, n_tiles]``.  Per tile the walk starts at replica 0; replica ``r`` replaces the
    best so far when its energy is strictly lower, or when the best is not finite and ``r``'s is: ties go to the lowest
    replica, a non-finite energy never beats a finite one, and replica 0 wins when none is finite."""
    n_tiles = int(n_tiles)
    e = np.asarray(energy, dtype=np.float64).reshape(-1, n_tiles) if n_tiles else np.zeros((1, 0))
    if e.shape[0] < 1:
        raise ValueError("select_replicas: no energies")
    best, best_e = np.zeros(n_tiles, np.int64), e[0].copy()
    with np.errstate(invalid="ignore"):
        for r in range(1, e.shape[0]):
            take = (e[r] < best_e) | (~np.isfinite(best_e) & np.isfinite(e[r]))
            best[take], best_e[take] = r, e[r][take]
    return best


#: ``tempering`` defaults: the factor between the schedules of neighbouring rungs (the swept value with the lowest mean winner
#: energy at R = 4, every 4096 -- which still is no lower than that of plain restarts: profiles/tempering.md) and the steps
#: between two exchanges (the shortest interval whose segments still get a hot start)
TEMPERING_RATIO, TEMPERING_EVERY = 1.25, 4096


def resolve_tempering(tempering, restarts: int):
    """``None`` / ``False`` -> None; ``True`` or ``{"ratio": r, "every": K}`` (either key optional) -> ``(ratio, every)``.
    Raises ``ValueError`` for fewer than two restarts, a ratio below 1 or not finite, an interval below 1, unknown keys."""
    if tempering is None or tempering is False:
        return None
    opts = {} if tempering is True else tempering
    if not isinstance(opts, dict) or set(opts) - {"ratio", "every"}:
        raise ValueError(f"tempering must be true or a mapping with 'ratio' and / or 'every', got {tempering!r}")
    if int(restarts) < 2:
        raise ValueError(f"tempering exchanges the replicas of a tile: it needs restarts >= 2, got {restarts}")
    ratio, every = opts.get("ratio", TEMPERING_RATIO), opts.get("every", TEMPERING_EVERY)
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not np.isfinite(ratio) or ratio < 1:
        raise ValueError(f"tempering: ratio must be a finite number >= 1, got {ratio!r}")
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError(f"tempering: every must be an integer >= 1, got {every!r}")
    return float(ratio), int(every)


def rungs_after(log, n_tiles: int, restarts: int) -> np.ndarray:
    """The rung of every chain, int64 ``[restarts, n_tiles]``, after the exchanges of ``log`` (records of
    ``EXCHANGE_RECORD_DTYPE`` from the ladder's start on): replica r starts on rung r, an accepted record swaps two."""
    rung = np.repeat(np.arange(restarts, dtype=np.int64), n_tiles)
    for a, b in zip(log["chain_a"][log["accepted"] != 0].tolist(), log["chain_b"][log["accepted"] != 0].tolist()):
        rung[a], rung[b] = rung[b], rung[a]
    return rung.reshape(restarts, n_tiles)


def exchange_rates(log, restarts: int) -> np.ndarray:
    """accepted / attempted per pair of neighbouring rungs, float64 ``[restarts - 1]`` (NaN: a pair never attempted)"""
    tried = np.bincount(log["k"], minlength=restarts - 1).astype(np.float64)
    took = np.bincount(log["k"], weights=(log["accepted"] != 0), minlength=restarts - 1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(tried > 0, took / tried, np.nan)


class TileBatchSampler:
    """All tiles of an image (or of a batch of images) sampled concurrently on one GPU."""

    def __init__(self, tiles: Sequence[ImageWMaps], energy_setup, energy_combinator, device: int = 0,
                 point_capacity: int = 1024, spec_waves: Optional[int] = 8, ctx: Optional[MppContext] = None,
                 use_split_merge: bool = False, keys=None, stacked_maps=None, restarts: int = 1, tempering=None,
                 recombine: bool = False):
        """``keys`` = (seeds, chain ids), one per tile: the Philox key and chain id each tile's chain uses instead of the
        launch's seed and ``chain0 + tile`` -- tiles of several images in one launch keep the chains they would run in a
        launch of their own image (``mpp_set_chain_keys``).

        ``restarts`` R > 1: R independent chains per tile (the context's ``replicas``), all from the tile's initial
        configuration; replica r of a tile draws from the chain id ``replica_chain_ids`` gives it (replica 0: the tile's
        own), and ``run`` hands back, per tile, the replica whose returned state has the lowest total energy
        (``select_replicas``; kept in ``replica_energy`` [R, n_tiles] and ``replica_winner`` [n_tiles]).  With ``keys`` of
        several images a third entry gives, per tile, the tile count of its image (the images' tiles in order): replica
        ids are per image.

        ``tempering`` = ``True`` or ``{"ratio": r, "every": K}`` (needs ``restarts`` >= 2): parallel tempering.  Replica r of
        a tile starts on rung r of a temperature ladder (its schedule ``ratio ** r`` times hotter) and every K steps
        neighbouring rungs of a tile exchange their schedules by a Metropolis test (``MppContext.run_tempered``).  The
        returned state is chosen as for restarts.  ``run`` keeps ``replica_rung`` [R, n_tiles] (the rungs at the returned
        state), ``exchange_log`` and ``exchange_rate`` [R - 1].  ``None``: the replicas never interact.

        ``recombine`` (needs ``restarts`` >= 2): the returned state of a tile is not its winning replica as a whole but, for
        every interaction cluster of the union of the replicas' points, the replica that spends the least energy there
        (``MppContext.recombine``) -- in real arithmetic never a higher energy than the winner's.
        ``replica_energy`` is that of the replicas as sampled, ``replica_winner`` the whole-tile winner (whose chain holds
        the composite afterwards), ``recombine_report`` the call's records.  Works with ``tempering``."""
        self.use_split_merge = use_split_merge
        self.restarts = int(restarts)
        if self.restarts < 1:
            raise ValueError(f"restarts must be >= 1, got {restarts}")
        self.recombine = bool(recombine)
        if self.recombine and self.restarts < 2:
            raise ValueError(f"recombine chooses among the restarts of a tile: it needs restarts >= 2, got {restarts}")
        self.replica_energy = self.replica_winner = self.recombine_report = None
        self.tempering = resolve_tempering(tempering, self.restarts)
        self.replica_rung = self.exchange_log = self.exchange_rate = None
        shapes = {tuple(t.shape[:2]) for t in tiles}
        if len(shapes) != 1:
            raise ValueError(f"all tiles of a batch must have the same shape, got {shapes}")
        self.tiles = list(tiles)
        self.energy_setup = energy_setup
        self.energy_combinator = energy_combinator
        self.mappings = tiles[0].mappings
        unit, pair = energy_setup.make_energies(tiles[0])
        self.model_units = unit
        self.model = E.build_model_desc(unit, pair, energy_combinator)
        auto_spec = spec_waves is None
        if self.restarts > 1:
            if ctx is not None and ctx.get_option("replicas") != self.restarts:
                raise ValueError(f"restarts={self.restarts}: the given context holds {ctx.get_option('replicas')} replica(s)")
            self.ctx = ctx or MppContext(device, point_capacity=point_capacity, spec_waves=8 if auto_spec else spec_waves,
                                         replicas=self.restarts)
        else:
            self.ctx = ctx or MppContext(device, point_capacity=point_capacity, spec_waves=8 if auto_spec else spec_waves)
        det0 = tiles[0].detection_map
        if stacked_maps is not None:                  # (det [T,p,p], marks 3 x [T,p,p,32]) already stacked on the GPU
            det, marks = stacked_maps
            if int(det.shape[0]) != len(tiles):
                raise ValueError("stacked_maps: one slice per tile")
        elif hasattr(det0, "data_ptr"):                 # maps already on the GPU (U-Net epilogue output)
            import torch
            det = torch.stack([t.detection_map for t in tiles]).contiguous()
            marks = [torch.stack([t.param_dist_maps[k] for t in tiles]).contiguous() for k in range(3)]
        else:
            det = np.stack([np.asarray(t.detection_map, dtype=np.float32) for t in tiles])
            marks = [np.stack([np.asarray(t.param_dist_maps[k], dtype=np.float32) for t in tiles]) for k in range(3)]
        self.ctx.set_maps(det, marks)
        if E.classic_image(unit) is not None:
            # a classic image energy (contrast setup): every tile brings its own picture, prepared as the setup prescribes
            self.ctx.set_image(np.stack([E.classic_image(energy_setup.make_energies(t)[0]) for t in tiles]))
            if spec_waves not in (1, 8):
                auto_spec = False
                self.ctx.set_option("spec_waves", 8)
        self._replica_keys = None                     # restarts > 1 with ``keys``: (seeds, chain ids) of all chains
        if keys is not None and self.restarts > 1:
            self._replica_keys = self._keys_of_replicas(keys)
        elif keys is not None:
            self.ctx.set_chain_keys(keys[0], keys[1])
        self.ctx.set_model(self.model, self.mappings)
        if auto_spec and ctx is None:
            self.ctx.set_option("spec_waves", choose_spec_waves(self.ctx, len(self.tiles) * self.restarts, use_split_merge))

    def _keys_of_replicas(self, keys):
        """(seeds, chain ids) of every chain from the per-tile ``keys`` = (seeds, chain ids, tiles of the tile's image)"""
        n, R = len(self.tiles), self.restarts
        if len(keys) < 3:
            raise ValueError("restarts > 1 with keys: a third entry gives each tile's image's tile count")
        seeds = np.asarray(keys[0], dtype=np.uint64).reshape(-1)
        chains = np.asarray(keys[1], dtype=np.int64).reshape(-1)
        per_image = np.asarray(keys[2], dtype=np.int64).reshape(-1)
        if not (len(seeds) == len(chains) == len(per_image) == n):
            raise ValueError("keys: one seed, one chain id and one tile count per tile")
        out = np.zeros((R, n), np.uint32)
        i = 0
        while i < n:                                   # image after image: its tiles are consecutive, ids chain0 + 0..m-1
            m = int(per_image[i])
            if m < 1 or i + m > n or np.any(chains[i:i + m] != chains[i] + np.arange(m)) or np.any(per_image[i:i + m] != m):
                raise ValueError("keys: the tiles of an image must be consecutive with consecutive chain ids")
            out[:, i:i + m] = replica_chain_ids(m, R, int(chains[i])).reshape(R, m)
            i += m
        return np.tile(seeds, R), out.reshape(-1)

    def init(self, init_config: Union[str, None, Sequence[Sequence[Rectangle]]]):
        n = len(self.tiles)
        if isinstance(init_config, str) and init_config == "naive":
            self.ctx.naive_init(self.energy_setup.detection_threshold, NMS_DISTANCE)
        else:
            if isinstance(init_config, str) and init_config == "gt":
                configs = [t.gt_config for t in self.tiles]
            elif init_config is None:
                configs = [[] for _ in range(n)]
            else:
                configs = list(init_config)
                if configs and isinstance(configs[0], Rectangle):
                    configs = [configs] * n
            for i, cfg in enumerate(configs):
                xy = np.array([[p.x, p.y] for p in cfg], dtype=np.int32).reshape(-1, 2)
                mk = np.array([[p.size, p.ratio, p.angle] for p in cfg], dtype=np.float64).reshape(-1, 3)
                for r in range(self.restarts):               # every replica starts where its tile starts
                    self.ctx.set_points(r * n + i, xy, mk)
        counts = self.ctx.counts()[:n].astype(np.float64)
        self.intensity = np.maximum(1.0, counts)             # reference sample_rjmcmc.py:68
        self.ctx.set_kernels(make_kernels(self.mappings, 1.0, use_split_merge=self.use_split_merge),
                             intensity=self.intensity if self.restarts == 1 else np.tile(self.intensity, self.restarts))

    def run(self, total_steps: int, snapshot_steps: Sequence[int], num_samples: int, T0: float, alpha: float,
            T_target: float, seed: int, chain0: int = 0, on_device=None, as_arrays: bool = False):
        """-> per tile, the list of the last ``num_samples`` sampled configurations.
        ``on_device``: a callable ``f(ctx)`` that takes each sampled state where it lies (e.g.
        ``ctx.pack_detections`` into an all-gather buffer) instead of copying it to host rectangles.
        ``as_arrays``: configurations as (xy [n, 2] int32, marks [n, 3] float64) instead of lists of ``Rectangle``.
        With ``restarts`` > 1 each tile's configuration is that of its winning replica, chosen on the returned state."""
        n, R = len(self.tiles), self.restarts
        if R > 1:
            if num_samples > 1:
                raise ValueError("restarts > 1 with num_samples > 1: a winner is defined for one returned state")
            if on_device is not None:
                raise ValueError("restarts > 1: the winners are chosen on the host, on_device is not supported")
            if self._replica_keys is not None:
                self.ctx.set_chain_keys(*self._replica_keys)
            else:
                self.ctx.set_chain_keys(np.full(R * n, int(seed), np.uint64), replica_chain_ids(n, R, chain0))
        self.ctx.set_schedule(T0, alpha, T_target)
        if self.tempering:
            self.ctx.set_ladder(self.tempering[0])
            self._logs = []
        wanted = list(snapshot_steps)[-num_samples:] if snapshot_steps else []
        samples = [[] for _ in self.tiles]

        def take():
            if on_device is not None:
                on_device(self.ctx)
                return
            if self.recombine:
                # (the energies of the replicas as sampled, then the call that rewrites the winners' chains; they are read after it)
                self.replica_energy = self.ctx.total_energy_all().reshape(R, n)
                self.recombine_report = self.ctx.recombine()
                self.replica_winner = self.recombine_report["winner"].astype(np.int64)
            chains = self.ctx.get_points_all()
            if R > 1:
                if not self.recombine:
                    self.replica_energy = self.ctx.total_energy_all().reshape(R, n)
                    self.replica_winner = select_replicas(self.replica_energy, n)
                if self.tempering:
                    self.replica_rung = rungs_after(np.concatenate(self._logs), n, R)
                chains = [chains[int(r) * n + i] for i, r in enumerate(self.replica_winner)]
            for i, pts in enumerate(chains[:n]):
                samples[i].append(pts if as_arrays else _to_rectangles(*pts))

        done = 0
        self.kernel_ms = 0.0
        self.hbm_chains = 0                                    # chains that outgrew the LDS and ran in device memory
        for t in wanted:                                       # the state after step t = after t+1 steps
            self._run_resumable(t + 1 - done, seed, chain0)
            done = t + 1
            take()
        if done < total_steps:                                 # the reference keeps stepping to max_iter
            self._run_resumable(total_steps - done, seed, chain0)
        if not wanted:
            take()
        if self.tempering:
            self.exchange_log = np.concatenate(self._logs)
            self.exchange_rate = exchange_rates(self.exchange_log, R)
            self.tempering_ms = self.ctx.tempering_stats()["ms"]
        return samples

    def _run_resumable(self, n_steps: int, seed: int, chain0: int):
        if self.tempering:
            self._logs.append(self.ctx.run_tempered(n_steps, seed, chain0, every=self.tempering[1]))
        else:
            self.ctx.run(n_steps, seed, chain0)
        self.kernel_ms += self.ctx.last_kernel_ms()
        self.hbm_chains = max(self.hbm_chains, self.ctx.get_option("hbm_chains"))


def sample_rjmcmc_batch(tiles: Sequence[ImageWMaps], rng: np.random.Generator, num_samples: int, energy_combinator,
                        init_config, init_temperature: float, alpha_t, burn_in: int, energy_setup,
                        samples_interval: int, target_temperature: float, verbose: int = 0, iter_multiplier=None,
                        use_split_merge: bool = False, device: int = 0, spec_waves: int = 8,
                        point_capacity: int = 1024, chain0: int = 0, restarts: int = 1, tempering=None,
                        recombine: bool = False):
    """``sample_rjmcmc`` for many equally-shaped tiles at once; returns one result list per tile.
    ``restarts`` R > 1: R chains per tile, the configuration of the one with the lowest energy is returned.
    ``tempering``: those chains on a temperature ladder, with exchanges (``TileBatchSampler``).
    ``recombine``: the returned configuration takes every interaction cluster from its best replica (``TileBatchSampler``)."""
    resolve_tempering(tempering, restarts)
    if recombine and restarts < 2:
        raise ValueError(f"recombine chooses among the restarts of a tile: it needs restarts >= 2, got {restarts}")
    if restarts > 1 and num_samples > 1:
        raise ValueError("restarts > 1 with num_samples > 1: a winner is defined for one returned state")
    alpha, T_target, total, snaps = resolve_schedule(num_samples, init_temperature, alpha_t, burn_in, samples_interval,
                                                      target_temperature, iter_multiplier)
    sampler = TileBatchSampler(tiles, energy_setup, energy_combinator, device=device, spec_waves=spec_waves,
                               point_capacity=point_capacity, use_split_merge=use_split_merge, restarts=restarts,
                               tempering=tempering, recombine=recombine)
    sampler.init(init_config)
    seed = int(rng.integers(0, 2 ** 63 - 1))
    start = time.perf_counter()
    samples = sampler.run(total, snaps, num_samples, init_temperature, alpha, T_target, seed, chain0)
    end = time.perf_counter()
    logging.info(f"rjmcmc on {len(tiles)} tile(s) ran in {end - start:.2f}s ({(end - start) / total:.1e}s/iter, "
                 f"kernel {sampler.kernel_ms:.1f} ms) (int. {sampler.intensity.tolist()} | iter {total - 1} | "
                 f"num_samples {num_samples})")
    return samples


def sample_rjmcmc(image_data: ImageWMaps, rng: np.random.Generator, num_samples: int, energy_combinator,
                  init_config, init_temperature: float, alpha_t, burn_in: int, energy_setup, samples_interval: int,
                  target_temperature: float, verbose: int = 0, iter_multiplier: float = None,
                  use_split_merge: bool = False, **gpu_options):
    """Drop-in for the reference's ``sample_rjmcmc`` (one tile).  Returns ``[points]`` for
    ``num_samples == 1`` and the last ``num_samples`` sampled configurations otherwise.  ``restarts=R`` (among the
    ``gpu_options``): the lowest-energy result of R independent chains; with ``recombine=True`` every interaction cluster
    of the result comes from its best chain."""
    return sample_rjmcmc_batch([image_data], rng, num_samples, energy_combinator, init_config, init_temperature,
                               alpha_t, burn_in, energy_setup, samples_interval, target_temperature, verbose,
                               iter_multiplier, use_split_merge, **gpu_options)[0]
