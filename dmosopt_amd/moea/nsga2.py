"""NSGA-II with batched, device-resident variation.

Semantics parity with reference NSGA2.py:18-326 (tournament pool of
popsize/2, SBX + polynomial mutation event stream, elitist remove_worst
survivor selection, operator-success tracking, optional adaptive population
size / operator rates). The per-individual Python variation loop of the
reference is re-designed as: the Bernoulli event stream is drawn on the host
(cheap control flow), then ALL crossovers and ALL mutations of a generation
execute as two batched tensor ops (one fused HIP kernel each on GPU).
"""

from __future__ import annotations

from typing import Any, Dict, Optional

import numpy as np
import torch

from dmosopt_amd import ops
from dmosopt_amd.datatypes import Struct
from dmosopt_amd.moea.base import MOEA, device_rank
from dmosopt_amd.hv.indicators import PopulationDiversity


class NSGA2Optimizer(MOEA):
    def __init__(
        self,
        popsize: int,
        nInput: int,
        nOutput: int,
        model: Optional[Any] = None,
        distance_metric: Optional[Any] = "crowding",
        optimize_mean_variance: bool = False,
        **kwargs,
    ):
        super().__init__(name="NSGA2", popsize=popsize, nInput=nInput, nOutput=nOutput, **kwargs)
        self.model = model
        self.distance_metric = distance_metric
        self.optimize_mean_variance = optimize_mean_variance
        self.y_distance_metrics = [distance_metric] if distance_metric is not None else None
        self.x_distance_fns = None
        self.x_rank_tensor = None
        if model is not None and getattr(model, "feasibility", None) is not None:
            self.x_distance_fns = [model.feasibility.rank]
            # the same rank on the device, where the model offers it
            self.x_rank_tensor = getattr(model.feasibility, "rank_tensor", None)

        p = self.opt_params
        if np.isscalar(p.di_crossover):
            p.di_crossover = np.full(nInput, float(p.di_crossover))
        if np.isscalar(p.di_mutation):
            p.di_mutation = np.full(nInput, float(p.di_mutation))
        if p.mutation_rate is None:
            p.mutation_rate = 1.0 / float(nInput)
        p.poolsize = int(round(p.popsize / 2.0))
        self.diversity_indicator = PopulationDiversity()
        # the native generation path: -1 what DMOSOPT_GEN_FUSED says, 0 the
        # chains of launches, 1 the fused spawn / select kernels; and whether
        # whole chunks of generations may go to the native driver (same
        # results on every route: tests/test_nsga2_gen_fused.py)
        self.gen_fused = -1
        self.native_chunks = True

    @property
    def default_parameters(self) -> Dict[str, Any]:
        return {
            "crossover_prob": 0.9,
            "mutation_prob": 0.1,
            "mutation_rate": None,
            "nchildren": 1,
            "di_crossover": 1.0,
            "di_mutation": 20.0,
            "max_population_size": 2000,
            "min_population_size": 100,
            "min_success_rate": 0.2,
            "max_success_rate": 0.75,
            "adaptive_population_size": False,
            "adaptive_operator_rates": False,
        }

    # ------------------------------------------------------------------
    def _di_tensors(self, pool: torch.Tensor):
        """di_crossover/di_mutation as device tensors, cached: they only
        change under adaptive operator rates, and re-uploading two small
        arrays every generation costs ~0.3 ms of H2D latency each."""
        cache = getattr(self, "_di_cache", None)
        if cache is None or cache[0].dtype != pool.dtype or cache[0].device != pool.device:
            p = self.opt_params
            cache = (
                torch.as_tensor(p.di_crossover, dtype=pool.dtype, device=pool.device),
                torch.as_tensor(p.di_mutation, dtype=pool.dtype, device=pool.device),
            )
            self._di_cache = cache
        return cache

    def _bounds_f32(self, device: torch.device):
        """The bounds columns as cached float32-contiguous tensors: they are
        stride-2 views of the (d,2) bounds tensor, and copying them costs two
        kernels + allocs per generation otherwise."""
        bc = getattr(self, "_bounds_cache", None)
        if bc is None or bc[0] != device:
            lo, hi = (
                self.state.bounds[:, k].to(device, torch.float32).contiguous() for k in (0, 1)
            )
            bc = self._bounds_cache = (device, lo, hi)
        return bc[1], bc[2]

    def _prefetch(self):
        """This optimizer's _SpawnPrefetch, made on first use."""
        if getattr(self, "_spawn_prefetch", None) is None:
            from dmosopt_amd.moea.variation import _SpawnPrefetch

            self._spawn_prefetch = _SpawnPrefetch()
        return self._spawn_prefetch

    def _x_dists(self, x: torch.Tensor):
        if self.x_distance_fns is None:
            return None
        on_device = device_rank(self.x_rank_tensor, x)
        if on_device is not None:  # no host trip
            return [on_device]
        out = []
        for fn in self.x_distance_fns:
            v = fn(x.cpu().numpy()) if not isinstance(x, np.ndarray) else fn(x)
            out.append(torch.as_tensor(np.asarray(v), dtype=x.dtype, device=x.device))
        return out

    def initialize_state(self, x, y, bounds, local_random, **params):
        perm, rank, _ = ops.order_mo(
            x, y, x_dists=self._x_dists(x), y_distance_metrics=self.y_distance_metrics
        )
        pop = self.opt_params.popsize
        perm = perm[:pop]
        # success counters live on the device so per-generation operator
        # tracking never forces a host sync (read with .item() only when the
        # adaptive-rate logic actually needs them)
        zero = torch.zeros((), dtype=torch.long, device=x.device)
        state = Struct(
            bounds=bounds,
            population_parm=x[perm],
            population_obj=y[perm],
            rank=rank[:pop],
            successful_crossovers=zero.clone(),
            total_crossovers=0,
            successful_mutations=zero.clone(),
            total_mutations=0,
        )
        return state

    def generate_strategy(self, **params):
        p = self.opt_params
        popsize, poolsize = p.popsize, p.poolsize
        rng = self.local_random
        xlb, xub = self.state.bounds[:, 0], self.state.bounds[:, 1]
        population = self.state.population_parm
        rank = self.state.rank

        poolsize = min(poolsize, population.shape[0])
        di_c, di_m = self._di_tensors(population)
        if population.device.type == "cuda" and ops.native_available():
            # tournament + event-decoded variation chained in ONE binding
            # call (the loop is host-dispatch-bound; the pool tensor never
            # surfaces to python)
            from dmosopt_amd.moea.variation import spawn_generation_native

            res = spawn_generation_native(
                population, rank, poolsize, 0.5, rng, popsize,
                p.crossover_prob, p.mutation_prob, p.mutation_rate,
                di_c, di_m, *self._bounds_f32(population.device),
                prefetch=self._prefetch(), fused=self.gen_fused,
            )
            if res is not None:
                x_gen, crossover_indices, mutation_indices = res
                self.state.total_crossovers += int(crossover_indices.shape[0]) // 2
                self.state.total_mutations += int(mutation_indices.shape[0])
                return x_gen, {
                    "crossover_indices": crossover_indices,
                    "mutation_indices": mutation_indices,
                    "clamped": True,  # variation kernels clamp to [xlb,xub]
                }
        pool_idx = ops.tournament_selection(
            population.shape[0], poolsize, [rank], rng,
            generator=self.torch_random,
        )
        pool = population[pool_idx]
        from dmosopt_amd.moea.variation import event_stream_variation

        x_gen, crossover_indices, mutation_indices = event_stream_variation(
            pool, rng, popsize, pool.shape[0], p.crossover_prob, p.mutation_prob,
            p.mutation_rate, di_c, di_m, xlb, xub, torch_random=self.torch_random,
        )
        self.state.total_crossovers += int(crossover_indices.shape[0]) // 2
        self.state.total_mutations += int(mutation_indices.shape[0])
        return x_gen, {
            "crossover_indices": crossover_indices,
            "mutation_indices": mutation_indices,
        }

    def _count_survivors(self, perm, c_idx, n_children):
        """Add the surviving crossover pairs and mutation children to the
        device-side success counters without a host round-trip: children are
        rows [0, n_children) of the concatenation, so survive where
        `perm < n_children`."""
        st = self.state
        if not isinstance(c_idx, torch.Tensor):
            c_idx = torch.as_tensor(np.asarray(c_idx), dtype=torch.long, device=perm.device)
        if (
            perm.device.type == "cuda"
            and ops.native_available()
            and n_children <= 2048
            and st.successful_crossovers.device.type == "cuda"
        ):
            from dmosopt_amd import _hipops

            if _hipops.survivor_count(
                perm.contiguous(), c_idx.contiguous(), n_children,
                st.successful_crossovers, st.successful_mutations,
            ):
                return
        # fixed-shape ops only: a boolean gather over the slot-type mask
        # (masked_select/isin would force a sync or a sort)
        is_cross = torch.zeros(n_children, dtype=torch.bool, device=perm.device)
        is_cross[c_idx] = True
        child = perm < n_children
        slot = torch.where(child, perm, torch.zeros_like(perm))
        surv_cross = is_cross[slot] & child
        st.successful_crossovers += surv_cross.sum() // 2
        st.successful_mutations += ((~is_cross[slot]) & child).sum()

    def update_strategy(self, x_gen, y_gen, gen_state, **params):
        p, st = self.opt_params, self.state
        popsize = p.popsize
        c_idx = gen_state["crossover_indices"]
        # (a) select; `counted`: the selection call counted the survivors too
        counted = False
        if (
            x_gen.device.type == "cuda"
            and self.x_distance_fns is None
            and self.y_distance_metrics == ["crowding"]
            and ops.native_available()
        ):
            from dmosopt_amd import _hipops

            select_args = (
                x_gen.float().contiguous(), y_gen.float().contiguous(),
                st.population_parm.float().contiguous(),
                st.population_obj.float().contiguous(), popsize,
            )
            # selection + survivor accounting in one extension call where
            # the count kernel takes the generation (<= 2048 children)
            counted = (
                isinstance(c_idx, torch.Tensor)
                and c_idx.device.type == "cuda"
                and st.successful_crossovers.device.type == "cuda"
                and x_gen.shape[0] <= 2048
            )
            if counted:
                parm, obj, rank, perm = _hipops.nsga2_select_acc(
                    *select_args, c_idx.contiguous(), st.successful_crossovers,
                    st.successful_mutations, fused=self.gen_fused,
                )
            else:
                parm, obj, rank, perm = _hipops.nsga2_select(*select_args, fused=self.gen_fused)
        else:
            population_parm = torch.cat([x_gen, st.population_parm], dim=0)
            population_obj = torch.cat([y_gen, st.population_obj], dim=0)
            parm, obj, rank, perm = ops.remove_worst(
                population_parm,
                population_obj,
                popsize,
                x_dists=self._x_dists(population_parm),
                y_distance_metrics=self.y_distance_metrics,
            )
        # (b) count survivors
        if not counted:
            self._count_survivors(perm, c_idx, x_gen.shape[0])

        st.population_parm, st.population_obj, st.rank = parm, obj, rank
        if parm.shape[0] < popsize and self.logger is not None:
            self.logger.warning(
                f"NSGA2: population shrank to {parm.shape[0]} (< {popsize})"
            )

        if p.adaptive_population_size:
            self.update_population_size()
        if p.adaptive_operator_rates:
            self.update_operator_rates()

    # ------------------------------------------------- native chunk driver
    def native_generations_eligible(
        self, mdl, termination=None, evaluator=None, optimize_mean_variance=False
    ) -> bool:
        """Whether engine.optimize_loop may hand whole chunks of generations
        to run_generations_native: a float32 GPU population on the native
        ops, the surrogate the fp32 native GP itself (no sharding, bf16 or
        feasibility model), mean-only objectives, crowding, nothing that
        looks at or changes the loop between two generations (termination,
        evaluator, adaptive sizes or rates), shapes inside the fused kernels'
        gate. False on CPU."""
        st, p = self.state, self.opt_params
        if st is None or termination is not None or evaluator is not None:
            return False
        if optimize_mean_variance or self.optimize_mean_variance:
            return False
        if not self.native_chunks or self.gen_fused == 0:
            return False
        x = st.population_parm
        if (
            not isinstance(x, torch.Tensor)
            or x.device.type != "cuda"
            or not ops.native_fp32(x, st.population_obj)
            or st.rank.dtype != torch.long
            or st.successful_crossovers.device != x.device
        ):
            return False
        if self.x_distance_fns is not None or self.y_distance_metrics != ["crowding"]:
            return False
        if p.adaptive_population_size or p.adaptive_operator_rates:
            return False
        objective = getattr(mdl, "objective", None)
        args_fn = getattr(objective, "native_mean_args", None)
        if args_fn is None or getattr(mdl, "feasibility", None) is not None:
            return False
        from dmosopt_amd import _hipops

        if self.gen_fused < 0 and not _hipops.gen_fused_default():
            return False
        pred = args_fn(x.device)
        if pred is None:
            return False
        X, theta = pred[0], pred[1]
        return (
            x.shape[0] == p.popsize
            and 1 <= p.poolsize <= p.popsize
            and X.shape[1] == x.shape[1]
            and theta.shape[0] == st.population_obj.shape[1]
            # a generation's event stream ends at popsize - 1 .. popsize + 1 children
            and _hipops.nsga2_generations_fit(
                p.popsize, p.popsize + 1, st.population_obj.shape[1]
            )
        )

    def run_generations_native(self, n_gen: int, mdl):
        """Up to ``n_gen`` generations, at most what is left of one prefetch
        chunk, queued by ONE native call (spawn, predict, select each): the
        state, the counters and the draws from ``local_random`` are those of
        as many generate / evaluate / update rounds. Returns (children per
        generation, x_gen rows of all of them, their y_gen rows). Only where
        native_generations_eligible."""
        from dmosopt_amd import _hipops

        p, st = self.opt_params, self.state
        population = st.population_parm
        di_c, di_m = self._di_tensors(population)
        items = self._prefetch().next_chunk(
            self.local_random, p.popsize, p.poolsize, p.crossover_prob,
            p.mutation_prob, population.device, n_gen,
        )
        meta, counts = [], []
        for seed_t, C, M, seed_sbx, seed_mut, _, off in items:
            meta += [seed_t, C, M, seed_sbx, seed_mut, *off[1:]]
            counts.append(2 * C + M)
            st.total_crossovers += C
            st.total_mutations += M
        x_all, y_all, parm, obj, rank = _hipops.nsga2_run_generations(
            population.contiguous(), st.population_obj.contiguous(),
            st.rank.contiguous(), p.poolsize, 0.5, items[0][6][0], meta,
            di_c.float().contiguous(), di_m.float().contiguous(),
            *self._bounds_f32(population.device),
            float(p.mutation_rate), *mdl.objective.native_mean_args(population.device),
            st.successful_crossovers, st.successful_mutations,
        )
        st.population_parm, st.population_obj, st.rank = parm, obj, rank
        return counts, x_all, y_all

    def get_population_strategy(self):
        return (
            self.state.population_parm.clone(),
            self.state.population_obj.clone(),
        )

    # -------------------------------------------------------- adaptation
    def update_population_size(self):
        diversity, cd_spread = self.diversity_indicator.do(
            self.state.rank, self.state.population_obj
        )
        p = self.opt_params
        if diversity < 0.5 and cd_spread < 2.0:
            new_size = min(p.max_population_size, int(p.popsize * 1.2))
        elif diversity > 0.9 or cd_spread > 1.0:
            new_size = max(p.min_population_size, int(p.popsize * 0.9))
        else:
            new_size = p.popsize
        p.popsize = new_size
        p.poolsize = int(round(new_size / 2.0))

    def update_operator_rates(self):
        p = self.opt_params
        s = self.state
        if s.total_crossovers > 0:
            rate = float(s.successful_crossovers) / s.total_crossovers
            if rate < p.min_success_rate:
                p.di_crossover = np.maximum(1.0, p.di_crossover * 0.9)
                p.crossover_prob = min(0.95, p.crossover_prob * 1.1)
            elif rate > p.max_success_rate:
                p.di_crossover = np.minimum(100.0, p.di_crossover * 1.1)
                p.crossover_prob = max(0.5, p.crossover_prob * 0.9)
        if s.total_mutations > 0:
            rate = float(s.successful_mutations) / s.total_mutations
            if rate < p.min_success_rate:
                p.di_mutation = np.maximum(1.0, p.di_mutation * 0.9)
                p.mutation_prob = min(1.0 - p.crossover_prob, p.mutation_prob * 1.05)
                p.mutation_rate = min(0.95, p.mutation_rate * 1.1)
            elif rate > p.max_success_rate:
                p.di_mutation = np.minimum(100.0, p.di_mutation * 1.1)
                p.mutation_prob = max(0.1, p.mutation_prob * 0.9)
                p.mutation_rate = max(0.05 / self.nInput, p.mutation_rate * 0.9)
        s.successful_crossovers = torch.zeros_like(s.successful_crossovers)
        s.total_crossovers = 0
        s.successful_mutations = torch.zeros_like(s.successful_mutations)
        s.total_mutations = 0
        self._di_cache = None  # di arrays changed; re-upload next generation
