"""NSGA-III (Deb & Jain 2014): reference-direction survival.

Parents come exactly as in NSGA-II (rank tournament, SBX / mutation event
stream, the native spawn on the GPU); survival is ``ops.nsga3_select``: the
last admitted front is filled direction by direction, least-crowded reference
direction first, instead of by crowding distance. The selection is stateless
per call (no running ideal or nadir point) and stays on the population's
device: one native call on the GPU, plain torch elsewhere. Non-finite
objectives are out of scope.

The user can say where on the front the solutions should go: ``ref_dirs``
takes any (H, m) set of nonnegative directions in place of the default
Das-Dennis lattice.
"""

from __future__ import annotations

from math import comb
from typing import Any, Dict, Optional

import numpy as np
import torch

from dmosopt_amd import ops
from dmosopt_amd.datatypes import Struct
from dmosopt_amd.moea.nsga2 import NSGA2Optimizer


def _lattice(m: int, p: int) -> np.ndarray:
    """All (a_1..a_m) / p with nonnegative integers summing to p, rows in
    lexicographic order."""
    rows = []

    def rec(prefix, left, k):
        if k == m - 1:
            rows.append(prefix + [left])
            return
        for a in range(left + 1):
            rec(prefix + [a], left - a, k + 1)

    rec([], p, 0)
    return np.asarray(rows, dtype=np.float64) / float(p)


def reference_directions(m: int, partitions) -> np.ndarray:
    """Das-Dennis simplex lattice with ``partitions`` divisions per axis:
    H = C(p + m - 1, m - 1) rows summing to 1, in lexicographic order. A
    pair ``(outer, inner)`` appends a second lattice shrunk halfway to the
    centroid (the two-layer sets used beyond ~5 objectives)."""
    m = int(m)
    if m < 1:
        raise ValueError("reference_directions: m must be >= 1")
    if np.isscalar(partitions):
        layers = [int(partitions)]
    else:
        layers = [int(p) for p in partitions]
        if len(layers) != 2:
            raise ValueError("reference_directions: partitions is an int or a pair")
    if any(p < 1 for p in layers):
        raise ValueError("reference_directions: partitions must be >= 1")
    Z = _lattice(m, layers[0])
    if len(layers) == 2:
        Z = np.vstack([Z, 0.5 * _lattice(m, layers[1]) + 0.5 / m])
    return Z


def default_partitions(m: int, popsize: int) -> int:
    """The largest p whose lattice has at most ``popsize`` directions (1 at
    the least)."""
    p = 1
    while comb(p + m, m - 1) <= popsize:
        p += 1
    return p


def _check_ref_dirs(Z, m: Optional[int] = None) -> np.ndarray:
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim != 2 or Z.shape[0] < 1:
        raise ValueError("ref_dirs must be a non-empty (H, m) array")
    if m is not None and Z.shape[1] != m:
        raise ValueError(f"ref_dirs has {Z.shape[1]} columns, the objectives {m}")
    if not np.isfinite(Z).all():
        raise ValueError("ref_dirs must be finite")
    if (Z < 0).any():
        raise ValueError("ref_dirs must be nonnegative")
    if (Z.sum(axis=1) <= 0).any():
        raise ValueError("ref_dirs must not contain a zero row")
    return Z


class NSGA3Optimizer(NSGA2Optimizer):
    def __init__(
        self,
        popsize: int,
        nInput: int,
        nOutput: int,
        model: Optional[Any] = None,
        distance_metric: Optional[Any] = None,
        optimize_mean_variance: bool = False,
        **kwargs,
    ):
        # no crowding metric: survival is by reference direction
        super().__init__(
            popsize, nInput, nOutput, model=model, distance_metric=None,
            optimize_mean_variance=optimize_mean_variance, **kwargs,
        )
        self.name = "NSGA3"
        if self.opt_params.ref_dirs is not None:
            self.opt_params.ref_dirs = _check_ref_dirs(self.opt_params.ref_dirs)
        self._ref_cache = None

    @property
    def default_parameters(self) -> Dict[str, Any]:
        params = dict(super().default_parameters)
        params.update({"ref_partitions": None, "ref_dirs": None})
        return params

    # ------------------------------------------------------------------
    def reference_dirs(self, y: torch.Tensor) -> torch.Tensor:
        """The (H, m) direction set for objectives shaped like ``y``, on its
        device in its dtype; built on first use for the column count seen
        (mean-variance mode doubles the columns)."""
        m = int(y.shape[1])
        c = self._ref_cache
        if c is None or c[0] != (m, y.device, y.dtype):
            p = self.opt_params
            if p.ref_dirs is not None:
                Z = _check_ref_dirs(p.ref_dirs, m)
            else:
                parts = p.ref_partitions
                if parts is None:
                    parts = default_partitions(m, p.popsize)
                Z = reference_directions(m, parts)
            c = self._ref_cache = (
                (m, y.device, y.dtype),
                torch.as_tensor(Z, dtype=y.dtype, device=y.device).contiguous(),
            )
        return c[1]

    def _priorities(self, x_gen, pop_parm, H: int):
        """(dir_prio (H,), row_prio (N,)): fresh random permutations from
        ``torch_random`` on the population's device (no H2D copy). With a
        feasibility model the merged rows are ordered by its rank, most
        feasible first, the random permutation breaking ties."""
        dev, g = x_gen.device, self.torch_random
        gdev = g.device if g is not None else dev
        n = x_gen.shape[0] + pop_parm.shape[0]
        dir_prio = torch.randperm(H, generator=g, device=gdev).to(dev)
        row_prio = torch.randperm(n, generator=g, device=gdev).to(dev)
        if self.x_distance_fns is not None:
            feas = self._x_dists(torch.cat([x_gen, pop_parm], dim=0))[0]
            order = ops.lexsort([row_prio, -feas])
            row_prio = torch.empty_like(order)
            row_prio[order] = torch.arange(n, device=dev)
        return dir_prio, row_prio

    def _select(self, x_gen, y_gen, pop_parm, pop_obj):
        Z = self.reference_dirs(y_gen)
        dir_prio, row_prio = self._priorities(x_gen, pop_parm, Z.shape[0])
        return ops.nsga3_select(
            x_gen, y_gen, pop_parm, pop_obj, self.opt_params.popsize, Z, dir_prio, row_prio
        )

    def initialize_state(self, x, y, bounds, local_random, **params):
        parm, obj, rank, perm, _, _, niche, _ = self._select(x, y, x[:0], y[:0])
        zero = torch.zeros((), dtype=torch.long, device=x.device)
        return Struct(
            bounds=bounds,
            population_parm=parm,
            population_obj=obj,
            rank=rank,
            niche=niche[perm],  # the direction of every survivor
            successful_crossovers=zero.clone(),
            total_crossovers=0,
            successful_mutations=zero.clone(),
            total_mutations=0,
        )

    def update_strategy(self, x_gen, y_gen, gen_state, **params):
        p, st = self.opt_params, self.state
        parm, obj, rank, perm, _, _, niche, _ = self._select(
            x_gen, y_gen, st.population_parm, st.population_obj
        )
        self._count_survivors(perm, gen_state["crossover_indices"], x_gen.shape[0])
        st.population_parm, st.population_obj, st.rank = parm, obj, rank
        st.niche = niche[perm]  # the direction of every survivor
        if p.adaptive_population_size:
            self.update_population_size()
        if p.adaptive_operator_rates:
            self.update_operator_rates()

    def native_generations_eligible(self, *args, **kwargs) -> bool:
        """No native chunk driver for this survival: always False."""
        return False
