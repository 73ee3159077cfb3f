"""Op dispatch layer.

Every op has a pure-PyTorch reference implementation (``torch_ref``) used on
CPU and as the numerics oracle. On CUDA (= HIP/ROCm) tensors the hand-written
gfx950 kernels from the in-tree extension ``dmosopt_amd._hipops`` are used.
Per the framework contract, running on a GPU without the native extension is
an ERROR (no silent eager fallback): build it with
``python setup.py build_ext --inplace`` or ``__graft_entry__.build()``.

Set ``DMOSOPT_AMD_FORCE_TORCH=1`` to force the torch path (debugging only).
"""

from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import torch_ref
from .torch_ref import (  # re-exported torch-native helpers
    anyclose,
    filter_samples,
    lexsort,
    sbx_crossover_batch,
    polynomial_mutation_batch,
    tournament_selection,
    tournament_prob_vector,
)

_FORCE_TORCH = os.environ.get("DMOSOPT_AMD_FORCE_TORCH", "0") == "1"

_native = None
_native_err: Optional[str] = None


def _load_native():
    global _native, _native_err
    if _native is not None or _native_err is not None:
        return _native
    try:
        from dmosopt_amd import _hipops  # built in-tree by setup.py

        _native = _hipops
    except ImportError as e:  # remember why, for the loud failure path
        _native_err = str(e)
    return _native


def native_available() -> bool:
    return _load_native() is not None


def _use_native(*tensors: torch.Tensor) -> bool:
    if _FORCE_TORCH:
        return False
    if not any(t.is_cuda for t in tensors if isinstance(t, torch.Tensor)):
        return False
    native = _load_native()
    if native is None:
        raise RuntimeError(
            "dmosopt_amd: tensors are on GPU but the native HIP extension "
            "dmosopt_amd._hipops is not built (import error: "
            f"{_native_err}). Build it with `python setup.py build_ext "
            "--inplace` (PYTORCH_ROCM_ARCH=gfx950); refusing to fall back "
            "to eager PyTorch on the GPU."
        )
    return True


def native_fp32(*tensors: torch.Tensor) -> bool:
    """The gate of the float32 native paths: every tensor is a float32 GPU
    tensor, the torch path is not forced and the native extension is loaded
    (a GPU tensor without the extension is an error, as in every op here)."""
    return all(
        t.is_cuda and t.dtype == torch.float32 for t in tensors
    ) and _use_native(*tensors)


def _nu_arg(nu) -> float:
    """Matern nu as the native bindings take it: 0.0 stands for RBF."""
    return 0.0 if (nu is None or nu == float("inf")) else float(nu)


# ------------------------------------------------------------------ ranking
def pareto_rank(Y: torch.Tensor) -> torch.Tensor:
    if _use_native(Y):
        # the native binding routes internally: N <= 1024 the one-workgroup
        # bit-matrix peel; N > 1024 the grid-wide COOPERATIVE peel (all CUs).
        # Both are sync-free from the host, and there is no fallback: a
        # refused launch raises. Host syncs in ranking stall pipelined
        # generation loops far beyond their kernel-time cost (round-2
        # lesson, NOTES.md).
        return _native.pareto_rank(Y.contiguous().float())
    return torch_ref.pareto_rank(Y)


def dominance_degree_matrix(Y: torch.Tensor) -> torch.Tensor:
    if _use_native(Y):
        return _native.dominance_degree_matrix(Y.contiguous().float())
    return torch_ref.dominance_degree_matrix(Y)


def crowding_distance(Y: torch.Tensor) -> torch.Tensor:
    if _use_native(Y):
        return _native.crowding_distance(Y.contiguous().float()).to(Y.dtype)
    return torch_ref.crowding_distance(Y)


def euclidean_distance_metric(Y: torch.Tensor) -> torch.Tensor:
    return torch_ref.euclidean_distance_metric(Y)


def fused_rank_metric_perm(rank: torch.Tensor, metric: torch.Tensor) -> torch.Tensor:
    """Fused sort key for the common (rank, -metric) case: one stable argsort
    on (rank << 32 | descending_monotone_bits(metric)) instead of two radix
    sorts + gathers per generation. The IEEE sign-flip mapping
    (b | 0x80000000 for b >= 0, ~b for b < 0) is a total-order bijection
    float32 -> uint32 that handles NEGATIVE metric values too (user-supplied
    callables may return them); ties fall back to index order exactly like
    np.lexsort."""
    d = torch.nan_to_num(
        metric.float(),
        nan=0.0,
        posinf=float(torch.finfo(torch.float32).max),
        neginf=float(torch.finfo(torch.float32).min),
    )
    b = d.view(torch.int32).to(torch.int64) & 0xFFFFFFFF  # raw bits as u32
    asc = torch.where(b >= 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)
    key = (rank.to(torch.int64) << 32) | ((0xFFFFFFFF - asc) & 0xFFFFFFFF)
    return torch.argsort(key, stable=True)


def order_mo(
    x: torch.Tensor,
    y: torch.Tensor,
    x_dists: Optional[List[torch.Tensor]] = None,
    y_distance_metrics: Optional[List] = None,
):
    # rank+crowding use dispatched kernels internally via the metric calls
    rank = pareto_rank(y)
    y_dist_vals: List[torch.Tensor] = []
    if y_distance_metrics:
        for metric in y_distance_metrics:
            if callable(metric):
                y_dist_vals.append(metric(y))
            elif metric == "crowding":
                y_dist_vals.append(crowding_distance(y))
            elif metric == "euclidean":
                y_dist_vals.append(euclidean_distance_metric(y))
            else:
                raise RuntimeError(f"order_mo: unknown distance metric {metric}")
    x_dist_vals = list(x_dists) if x_dists else []
    if (
        not x_dist_vals
        and len(y_dist_vals) == 1
        and y.device.type == "cuda"
    ):
        perm = fused_rank_metric_perm(rank, y_dist_vals[0])
        return perm, rank[perm], (y_dist_vals[0][perm],)
    keys = [-d for d in x_dist_vals] + [-d for d in y_dist_vals] + [rank.to(y.dtype)]
    perm = lexsort(keys)
    return perm, rank[perm], tuple(d[perm] for d in y_dist_vals)


def remove_worst(
    population_parm: torch.Tensor,
    population_obj: torch.Tensor,
    pop: int,
    x_dists: Optional[List[torch.Tensor]] = None,
    y_distance_metrics: Optional[List] = None,
):
    perm, rank, _ = order_mo(
        population_parm, population_obj, x_dists=x_dists, y_distance_metrics=y_distance_metrics
    )
    perm = perm[:pop]
    return population_parm[perm], population_obj[perm], rank[:pop], perm


def nsga3_select_native(x_gen, y_gen, pop_parm, pop_obj, Z) -> bool:
    """The gate of the native NSGA-III selection: float32 GPU populations on
    the native path and a shape ``_hipops.nsga3_select_fits`` admits."""
    return native_fp32(x_gen, y_gen, pop_parm, pop_obj) and _native.nsga3_select_fits(
        y_gen.shape[0] + pop_obj.shape[0], Z.shape[0], y_gen.shape[1]
    )


def nsga3_select(x_gen, y_gen, pop_parm, pop_obj, keep, Z, dir_prio, row_prio):
    """NSGA-III survivor selection of the merged rows ``[x_gen; pop_parm]``
    against the reference directions ``Z`` (H, m): Pareto rank, ideal and
    intercept normalisation, association to the nearest direction, niching
    with the tie priorities ``dir_prio`` (H,) / ``row_prio`` (N,) (permutations,
    lower = earlier). Stateless; non-finite objectives are out of scope.

    Returns (parm, obj, rank, perm, ideal, scale, niche, dist): the rows kept
    (min(keep, N) of them), their index ``perm`` into the merged rows, and for
    inspection the ideal point, the scale and every merged row's direction and
    distance (-1 / +inf outside the fronts admitted). Float32 GPU tensors
    inside the gate run ops/hip/nsga3.hip; everything else
    torch_ref.nsga3_select in the objectives' dtype, on their device."""
    if nsga3_select_native(x_gen, y_gen, pop_parm, pop_obj, Z):
        return tuple(_native.nsga3_select(
            x_gen.contiguous(), y_gen.contiguous(),
            pop_parm.contiguous(), pop_obj.contiguous(), int(keep),
            Z.float().contiguous(), dir_prio.contiguous(), row_prio.contiguous(),
        ))
    parm = torch.cat([x_gen, pop_parm], dim=0)
    obj = torch.cat([y_gen, pop_obj], dim=0)
    return torch_ref.nsga3_select(
        parm, obj, keep, Z.to(obj.dtype), dir_prio, row_prio, rank=pareto_rank(obj)
    )


def top_k_mo(x: torch.Tensor, y: torch.Tensor, top_k=None):
    """Top-k rows by non-dominated sort (reference MOEA.top_k_MO,
    MOEA.py:350-372); returns (x, y) unchanged when top_k is not an int or
    the population is already small enough."""
    if not isinstance(top_k, int) or x.shape[0] <= top_k:
        return x, y
    perm, _, _ = order_mo(x, y)
    perm = perm[:top_k]
    return x[perm], y[perm]


def get_duplicates(X: torch.Tensor, eps: float = 1e-16) -> torch.Tensor:
    if _use_native(X):
        return _native.get_duplicates(X.contiguous().float(), eps)
    return torch_ref.get_duplicates(X, eps)


def remove_duplicates(x: torch.Tensor, y: torch.Tensor, eps: float = 1e-16):
    dup = get_duplicates(x, eps)
    return x[~dup], y[~dup]


# ------------------------------------------------------------- variation ops
def sbx_from_pool(pool, i1, i2, di, lo, hi, seed: int, generator=None):
    """SBX on pool rows (i1, i2) -> (child1, child2), fused RNG on GPU."""
    if native_fp32(pool):
        return _native.sbx_batch(
            pool.contiguous(),
            i1.to(torch.int32).contiguous(),
            i2.to(torch.int32).contiguous(),
            di.float().contiguous(),
            lo.float().contiguous(),
            hi.float().contiguous(),
            int(seed),
        )
    return sbx_crossover_batch(pool[i1], pool[i2], di, lo, hi, generator=generator)


def mutation_from_pool(pool, idx, di, lo, hi, mutation_rate: float, seed: int, generator=None):
    """Polynomial mutation on pool rows idx, fused RNG on GPU."""
    if native_fp32(pool):
        return _native.mutation_batch(
            pool.contiguous(),
            idx.to(torch.int32).contiguous(),
            di.float().contiguous(),
            lo.float().contiguous(),
            hi.float().contiguous(),
            float(mutation_rate),
            int(seed),
        )
    return polynomial_mutation_batch(
        pool[idx], di, lo, hi, mutation_rate=mutation_rate, generator=generator
    )


# -------------------------------------------------------------------- GP ops
def gp_pred_args(X, theta, alpha, y_mean, y_std, nu, anisotropic):
    """Per-fit arguments of the native predict calls, converted once."""
    return (
        X.contiguous(), theta.contiguous().float(), alpha.contiguous().float(),
        y_mean.float().contiguous(), y_std.float().contiguous(), _nu_arg(nu),
        bool(anisotropic),
    )


# Native predict calls on arguments the caller holds converted already
# (models/gp.py caches gp_pred_args per fit: the generation loop is host-
# dispatch-bound) and after the caller has passed native_fp32 itself.
def gp_predict_mean_cached(Xq, pred_args, q_lb, q_invrg):
    """Posterior mean (P, B) of float32 queries (raw with q_lb / q_invrg)."""
    return _native.gp_predict_mean(Xq, *pred_args, q_lb, q_invrg)


def gp_predict_mean_var_cached(Xq, pred_args, Linv, q_lb, q_invrg, var_decimals):
    """(P, 2B) block [mean | var], var = y_std^2 * max(sf2 + noise -
    |Linv k*|^2, 0); ``var_decimals >= 0`` rounds the variance columns."""
    return _native.gp_predict_mean_var(
        Xq, *pred_args[:3], Linv, *pred_args[3:], q_lb, q_invrg, var_decimals
    )


def gp_predict_mean_fused(Xq, X, theta, alpha, y_mean, y_std, nu, anisotropic):
    """Fused normalized-query posterior mean; None when native doesn't apply."""
    if Xq.is_cuda and native_fp32(X):
        return gp_predict_mean_cached(
            Xq.float().contiguous(),
            gp_pred_args(X, theta, alpha, y_mean, y_std, nu, anisotropic), None, None,
        )
    return None


def gp_predict_mean_var_fused(
    Xq, X, theta, alpha, Linv, y_mean, y_std, nu, anisotropic,
    q_lb=None, q_invrg=None, var_decimals=-1,
):
    """gp_predict_mean_var_cached on unconverted arguments; None when native
    doesn't apply."""
    if Xq.is_cuda and native_fp32(X):
        return gp_predict_mean_var_cached(
            Xq.float().contiguous(),
            gp_pred_args(X, theta, alpha, y_mean, y_std, nu, anisotropic),
            Linv.contiguous().float(), q_lb, q_invrg, int(var_decimals),
        )
    return None


def gp_predict_pof_cached(Xq, pred_args, Linv, q_lb, q_invrg):
    """Native (P, B + 1) block [PoF | rank] of float32 queries (raw with
    q_lb / q_invrg): PoF_b = Phi(z_b) with z_b the posterior mean over the
    noise-inclusive posterior deviation (ops/hip/gp_pof.hip), rank the mean
    over b in column order. Arguments as gp_predict_mean_var_cached, after
    the caller has passed native_fp32 itself."""
    return _native.gp_predict_pof(
        Xq, *pred_args[:3], Linv, *pred_args[3:], q_lb, q_invrg
    )


def gp_predict_pof(
    Xq, X, theta, alpha, Linv, y_mean, y_std, nu, anisotropic,
    q_lb=None, q_invrg=None,
):
    """GP probability of feasibility, (P, B + 1) = [PoF | rank]. Float32 GPU
    tensors run the fused native call; everything else (CPU, float64, forced
    torch) torch_ref.gp_predict_pof_ref in the dtype of X."""
    if Xq.is_cuda and native_fp32(X):
        return gp_predict_pof_cached(
            Xq.float().contiguous(),
            gp_pred_args(X, theta, alpha, y_mean, y_std, nu, anisotropic),
            Linv.contiguous().float(),
            None if q_lb is None else q_lb.float().contiguous(),
            None if q_invrg is None else q_invrg.float().contiguous(),
        )
    return torch_ref.gp_predict_pof_ref(
        Xq, X, theta, alpha, Linv, y_mean, y_std, nu, anisotropic, q_lb, q_invrg
    )


#: widest input the gradient kernel takes (16 dimensions per thread)
GP_MEAN_GRAD_MAX_D = 128


def gp_mean_grad_native(Xq, X) -> bool:
    """The gate of the native mean-gradient path: GPU queries, a float32 GPU
    fit on the native path, D <= GP_MEAN_GRAD_MAX_D."""
    return Xq.is_cuda and X.shape[1] <= GP_MEAN_GRAD_MAX_D and native_fp32(X)


def gp_predict_mean_grad_cached(Xq, pred_args, q_lb, q_invrg):
    """Native (mean (P, B), jac (P, B, D)) of float32 queries (raw with q_lb /
    q_invrg) after the caller has passed gp_mean_grad_native itself; the mean
    is bitwise gp_predict_mean_cached's."""
    mean, jac = _native.gp_predict_mean_grad(Xq, *pred_args, q_lb, q_invrg)
    return mean, jac


def gp_predict_mean_grad(
    Xq, X, theta, alpha, y_mean, y_std, nu, anisotropic, q_lb=None, q_invrg=None
):
    """Posterior mean (P, B) and its gradient in the query point (P, B, D),
    in the units the queries come in (raw with q_lb / q_invrg, unit box
    without). Float32 GPU tensors with D <= 128 run the fused native kernels
    (ops/hip/gp_mean_grad.hip); everything else the closed form in plain
    torch, in the dtype of X."""
    if gp_mean_grad_native(Xq, X):
        return gp_predict_mean_grad_cached(
            Xq.float().contiguous(),
            gp_pred_args(X, theta, alpha, y_mean, y_std, nu, anisotropic),
            None if q_lb is None else q_lb.float().contiguous(),
            None if q_invrg is None else q_invrg.float().contiguous(),
        )
    return torch_ref.gp_predict_mean_grad_ref(
        Xq, X, theta, alpha, y_mean, y_std, nu, anisotropic, q_lb, q_invrg
    )


def gp_predict_path_cached(Xq, pred_args, Omega, tau, amp, q_lb, q_invrg):
    """Native sample-path values (P, B) of float32 queries (raw with q_lb /
    q_invrg) after the caller has passed gp_mean_grad_native itself.
    ``pred_args`` is gp_pred_args output with the path's weights alpha' in the
    alpha slot; Omega, tau, amp are contiguous float32."""
    return _native.gp_predict_path(Xq, *pred_args, Omega, tau, amp, q_lb, q_invrg)


def gp_predict_path(
    Xq, X, theta, alpha_path, y_mean, y_std, nu, anisotropic, Omega, tau, amp,
    q_lb=None, q_invrg=None,
):
    """Values of one GP posterior sample path per batch row, (P, B):

        y_mean_b + y_std_b (k_b(u, X) alpha_path_b
                            + sum_j amp_bj cos(2 pi (tau_bj + Omega_bj . u)))

    with u the queries (raw with q_lb / q_invrg, unit box without). Float32
    GPU tensors with D <= 128 run the posterior-mean launches with alpha_path
    and the feature kernels of ops/hip/gp_path.hip in one extension call;
    everything else the cross kernel, a bmm and
    torch_ref.gp_path_features_ref, in the dtype of X."""
    if gp_mean_grad_native(Xq, X):
        return gp_predict_path_cached(
            Xq.float().contiguous(),
            gp_pred_args(X, theta, alpha_path, y_mean, y_std, nu, anisotropic),
            Omega.float().contiguous(), tau.float().contiguous(),
            amp.float().contiguous(),
            None if q_lb is None else q_lb.float().contiguous(),
            None if q_invrg is None else q_invrg.float().contiguous(),
        )
    return gp_predict_path_composed(
        Xq, X, theta, alpha_path, y_mean, y_std, nu, anisotropic, Omega, tau, amp,
        q_lb, q_invrg,
    )


def gp_predict_path_composed(
    Xq, X, theta, alpha_path, y_mean, y_std, nu, anisotropic, Omega, tau, amp,
    q_lb=None, q_invrg=None,
):
    """gp_predict_path as a composition of torch ops in the dtype of X, on
    any device: the dispatched cross kernel, a bmm and the reference
    features."""
    from dmosopt_amd.models import gp_core

    dt = X.dtype
    B = theta.shape[0]
    u = Xq.to(dt)
    if q_lb is not None:
        u = (u - q_lb.to(dt)) * q_invrg.to(dt)
    Ks = gp_core.build_kernel(u, X, theta.to(dt), nu=nu, anisotropic=anisotropic)
    upd = torch.bmm(Ks, alpha_path.to(dt).reshape(B, -1, 1))[:, :, 0]  # (B, P)
    feat = torch_ref.gp_path_features_ref(u, Omega, tau, amp)
    return (y_mean.to(dt).reshape(B)[None, :]
            + y_std.to(dt).reshape(B)[None, :] * (upd + feat).T)


def sceua_propose(cx, lcs, bl, bu, nps, seed):
    return _native.sceua_propose(cx, lcs, bl, bu, nps, seed)


def sceua_accept(cx, cf, cand, fall, lcs, act, icall, nps):
    return _native.sceua_accept(cx, cf, cand, fall, lcs, act, icall, nps)


def sceua_propose_sched(cx, sched, step, bl, bu, cand):
    """sceua_propose for the stage ``step[0]`` of the device-side schedule
    ``sched`` (nspl, nps + 2) int32 — per row the nps simplex positions and
    the low / high 32-bit words of the stage's Philox seed — written into the
    caller's ``cand`` (3, S*G, nopt). Posts ``step[0] + 1`` in ``step[1]``."""
    _native.sceua_propose_sched(cx, sched, step, bl, bu, cand)


def sceua_accept_sched(cx, cf, cand, fall, sched, step, act, icall):
    """sceua_accept for the stage ``step[1] - 1`` of the device-side schedule;
    its last act advances ``step[0]`` to ``step[1]``."""
    _native.sceua_accept_sched(cx, cf, cand, fall, sched, step, act, icall)


def sceua_unpartition(cx, cf, x, xf):
    """Complexes (S,G,npg,.) -> population (S,npt,.), row p*G + g = position
    p of complex g, into the caller's ``x`` / ``xf``."""
    _native.sceua_unpartition(cx, cf, x, xf)


def sceua_partition_pack(x, xf, order, icall, xs, xfs, cx, cf, pack):
    """Population gathered by ``order`` (S,npt) int64 -> ``xs`` / ``xfs``, its
    partition into the complexes ``cx`` / ``cf``, and the termination pack
    (S, 2 + 2 nopt) float32: icall, best f, per-dimension max, then min."""
    _native.sceua_partition_pack(x, xf, order, icall, xs, xfs, cx, cf, pack)


def gp_nmll_into(X, theta, y, K, Z, logdet, info, out, nu, anisotropic, jitter):
    """gp_nmll_fused's values, bit for bit, into caller-owned float32 buffers
    K (B,N,N), Z (B,N), logdet (B,), out (B,) and int32 info (B,): no
    allocation, and where the look-ahead fused-solve route applies no fill,
    copy or reduce launch either. Native only."""
    _native.gp_nmll_into(
        X, theta, y, K, Z, logdet, info, out, _nu_arg(nu), bool(anisotropic),
        float(jitter),
    )


def gp_nmll_fused(X, theta, y, nu, anisotropic, jitter):
    """Fused batched GP NMLL (assemble + Cholesky + solve + reduce) in one
    extension call; None if the native path does not apply."""
    if native_fp32(X):
        return _native.gp_nmll(
            X.contiguous(), theta.contiguous().float(), y.contiguous().float(),
            _nu_arg(nu), bool(anisotropic), float(jitter),
        )
    return None


def gp_nmll_grad(X, theta, y, nu, anisotropic, jitter):
    """Batched GP NMLL and its analytic gradient -> (nmll (B,), grad (B,p)).
    Float32 GPU tensors run the fused native pipeline (value pipeline of
    gp_nmll, then alpha, K^-1 and the gp_nmll_grad.hip tile kernels in the
    same extension call); everything else the closed form in plain torch."""
    if native_fp32(X):
        nmll, grad = _native.gp_nmll_grad(
            X.contiguous(), theta.contiguous().float(), y.contiguous().float(),
            _nu_arg(nu), bool(anisotropic), float(jitter),
        )
        return nmll, grad
    return torch_ref.gp_nmll_grad_ref(X, theta, y, nu, anisotropic, jitter)


def matern_train_kernel(X, theta, nu, anisotropic, jitter):
    """Batched symmetric kernel matrices K (B,N,N) with noise+jitter diag."""
    if native_fp32(X):
        return _native.matern_train(
            X.contiguous(), theta.contiguous().float(), _nu_arg(nu), bool(anisotropic), float(jitter)
        )
    from dmosopt_amd.models import gp_core

    return gp_core.build_kernel_torch(X, None, theta, nu=nu, anisotropic=anisotropic, jitter=jitter)


def matern_cross_kernel(Xq, X, theta, nu, anisotropic):
    """Batched cross kernel K* (B,P,N), no diagonal noise."""
    if native_fp32(X):
        return _native.matern_cross(
            Xq.contiguous(), X.contiguous(), theta.contiguous().float(), _nu_arg(nu), bool(anisotropic)
        )
    from dmosopt_amd.models import gp_core

    return gp_core.build_kernel_torch(Xq, X, theta, nu=nu, anisotropic=anisotropic)


def matern_cross_bf16_kernel(Xq, X, theta, nu, anisotropic, q_lb=None, q_invrg=None):
    """bf16-MFMA cross kernel (config #2 precision path): inputs rounded to
    bf16 in LDS, dot products on v_mfma_f32_16x16x32_bf16 (fp32 accumulate),
    Matern transform and output in fp32. GPU-only — no host fallback (the
    bf16 route is explicitly requested, silence would hide a missing
    extension)."""
    if not native_fp32(X):
        raise RuntimeError(
            "matern_cross_bf16 requires the gfx950 native extension and "
            "float32 CUDA tensors"
        )
    return _native.matern_cross_bf16(
        Xq.contiguous(), X.contiguous(), theta.contiguous().float(), _nu_arg(nu),
        bool(anisotropic), q_lb, q_invrg,
    )


def chol_factor_batched_bf16(K):
    """Batched Cholesky with the trailing SYRK updates on the bf16 matrix
    units (panels stay exact fp32). Falls back to the fp32 factorization
    when the native path is unavailable (CPU tests)."""
    if native_fp32(K) and K.shape[1] > 32:
        logdet, info = _native.cholesky_batched_bf16_(K)
        return K, logdet, info
    return chol_factor_batched(K)


def chol_factor_batched(K):
    """Factor K (B,N,N) in place -> (L, logdet (B,), info (B,)).

    Routing: the native launcher picks between the multi-launch
    right-looking path (small batches; panel + MFMA SYRK tile launches)
    and the one-workgroup-per-matrix kernel (B >= ~48) — either way the
    ONLY working path at N ~ 300, where ROCm 7.2's batched rocSOLVER f32
    cholesky raises launch failures. Single large factorizations
    (N >= 1200, where rocSOLVER's multi-CU decomposition wins ~10x and
    was verified working) dispatch to torch/rocSOLVER."""
    if native_fp32(K):
        # crossover re-measured round 2 (profiles/README.md large-N table):
        # native wins to N=2048, parity at 4096
        if K.shape[1] < 2048:
            logdet, info = _native.cholesky_batched_(K)
            return K, logdet, info
    L, info = torch.linalg.cholesky_ex(K)
    logdet = torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(dim=-1)
    return L, logdet, info


CHOL_SCHEDULES = {"classic": 0, "lookahead": 1, "onelaunch": 2}
# diagonal factor of the panel; None = the process default
# (DMOSOPT_CHOL_FACTOR, "reg" unless set to "lds")
CHOL_FACTORS = {None: -1, "lds": 0, "reg": 1}


def chol_factor_multik(K, rhs=None, schedule="classic", factor=None):
    """Multi-launch factorization of K (B,N,N) with an EXPLICIT trailing-
    update schedule ("classic", "lookahead", or "onelaunch": the whole
    factorization in one launch where N fits, else look-ahead), an explicit
    diagonal factor ("lds", "reg" or None for the process default) and an
    optional rhs (B,N) carried through the fused forward solve.

    Returns (L, logdet (B,), info (B,), z) with z = L^-1 rhs (None without
    rhs); the inputs are left untouched. DMOSOPT_CHOL_LOOKAHEAD and
    DMOSOPT_CHOL_FACTOR are latched once per process, so this is how the
    schedules and the factors are compared inside one process. Native only:
    a missing extension is an error."""
    if not native_fp32(K):
        raise RuntimeError("chol_factor_multik needs the native extension "
                           "and a float32 GPU tensor")
    L = K.contiguous().clone()
    z = None if rhs is None else rhs.contiguous().float().clone()
    logdet, info = _native.cholesky_multik_sched_(
        L, z, CHOL_SCHEDULES[schedule], CHOL_FACTORS[factor])
    return L, logdet, info, z


def chol_solve_batched(L, Y):
    """Solve K X = Y given the factor L (B,N,N); Y (B,N,R) -> X (B,N,R)."""
    if native_fp32(L):
        Z = Y.contiguous().clone()
        _native.forward_solve_(L.contiguous(), Z)
        _native.backward_solve_(L.contiguous(), Z)
        return Z
    return torch.cholesky_solve(Y, L)


def tri_solve_forward(L, Y):
    """Solve L Z = Y (B,N,R)."""
    if native_fp32(L):
        Z = Y.contiguous().clone()
        _native.forward_solve_(L.contiguous(), Z)
        return Z
    return torch.linalg.solve_triangular(L, Y, upper=False)


__all__ = [
    "pareto_rank",
    "dominance_degree_matrix",
    "crowding_distance",
    "euclidean_distance_metric",
    "order_mo",
    "remove_worst",
    "nsga3_select",
    "top_k_mo",
    "get_duplicates",
    "remove_duplicates",
    "lexsort",
    "sbx_crossover_batch",
    "polynomial_mutation_batch",
    "tournament_selection",
    "tournament_prob_vector",
    "anyclose",
    "filter_samples",
    "native_available",
]
