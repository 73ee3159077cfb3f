"""Pure-PyTorch reference implementations of the population ops.

These are the numerics oracles for the HIP kernels in ``ops/hip`` and the
CPU execution path. Semantics follow the reference implementation
(``/root/reference/dmosopt/dda.py``, ``MOEA.py``, ``indicators.py``) but are
fully vectorized: no per-individual Python loops. All functions take/return
torch tensors; float64 on CPU, float32 on device by default.
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

Tensor = torch.Tensor


# ------------------------------------------------------------------ ranking
def dominance_degree_matrix(Y: Tensor) -> Tensor:
    """D[i,j] = #objectives where Y[i,k] <= Y[j,k]  (N x N int32).

    Reference: dda.py:25-31.
    """
    n, d = Y.shape
    D = torch.zeros((n, n), dtype=torch.int32, device=Y.device)
    for k in range(d):
        yk = Y[:, k]
        D += (yk[:, None] <= yk[None, :]).to(torch.int32)
    return D


def pareto_rank(Y: Tensor) -> Tensor:
    """0-based Pareto front index per row of Y (minimization).

    DDA ranking (dda.py:34-76 semantics: D[i][j] == m, after zeroing
    mutual-domination entries of identical rows, means i dominates j) with
    a dominator-COUNT front peel: n_dom[j] = #alive dominators; a front is
    n_dom == 0; peeling subtracts only the peeled rows' contributions —
    O(N^2) total instead of a full-matrix max per front.
    """
    n, d = Y.shape
    if n == 0:
        return torch.zeros(0, dtype=torch.long, device=Y.device)
    D = dominance_degree_matrix(Y)
    # zero out mutual-domination entries for identical objective rows
    identical = (D == d) & (D.T == d)
    Dom = (D == d) & ~identical  # Dom[i][j]: i dominates j
    n_dom = Dom.sum(dim=0)  # (n,) alive dominator counts
    rank = torch.zeros(n, dtype=torch.long, device=Y.device)
    alive = torch.ones(n, dtype=torch.bool, device=Y.device)
    k = 0
    remaining = n
    while remaining > 0:
        front = alive & (n_dom == 0)
        if not bool(front.any()):
            front = alive  # numerical safety: avoid infinite loop
        rank[front] = k
        alive &= ~front
        idx = front.nonzero(as_tuple=True)[0]
        remaining -= int(idx.numel())
        if remaining > 0:
            n_dom = n_dom - Dom[idx].sum(dim=0)
        k += 1
    return rank


def crowding_distance(Y: Tensor) -> Tensor:
    """Crowding distance metric (reference indicators.py:12-51), vectorized.

    Normalizes Y per-dimension to [0,1]; boundary points get 1.0 per dim,
    interior points get the gap US[i+1]-US[i-1]; scatter-added back.
    """
    n, d = Y.shape
    if n == 1:
        return torch.ones(1, dtype=Y.dtype, device=Y.device)
    lb = Y.min(dim=0, keepdim=True).values
    ub = Y.max(dim=0, keepdim=True).values
    span = (ub - lb).clamp_min_(0)
    span = torch.where(span == 0, torch.ones_like(span), span)
    U = (Y - lb) / span

    idx = U.argsort(dim=0)  # (n, d) indices of sorted order per dim
    US = torch.gather(U, 0, idx)
    DS = torch.empty_like(US)
    DS[0, :] = 1.0
    DS[-1, :] = 1.0
    if n > 2:
        DS[1:-1, :] = US[2:, :] - US[:-2, :]
    # scatter-add per dimension: D[idx[i,j]] += DS[i,j]
    D = torch.zeros(n, dtype=Y.dtype, device=Y.device)
    D.scatter_add_(0, idx.T.reshape(-1), DS.T.reshape(-1))
    D = torch.nan_to_num(D, nan=0.0)
    return D


def euclidean_distance_metric(Y: Tensor) -> Tensor:
    """Row norms of per-dimension normalized Y (indicators.py:54-65)."""
    lb = Y.min(dim=0).values
    ub = Y.max(dim=0).values
    span = ub - lb
    span = torch.where(span == 0, torch.ones_like(span), span)
    U = (Y - lb) / span
    return torch.sqrt((U * U).sum(dim=1))


def lexsort(keys: Sequence[Tensor]) -> Tensor:
    """np.lexsort equivalent: last key is primary. Stable sorts in sequence."""
    n = keys[0].shape[0]
    perm = torch.arange(n, device=keys[0].device)
    for k in keys:  # least-significant first
        kk = k[perm]
        order = torch.argsort(kk, stable=True)
        perm = perm[order]
    return perm


def order_mo(
    x: Tensor,
    y: Tensor,
    x_dists: Optional[List[Tensor]] = None,
    y_distance_metrics: Optional[List] = None,
) -> Tuple[Tensor, Tensor, Tuple[Tensor, ...]]:
    """Permutation of a non-dominated sort: by (rank, -y_dists..., -x_dists...).

    Mirrors reference MOEA.sortMO/orderMO (MOEA.py:242-347): primary key is
    pareto rank, then negated objective-space distances, then negated
    x-space distances. Returns (perm, rank[perm], y_dists_sorted).
    """
    rank = pareto_rank(y)
    y_dist_vals: List[Tensor] = []
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
    x_dist_vals: List[Tensor] = list(x_dists) if x_dists else []
    # np.lexsort((−x0, ..., −y0, ..., rank)): rank primary, then −y, then −x
    keys = [-d for d in x_dist_vals] + [-d for d in y_dist_vals] + [rank.to(y.dtype)]
    perm = lexsort(keys)
    y_sorted_dists = tuple(d[perm] for d in y_dist_vals)
    return perm, rank[perm], y_sorted_dists


# ----------------------------------------------------------------- variation
def sbx_crossover_batch(
    parent1: Tensor,
    parent2: Tensor,
    di_crossover: Tensor,
    xlb: Tensor,
    xub: Tensor,
    u: Optional[Tensor] = None,
    generator: Optional[torch.Generator] = None,
) -> Tuple[Tensor, Tensor]:
    """Batched SBX crossover (reference MOEA.py:215-239).

    parent1/parent2: (B, d). Returns two (B, d) children clipped to bounds.
    """
    if u is None:
        u = torch.rand(parent1.shape, dtype=parent1.dtype, device=parent1.device, generator=generator)
    di = di_crossover.to(parent1.dtype)
    beta = torch.where(
        u <= 0.5,
        (2.0 * u) ** (1.0 / (di + 1.0)),
        (1.0 / (2.0 * (1.0 - u))) ** (1.0 / (di + 1.0)),
    )
    c1 = 0.5 * ((1.0 - beta) * parent1 + (1.0 + beta) * parent2)
    c2 = 0.5 * ((1.0 + beta) * parent1 + (1.0 - beta) * parent2)
    return c1.clamp(xlb, xub), c2.clamp(xlb, xub)


def polynomial_mutation_batch(
    parent: Tensor,
    di_mutation: Tensor,
    xlb: Tensor,
    xub: Tensor,
    mutation_rate: float = 0.5,
    u: Optional[Tensor] = None,
    generator: Optional[torch.Generator] = None,
) -> Tensor:
    """Batched polynomial mutation (reference MOEA.py:191-212).

    A gene mutates 'low' when u < mutation_rate (delta in [-1,0]) else 'high'
    (delta in [0,1]); the child is parent + (xub-xlb)*delta, clipped.
    """
    if u is None:
        u = torch.rand(parent.shape, dtype=parent.dtype, device=parent.device, generator=generator)
    di = di_mutation.to(parent.dtype)
    delta_lo = (2.0 * u) ** (1.0 / (di + 1.0)) - 1.0
    delta_hi = 1.0 - (2.0 * (1.0 - u)) ** (1.0 / (di + 1.0))
    delta = torch.where(u < mutation_rate, delta_lo, delta_hi)
    child = parent + (xub - xlb) * delta
    return child.clamp(xlb, xub)


_TOURNAMENT_PROB_CACHE = {}


def tournament_prob_vector(n: int, p: float = 0.5) -> torch.Tensor:
    """Geometric selection probabilities p(1-p)^i over sorted candidates
    (cached per (n, p): rebuilt thousands of times per epoch otherwise)."""
    key = (n, p)
    out = _TOURNAMENT_PROB_CACHE.get(key)
    if out is None:
        i = torch.arange(n, dtype=torch.float64)
        prob = p * (1.0 - p) ** i
        out = prob / prob.sum()
        _TOURNAMENT_PROB_CACHE[key] = out
    return out


def tournament_selection(
    pop: int,
    poolsize: int,
    metrics: Sequence[Tensor],
    np_random,
    generator=None,
) -> Tensor:
    """Tournament selection into the mating pool (reference MOEA.py:385-395).

    Sorts candidates by lexsort(metrics) and samples `poolsize` without
    replacement with geometric probability over sorted position. With a
    device ``generator`` and device metrics the weighted draw runs on the
    GPU via the Gumbel top-k trick (exact weighted sampling without
    replacement: argmax_k of log(p_i) + Gumbel noise); otherwise the host
    numpy Generator draws, matching the reference's control stream.
    """
    # adaptive population sizing can briefly set poolsize above the CURRENT
    # population (the reference's update_population_size jumps straight to
    # min_population_size, NSGA2.py:268-270, and would crash its own
    # replace=False draw) — clamp to what exists
    poolsize = min(poolsize, pop)
    dev_metrics = [m if isinstance(m, torch.Tensor) else torch.as_tensor(m) for m in metrics]
    sorted_candidates = lexsort(dev_metrics)
    dev = sorted_candidates.device
    if generator is not None and dev.type == "cuda":
        logp = _tournament_logp(pop, dev)
        u = torch.rand(pop, dtype=torch.float32, device=dev, generator=generator)
        keys = logp - torch.log(-torch.log(u.clamp_min(1e-12)).clamp_min(1e-12))
        pool_pos = torch.topk(keys, poolsize).indices
        return sorted_candidates[pool_pos]
    prob = tournament_prob_vector(pop).numpy()  # cached
    pool_pos = np_random.choice(pop, size=poolsize, p=prob, replace=False)
    pool_pos = torch.as_tensor(pool_pos, dtype=torch.long, device=dev)
    return sorted_candidates[pool_pos]


_TOURNAMENT_LOGP_CACHE = {}


def _tournament_logp(pop: int, device) -> Tensor:
    key = (pop, str(device))
    out = _TOURNAMENT_LOGP_CACHE.get(key)
    if out is None:
        out = tournament_prob_vector(pop).log().to(device=device, dtype=torch.float32)
        _TOURNAMENT_LOGP_CACHE[key] = out
    return out


# ----------------------------------------------------------------- distance
def get_duplicates(X: Tensor, eps: float = 1e-16) -> Tensor:
    """Boolean mask of rows that duplicate an earlier row.

    Reference MOEA.get_duplicates (MOEA.py:426-436): pairwise euclidean
    distances, upper triangle (incl. diagonal) set to inf, then a row is a
    duplicate if any distance in its row is <= eps. With Y=X this marks, for
    each pair within eps, the row with the *smaller* index.
    """
    n = X.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.bool, device=X.device)
    # donot_use_mm: the GEMM (x^2-2xy+y^2) formulation leaves exact
    # duplicates at ~eps-sized residuals whose ULPs depend on the BLAS
    # threading/partitioning of the moment — the eps=1e-16 threshold then
    # flips run to run (observed: same-seed archives diverging). The
    # direct-difference path is deterministic and exact at zero distance.
    D = torch.cdist(X.double(), X.double(),
                    compute_mode="donot_use_mm_for_euclid_dist")
    iu = torch.triu_indices(n, n, offset=0, device=X.device)
    D[iu[0], iu[1]] = float("inf")
    D = torch.nan_to_num(D, nan=float("inf"))
    return (D <= eps).any(dim=1)


def anyclose(x: Tensor, X: Tensor, rtol: float = 1e-4, atol: float = 1e-8) -> bool:
    """True if any row of X is allclose to x."""
    if X.numel() == 0:
        return False
    return bool(torch.isclose(X, x[None, :], rtol=rtol, atol=atol).all(dim=1).any())


# ------------------------------------------------------------------- misc
def remove_worst(
    population_parm: Tensor,
    population_obj: Tensor,
    pop: int,
    x_dists: Optional[List[Tensor]] = None,
    y_distance_metrics: Optional[List] = None,
) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Elitist survivor selection: non-dominated sort, keep top `pop`.

    Returns (x, y, rank, perm) truncated to pop rows (MOEA.py:398-423).
    """
    perm, rank, _ = order_mo(
        population_parm, population_obj, x_dists=x_dists, y_distance_metrics=y_distance_metrics
    )
    perm = perm[:pop]
    return population_parm[perm], population_obj[perm], rank[:pop], perm


def filter_samples(y: Tensor, *companions, nan: str = "remove", outliers: str = "ignore"):
    """NaN / outlier filtering of objective rows (MOEA.py:445-467)."""
    mask = torch.ones(y.shape[0], dtype=torch.bool, device=y.device)
    if nan == "max":
        m = torch.nan_to_num(y).max(dim=0).values
        fill = torch.maximum(1e3 * m, torch.full_like(m, 1e5))
        y = torch.where(torch.isnan(y), fill[None, :], y)
    elif nan == "remove":
        mask = ~torch.isnan(y).any(dim=1)
    else:
        y = torch.nan_to_num(y, nan=float(nan))

    if outliers == "zscore":
        ylog = torch.log(y + 1.0)
        z = (ylog - ylog.mean(dim=0)) / ylog.std(dim=0, unbiased=True)
        mask = ~(z.abs() > 2).any(dim=1)

    out = [y[mask]]
    for c in companions:
        out.append(c[mask] if c is not None else None)
    return tuple(out)


# -------------------------------------------------------------------- GP ops
def gp_nmll_grad_ref(X: Tensor, theta: Tensor, y: Tensor, nu, anisotropic: bool,
                     jitter: float) -> Tuple[Tensor, Tensor]:
    """GP negative log marginal likelihood and its analytic gradient for a
    batch of theta, in the input dtype.

    X (N, D); theta (B, p) = [log sf2, log ell (1 or D), log noise]; y (N,)
    shared or (B, N) per-candidate rows. K = sf2 C + (noise + jitter) I,
    alpha = K^-1 y, W = K^-1 - alpha alpha^T, u_k = ((x_ik - x_jk)/ell_k)^2,
    d2 = sum_k u_k, g = -dc/d(d2):

        d/d log sf2   = 1/2 sf2   sum_ij W_ij c_ij
        d/d log noise = 1/2 noise tr(W)
        d/d log ell_k =     sf2   sum_ij W_ij g_ij u_k,ij   (isotropic: d2)

    d2 is the direct-difference sum, one dimension at a time (no (B,N,N,D)
    temporary). Returns (nmll (B,), grad (B, p)); a failed factorization or
    a non-finite value gives +inf and a zero gradient row.
    """
    import math

    N, D = X.shape
    B = theta.shape[0]
    theta = theta.to(X.dtype)
    sf2 = torch.exp(theta[:, 0])
    noise = torch.exp(theta[:, -1])
    inv_ell = torch.exp(-theta[:, 1 : 1 + D]) if anisotropic else torch.exp(-theta[:, 1:2])
    xs = X[None, :, :] * inv_ell[:, None, :]  # (B, N, D)

    def u_k(k):
        t = xs[:, :, None, k] - xs[:, None, :, k]
        return t * t

    d2 = torch.zeros(B, N, N, dtype=X.dtype, device=X.device)
    for k in range(D):
        d2 += u_k(k)
    rbf = nu is None or nu == float("inf") or nu == 0.0
    if rbf:
        c = torch.exp(-0.5 * d2)
        g = 0.5 * c
    else:
        r = torch.sqrt(d2)
        if nu == 0.5:
            c = torch.exp(-r)
            pos = r > 0
            g = torch.where(pos, c / (2.0 * torch.where(pos, r, torch.ones_like(r))),
                            torch.zeros_like(r))
        elif nu == 1.5:
            s = math.sqrt(3.0) * r
            e = torch.exp(-s)
            c = (1.0 + s) * e
            g = 1.5 * e
        elif nu == 2.5:
            s = math.sqrt(5.0) * r
            e = torch.exp(-s)
            c = (1.0 + s + (5.0 / 3.0) * d2) * e
            g = (5.0 / 6.0) * (1.0 + s) * e
        else:
            raise ValueError(f"Unsupported Matern nu={nu}")
    eye = torch.eye(N, dtype=X.dtype, device=X.device)
    K = sf2[:, None, None] * c + (noise + jitter)[:, None, None] * eye
    L, info = torch.linalg.cholesky_ex(K)
    bad = info != 0
    # keep the solves finite for a failed candidate; its row is masked below
    L = torch.where(bad[:, None, None], eye, L)
    yb = (y[None, :].expand(B, N) if y.dim() == 1 else y).to(X.dtype)
    alpha = torch.cholesky_solve(yb[:, :, None], L)[:, :, 0]  # (B, N)
    Kinv = torch.cholesky_solve(eye[None].expand(B, N, N), L)
    W = Kinv - alpha[:, :, None] * alpha[:, None, :]
    nmll = (
        0.5 * (yb * alpha).sum(dim=1)
        + torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(dim=-1)
        + 0.5 * N * math.log(2.0 * math.pi)
    )
    grad = torch.empty_like(theta)
    grad[:, 0] = 0.5 * sf2 * (W * c).sum(dim=(1, 2))
    grad[:, -1] = 0.5 * noise * torch.diagonal(W, dim1=-2, dim2=-1).sum(dim=-1)
    H = W * g
    if anisotropic:
        for k in range(D):
            grad[:, 1 + k] = sf2 * (H * u_k(k)).sum(dim=(1, 2))
    else:
        grad[:, 1] = sf2 * (H * d2).sum(dim=(1, 2))
    bad = bad | ~torch.isfinite(nmll)
    nmll = torch.where(bad, torch.full_like(nmll, float("inf")), nmll)
    grad = torch.where(bad[:, None], torch.zeros_like(grad), grad)
    return nmll, grad


def gp_predict_mean_grad_ref(Xq: Tensor, X: Tensor, theta: Tensor, alpha: Tensor,
                             y_mean: Tensor, y_std: Tensor, nu, anisotropic: bool,
                             q_lb: Optional[Tensor] = None,
                             q_invrg: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """GP posterior mean and its gradient in the query point, in the dtype of
    X, on any device.

    Xq (P, D) raw queries with q_lb / q_invrg (u = (Xq - q_lb) * q_invrg),
    unit-box queries without; X (N, D); theta (B, p) = [log sf2, log ell (1
    or D), log noise]; alpha (B, N) or (B, N, 1) standardised weights. With
    r2 = sum_d ((u_d - X_id)/ell_d)^2 and g = dk/d(r2):

        mean[p, b]   = y_mean_b + y_std_b sum_i alpha_bi sf2_b k(r2)
        jac[p, b, d] = y_std_b q_invrg_d (2/ell_bd^2)
                       sum_i alpha_bi sf2_b g(r2) (u_d - X_id)

    Both r2 and the factor of the sum are direct differences, one dimension
    at a time (no (B, P, N, D) temporary). nu = 1/2 has a kink at r = 0: a
    training point the query sits on contributes 0 to the gradient. Returns
    (mean (P, B), jac (P, B, D)), jac in the units the queries come in.
    """
    import math

    dt = X.dtype
    P, D = Xq.shape
    B = theta.shape[0]
    theta, Xq = theta.to(dt), Xq.to(dt)
    alpha = alpha.to(dt).reshape(B, -1)
    y_mean, y_std = y_mean.to(dt).reshape(B), y_std.to(dt).reshape(B)
    u = Xq if q_lb is None else (Xq - q_lb.to(dt)) * q_invrg.to(dt)
    sf2 = torch.exp(theta[:, 0])
    inv_ell = torch.exp(-theta[:, 1 : 1 + D]) if anisotropic else torch.exp(-theta[:, 1:2])
    inv_ell = inv_ell.expand(B, D)
    us = u[None, :, :] * inv_ell[:, None, :]  # (B, P, D)
    xs = X[None, :, :] * inv_ell[:, None, :]  # (B, N, D)

    def s_k(k):
        return us[:, :, None, k] - xs[:, None, :, k]  # (B, P, N)

    d2 = torch.zeros(B, P, X.shape[0], dtype=dt, device=X.device)
    for k in range(D):
        t = s_k(k)
        d2 += t * t
    if nu is None or nu == float("inf") or nu == 0.0:
        c = torch.exp(-0.5 * d2)
        g = -0.5 * c
    else:
        r = torch.sqrt(d2)
        if nu == 0.5:
            c = torch.exp(-r)
            pos = r > 0
            g = torch.where(pos, -c / (2.0 * torch.where(pos, r, torch.ones_like(r))),
                            torch.zeros_like(r))
        elif nu == 1.5:
            s = math.sqrt(3.0) * r
            e = torch.exp(-s)
            c = (1.0 + s) * e
            g = -1.5 * e
        elif nu == 2.5:
            s = math.sqrt(5.0) * r
            e = torch.exp(-s)
            c = (1.0 + s + (5.0 / 3.0) * d2) * e
            g = -(5.0 / 6.0) * (1.0 + s) * e
        else:
            raise ValueError(f"Unsupported Matern nu={nu}")
    sa = sf2[:, None] * alpha  # (B, N)
    mean = y_mean[None, :] + y_std[None, :] * (c * sa[:, None, :]).sum(dim=2).T
    w = g * sa[:, None, :]  # (B, P, N)
    jac = torch.empty(P, B, D, dtype=dt, device=X.device)
    scale = 2.0 * inv_ell * y_std[:, None]  # (B, D); s_k carries one 1/ell
    if q_invrg is not None:
        scale = scale * q_invrg.to(dt)[None, :]
    for k in range(D):
        jac[:, :, k] = ((w * s_k(k)).sum(dim=2) * scale[:, k : k + 1]).T
    return mean, jac


def gp_path_features_ref(U: Tensor, Omega: Tensor, tau: Tensor, amp: Tensor) -> Tensor:
    """Random-Fourier-feature term of a GP sample path in plain torch, on any
    device: U (P, D) unit-box queries, Omega (B, M, D) frequencies in turns
    per unit, tau (B, M) offsets in turns, amp (B, M) -> (B, P),

        f[b, p] = sum_j amp_bj cos(2 pi (tau_bj + sum_d Omega_bjd U_pd)).

    The phase is always formed in float64 from the given values (tau first,
    then one dimension at a time in index order, as the kernel of
    ops/hip/gp_path.hip does) and reduced to the turn fraction t - round(t)
    there: heavy-tailed frequencies give phases of 1e3..1e5 turns. The cosine
    and the sum over the features run in the dtype of U. Batch rows are
    walked in slices that bound the (B, P, M) temporaries.
    """
    import math

    dt = U.dtype
    B, M, D = Omega.shape
    P = U.shape[0]
    U64, amp_t = U.double(), amp.to(dt)
    out = torch.empty(B, P, dtype=dt, device=U.device)
    step = max(1, (1 << 22) // max(1, P * M))
    for b0 in range(0, B, step):
        Om = Omega[b0 : b0 + step].double()
        t = tau[b0 : b0 + step].double()[:, None, :].expand(-1, P, -1).clone()
        for k in range(D):
            t += Om[:, None, :, k] * U64[None, :, k, None]
        frac = (t - torch.round(t)).to(dt)
        out[b0 : b0 + step] = (
            amp_t[b0 : b0 + step, None, :] * torch.cos((2.0 * math.pi) * frac)
        ).sum(dim=2)
    return out


def gp_predict_pof_ref(Xq: Tensor, X: Tensor, theta: Tensor, alpha: Tensor,
                       Linv: Tensor, y_mean: Tensor, y_std: Tensor, nu,
                       anisotropic: bool, q_lb: Optional[Tensor] = None,
                       q_invrg: Optional[Tensor] = None,
                       L: Optional[Tensor] = None) -> Tensor:
    """GP probability of feasibility in plain torch, in the dtype of X, on
    any device: the (P, B + 1) block [PoF_0 .. PoF_{B-1} | rank].

    Xq (P, D) raw queries with q_lb / q_invrg, unit-box queries without;
    alpha (B, N) or (B, N, 1); Linv (B, N, N) = L^-1 of the fit. With the
    standardised posterior mean mu_n = k* alpha and the noise-inclusive
    variance var_n = max(sf2 + noise - |Linv k*|^2, 0):

        z_b   = (mu_n + y_mean_b / y_std_b) / sqrt(max(var_n, 1e-12))
        PoF_b = 0.5 erfc(-z_b / sqrt 2)        (accurate in both tails)
        rank  = (1/B) sum_b PoF_b              (added in column order)

    The closed form of ops/hip/gp_pof.hip, which replaces it on float32 GPU
    fits. With the factor ``L`` (B, N, N) given, Linv k* is the triangular
    solve L v = k* that FittedGP.predict uses on the CPU and ``Linv`` is not
    read (it may be None): the two agree to rounding, but the explicit
    inverse carries cond(L) once more, ~1e-11 of PoF in float64.

    nu = 1/2 only: the variance reads a direct-difference cross kernel, as
    the native bindings do (its kernel has an infinite slope in d2 at 0, so
    the cancellation of the norms-form d2 reaches the variance); the mean
    keeps the norms form.
    """
    import math

    from dmosopt_amd.models.gp_core import build_kernel_torch

    dt = X.dtype
    B = theta.shape[0]
    theta, Xq = theta.to(dt), Xq.to(dt)
    y_mean, y_std = y_mean.to(dt).reshape(B), y_std.to(dt).reshape(B)
    u = Xq if q_lb is None else (Xq - q_lb.to(dt)) * q_invrg.to(dt)
    Ks = build_kernel_torch(u, X, theta, nu=nu, anisotropic=anisotropic)  # (B,P,N)
    mean_n = torch.bmm(Ks, alpha.to(dt).reshape(B, -1, 1))[:, :, 0]  # (B, P)
    if nu == 0.5:
        D = X.shape[1]
        inv_ell = (torch.exp(-theta[:, 1 : 1 + D]) if anisotropic
                   else torch.exp(-theta[:, 1:2])).expand(B, D)
        d2 = torch.zeros_like(Ks)
        for k in range(D):  # one dimension at a time: no (B, P, N, D) temporary
            t = (u[None, :, None, k] - X[None, None, :, k]) * inv_ell[:, None, None, k]
            d2 += t * t
        Ks = torch.exp(theta[:, 0])[:, None, None] * torch.exp(-torch.sqrt(d2))
    if L is not None:
        v = torch.linalg.solve_triangular(L.to(dt), Ks.transpose(1, 2), upper=False)
    else:
        v = torch.bmm(Linv.to(dt), Ks.transpose(1, 2))  # (B, N, P)
    kss = torch.exp(theta[:, 0]) + torch.exp(theta[:, -1])
    var_n = (kss[:, None] - (v * v).sum(dim=1)).clamp_min(0.0)
    z = (mean_n + (y_mean / y_std)[:, None]) / torch.sqrt(var_n.clamp_min(1e-12))
    pof = 0.5 * torch.special.erfc(-z * math.sqrt(0.5))  # (B, P)
    out = torch.empty(Xq.shape[0], B + 1, dtype=dt, device=X.device)
    out[:, :B] = pof.T
    out[:, B] = mean_in_column_order(out[:, :B])
    return out


def mean_in_column_order(P: Tensor) -> Tensor:
    """Row means of P (n, C) with the columns added one at a time in index
    order, then one division by C: the order the feasibility kernel uses, so
    the result does not depend on how a reduction splits the row. The
    divisor is a tensor: a scalar one may become a multiplication by 1/C."""
    s = P[:, 0].clone()
    for b in range(1, P.shape[1]):
        s += P[:, b]
    return s / torch.full_like(s, P.shape[1])


# ------------------------------------------------------------------ NSGA-III
# Reference-direction survival (Deb & Jain 2014), stateless per call; the
# contract of ops/hip/nsga3.hip, in the dtype of the objectives. Every function
# but nsga3_niche_sequential is fixed-shape tensor code without a host sync.
# Non-finite objectives are out of scope.
def nsga3_level(rank: Tensor, keep: int) -> Tensor:
    """The last front admitted: the smallest l with #{rank <= l} >= min(keep,
    N), as a 0-d long tensor. S = {rank <= l}, P = {rank < l}, F = {rank == l}."""
    n = rank.shape[0]
    counts = torch.zeros(n, dtype=torch.long, device=rank.device)
    counts.scatter_add_(0, rank.clamp(0, n - 1), torch.ones_like(rank))
    # the cumulative counts ascend: the entries below K come before front l
    return (counts.cumsum(0) < min(int(keep), n)).sum()


def nsga3_normalize(Y: Tensor, rank: Tensor, keep: int):
    """(ideal (m,), scale (m,), l): ideal the column minimum over S; scale the
    hyperplane intercepts through the ASF extremes of the first front
    (weights 1 on the axis, 1e-6 off it, ties to the lowest row), solved in
    double; the first front's column maximum of Y - ideal where two extremes
    coincide or the solve is singular or not positive; 1 where that is below
    1e-6."""
    n, m = Y.shape
    dt, dev = Y.dtype, Y.device
    l = nsga3_level(rank, keep)
    in_S, in_F0 = rank <= l, rank == 0
    inf = torch.full_like(Y, float("inf"))
    ideal = torch.where(in_S[:, None], Y, inf).min(dim=0).values
    T = Y - ideal
    w = torch.full((m, m), 1e-6, dtype=dt, device=dev)
    w.fill_diagonal_(1.0)
    asf = (T[:, None, :] / w[None, :, :]).max(dim=2).values  # [row, axis]
    ext = torch.where(in_F0[:, None], asf, inf).argmin(dim=0)  # first minimum
    E = T[ext].to(torch.float64)
    a, info = torch.linalg.solve_ex(E, torch.ones(m, 1, dtype=torch.float64, device=dev))
    a = a[:, 0]
    same = (ext[:, None] == ext[None, :]) & ~torch.eye(m, dtype=torch.bool, device=dev)
    ok = ~same.any() & (info == 0) & torch.isfinite(a).all() & (a > 0).all()
    fallback = torch.where(in_F0[:, None], T, -inf).max(dim=0).values
    scale = torch.where(ok, (1.0 / a).to(dt), fallback)
    scale = torch.where(scale >= 1e-6, scale, torch.ones_like(scale))
    return ideal, scale, l


def nsga3_associate(Y: Tensor, ideal: Tensor, scale: Tensor, Z: Tensor, in_S: Tensor):
    """(niche (N,) long, dist (N,)): the direction nearest to each normalised
    row by perpendicular distance, ties to the lowest direction, and that
    distance, formed from the residual y' - (y'.z)z component by component.
    Rows outside ``in_S`` hold -1 / +inf."""
    yp = (Y - ideal) / scale
    Zt = Z.to(Y.dtype)
    zh = Zt / Zt.square().sum(dim=1, keepdim=True).sqrt()
    n, (H, m) = Y.shape[0], zh.shape
    niche = torch.empty(n, dtype=torch.long, device=Y.device)
    dist = torch.empty(n, dtype=Y.dtype, device=Y.device)
    step = max(1, (1 << 22) // (H * m))  # rows per (rows, H, m) block
    for i0 in range(0, n, step):
        y = yp[i0:i0 + step]
        dot = (y[:, None, :] * zh[None, :, :]).sum(dim=2)
        res = y[:, None, :] - dot[:, :, None] * zh[None, :, :]
        d = res.square().sum(dim=2).sqrt()
        h = d.argmin(dim=1)  # first minimum
        niche[i0:i0 + step] = h
        dist[i0:i0 + step] = d.gather(1, h[:, None])[:, 0]
    niche = torch.where(in_S, niche, torch.full_like(niche, -1))
    dist = torch.where(in_S, dist, torch.full_like(dist, float("inf")))
    return niche, dist


def nsga3_niche_sequential(rank, niche, dist, keep, H, dir_prio, row_prio) -> Tensor:
    """The textbook niching loop on the host, the oracle of nsga3_niche: P in
    (rank, index) order, then R times the direction with a candidate left and
    the smallest (niche count, dir_prio), its (dist, index)-minimal candidate
    while the count is zero and its row_prio-minimal one after that."""
    r, pi, d = rank.tolist(), niche.tolist(), dist.tolist()
    dp, rp = dir_prio.tolist(), row_prio.tolist()
    n = len(r)
    K = min(int(keep), n)
    l = 0
    while sum(1 for v in r if v <= l) < K:
        l += 1
    P = sorted((i for i in range(n) if r[i] < l), key=lambda i: (r[i], i))
    rho = [0] * H
    for i in P:
        rho[pi[i]] += 1
    cand = {}
    for i in range(n):
        if r[i] == l:
            cand.setdefault(pi[i], []).append(i)
    picks = []
    for _ in range(K - len(P)):
        h = min(cand, key=lambda h: (rho[h], dp[h]))
        if rho[h] == 0:
            i = min(cand[h], key=lambda i: (d[i], i))
        else:
            i = min(cand[h], key=lambda i: rp[i])
        cand[h].remove(i)
        if not cand[h]:
            del cand[h]  # exhausted: out of the race
        rho[h] += 1
        picks.append(i)
    return torch.tensor(P + picks, dtype=torch.long, device=rank.device)


def _segment_heads(sorted_keys: Tensor) -> Tensor:
    head = torch.ones_like(sorted_keys, dtype=torch.bool)
    head[1:] = sorted_keys[1:] != sorted_keys[:-1]
    return head


def nsga3_niche(rank, niche, dist, keep, H, dir_prio, row_prio) -> Tensor:
    """nsga3_niche_sequential in closed form. Each direction's candidates are
    listed: the (dist, index)-minimal one first where the initial niche count
    rho_h is 0, the others by row_prio. The candidate at position t gets the
    key (rho_h + t) H + dir_prio[h]; picking h raises rho_h alone, so the
    loop serves every direction at count c, in dir_prio order, before any at
    c + 1, and its picks are the R smallest keys in key order."""
    n = rank.shape[0]
    dev = rank.device
    K = min(int(keep), n)
    ar = torch.arange(n, device=dev)
    l = nsga3_level(rank, keep)
    in_P, in_F = rank < l, rank == l
    pi = niche.clamp(0, H - 1)
    rho = torch.zeros(H, dtype=torch.long, device=dev).scatter_add_(0, pi, in_P.long())
    seg = torch.where(in_F, pi, torch.full_like(pi, H))  # non-candidates last
    o = lexsort([dist, seg])  # by (direction, dist, index)
    is_first = torch.zeros(n, dtype=torch.bool, device=dev)
    is_first[o] = _segment_heads(seg[o])
    is_first &= in_F & (rho[pi] == 0)
    o = lexsort([row_prio, (~is_first).long(), seg])  # list order
    head = _segment_heads(seg[o])
    start = torch.cummax(torch.where(head, ar, torch.zeros_like(ar)), dim=0).values
    t = torch.empty_like(ar)
    t[o] = ar - start
    key = torch.where(
        in_F, (1 << 40) + (rho[pi] + t) * H + dir_prio[pi],
        torch.where(in_P, rank * n + ar,
                    torch.full_like(ar, torch.iinfo(torch.long).max)))
    return torch.argsort(key, stable=True)[:K]


def nsga3_select(parm, obj, keep, Z, dir_prio, row_prio, rank=None):
    """NSGA-III survival of the rows (parm, obj): (parm, obj, rank, perm,
    ideal, scale, niche, dist) with perm (min(keep, N),) the rows kept, P
    first in (rank, index) order, then the picks in pick order; niche / dist
    over all N rows. ``rank``: the Pareto rank of obj where the caller has it."""
    if rank is None:
        rank = pareto_rank(obj)
    ideal, scale, l = nsga3_normalize(obj, rank, keep)
    niche, dist = nsga3_associate(obj, ideal, scale, Z, rank <= l)
    perm = nsga3_niche(rank, niche, dist, keep, Z.shape[0], dir_prio, row_prio)
    return parm[perm], obj[perm], rank[perm], perm, ideal, scale, niche, dist
