"""Exact-GP math core — batched over hyperparameter candidates and objectives.

All heavy math flows through a small internal API (kernel build, Cholesky,
solves) so the gfx950 HIP kernels can replace the torch ops 1:1:

    K = signal_var * Matern_nu(||x-x'|| / ell) + noise_var * I

theta layout (log-space, sklearn-compatible ordering; reference
model.py:1227-1229): [log signal_var, log ell (1 or d values), log noise_var].

Reference semantics: per-objective sklearn GaussianProcessRegressor with
ConstantKernel*Matern(nu=2.5)+WhiteKernel, inputs scaled to [0,1], y
standardized (normalize_y=True), hyperparameters from SCE-UA on the negative
log marginal likelihood (reference model.py:1182-1275, 1419-1753).
"""

from __future__ import annotations

import contextlib
import math
from typing import Optional, Tuple

import torch

from dmosopt_amd import ops


def _strict_cpu_det() -> bool:
    import os

    return os.environ.get("DMOSOPT_CPU_STRICT_DET", "0") == "1"


@contextlib.contextmanager
def _single_threaded_cpu_math(enabled: bool):
    """OPT-IN (DMOSOPT_CPU_STRICT_DET=1): pin torch to ONE intra-op thread
    for a CPU numerics region.

    Defense against thread-team-dependent BLAS rounding. The same-seed
    reproducibility flake this was built for turned out to be the
    UNSEEDED surrogate search (profiles/README.md, determinism hunt) —
    with that fixed, 40/40 same-seed process pairs reproduce bitwise and
    direct MKL repeatability probes (200x nmll under load) never showed
    drift, so the ~8x CPU fit cost of sequential math is not paid by
    default. Enable for belt-and-braces CPU-rank determinism auditing."""
    if not (enabled and _strict_cpu_det()):
        yield
        return
    n0 = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n0)

SQRT5 = math.sqrt(5.0)
SQRT3 = math.sqrt(3.0)
LOG2PI = math.log(2.0 * math.pi)


def pairwise_sq_dists(X1: torch.Tensor, X2: torch.Tensor) -> torch.Tensor:
    """Squared euclidean distances, (..., N1, N2). Uses the |a|^2+|b|^2-2ab
    expansion so the inner product maps onto MFMA GEMM in the HIP kernel."""
    n1 = (X1 * X1).sum(dim=-1, keepdim=True)  # (..., N1, 1)
    n2 = (X2 * X2).sum(dim=-1, keepdim=True).transpose(-1, -2)  # (..., 1, N2)
    d2 = n1 + n2 - 2.0 * (X1 @ X2.transpose(-1, -2))
    return d2.clamp_min_(0.0)


def matern_from_d2(d2: torch.Tensor, nu: float) -> torch.Tensor:
    """Matern correlation from squared scaled distance r^2 = d2.

    sqrt is taken of d2 + tiny so autograd through the kernel diagonal
    (d2 == 0) yields finite gradients instead of the inf * 0 = NaN that
    d(sqrt)/d(d2)|_0 produces; the value perturbation is ~1e-12 in r.
    """
    if nu == 2.5:
        r = torch.sqrt(d2 + 1e-24)
        s = SQRT5 * r
        return (1.0 + s + (5.0 / 3.0) * d2) * torch.exp(-s)
    if nu == 1.5:
        r = torch.sqrt(d2 + 1e-24)
        s = SQRT3 * r
        return (1.0 + s) * torch.exp(-s)
    if nu == 0.5:
        return torch.exp(-torch.sqrt(d2 + 1e-24))
    if nu == float("inf") or nu is None:  # RBF
        return torch.exp(-0.5 * d2)
    raise ValueError(f"Unsupported Matern nu={nu}")


def build_kernel_torch(
    X1: torch.Tensor,
    X2: Optional[torch.Tensor],
    theta: torch.Tensor,
    nu: float = 2.5,
    anisotropic: bool = False,
    jitter: float = 0.0,
) -> torch.Tensor:
    """Kernel matrices for a BATCH of hyperparameters.

    X1: (N1, d); X2: (N2, d) or None (=X1, adds noise_var+jitter on diag).
    theta: (B, p) log-hyperparameters. Returns (B, N1, N2).
    """
    B = theta.shape[0]
    d = X1.shape[-1]
    sf2 = torch.exp(theta[:, 0])  # (B,)
    noise = torch.exp(theta[:, -1])  # (B,)
    sym = X2 is None
    if X2 is None:
        X2 = X1
    if anisotropic:
        ell = torch.exp(theta[:, 1 : 1 + d])  # (B, d)
        x1s = X1[None, :, :] / ell[:, None, :]
        x2s = X2[None, :, :] / ell[:, None, :]
        d2 = pairwise_sq_dists(x1s, x2s)  # (B, N1, N2)
    else:
        ell = torch.exp(theta[:, 1])  # (B,)
        d2 = pairwise_sq_dists(X1, X2)[None, :, :] / (ell * ell)[:, None, None]
    K = sf2[:, None, None] * matern_from_d2(d2, nu)
    if sym:
        n = X1.shape[0]
        idx = torch.arange(n, device=X1.device)
        K[:, idx, idx] += (noise + jitter)[:, None]
    return K


def build_kernel(
    X1: torch.Tensor,
    X2: Optional[torch.Tensor],
    theta: torch.Tensor,
    nu: float = 2.5,
    anisotropic: bool = False,
    jitter: float = 0.0,
) -> torch.Tensor:
    """Dispatching kernel build: gfx950 fused-assembly kernel on GPU,
    torch on CPU."""
    if X2 is None:
        return ops.matern_train_kernel(X1, theta, nu, anisotropic, jitter)
    return ops.matern_cross_kernel(X1, X2, theta, nu, anisotropic)


class _NmllGraph:
    """hipGraph-captured fused NMLL pipeline (gfx950).

    One SCE-UA fit issues ~170 fused-NMLL calls with IDENTICAL shapes (the
    stage batch is always 3*S*G candidates against the same X and the same
    per-candidate y rows) — each call a fixed ~27-launch pipeline (kernel
    assembly + 20 Cholesky panel/SYRK launches + solve + reduce) that is
    launch-gap bound at B ~ 18 workgroups. Capturing the pipeline once and
    replaying it turns those ~27 dispatches into 3 small D2D input copies +
    one graph launch. Inputs are copied into graph-owned buffers before
    replay, so allocator address reuse cannot alias stale data; X and y,
    constant within a fit, are copied only when their source changes
    (_bind), theta on every call."""

    def __init__(self, X, y, theta, nu, anisotropic, jitter):
        self.Xb = X.contiguous().clone()
        self.yb = y.contiguous().clone()
        self.tb = theta.contiguous().clone()
        self.args = (nu, anisotropic, jitter)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):  # warmup outside capture
                ops.gp_nmll_fused(self.Xb, self.tb, self.yb, nu, anisotropic, jitter)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = ops.gp_nmll_fused(
                self.Xb, self.tb, self.yb, nu, anisotropic, jitter
            )
        # NOTE: a hipMemsetAsync enqueued inside the captured region raced
        # with the following kernel's accumulation ON REPLAY (ROCm 7.2;
        # bit-nondeterministic outputs with bit-identical inputs,
        # scripts_det_debug6.py) — the multik Cholesky therefore zeroes
        # logdet with an explicit kernel (cholesky.hip zero_f32_kernel)
        # instead of a memset. Keep memsets out of captured pipelines.

        # static-input binding: (source tensor, its version) last copied
        # into Xb / yb. Holding the source keeps its id from being reused.
        self._bound = {"X": (None, -1), "y": (None, -1)}

    def _bind(self, slot, buf, src):
        """Copy src into the graph buffer unless it is the very tensor (same
        object, not written since) already copied there: within one fit X
        and the gathered per-row y never change, so every replay after the
        first skips two of the three D2D copies on the serial chain."""
        bound, version = self._bound[slot]
        if _nmll_bind_enabled() and bound is src and version == src._version:
            return
        buf.copy_(src)
        self._bound[slot] = (src, src._version)

    def run(self, X, y, theta):
        self._bind("X", self.Xb, X)
        self._bind("y", self.yb, y)
        self.tb.copy_(theta)
        self.graph.replay()
        # the clone stays: callers keep results across later replays
        return self.out.clone()


class _StageGraph:
    """One whole SCE-UA CCE stage as ONE captured linear chain (gfx950):
    propose -> kernel assembly with the factorization's prologue -> the
    Cholesky launches, the last one with the NMLL epilogue -> accept;
    ceil(N/32) + 3 kernel nodes, no memset node, no parallel branch. One
    replay is one stage: the two SCE-UA kernels read the stage's simplex
    positions and Philox seed from a per-shuffle schedule in device memory,
    selected by a device counter that accept advances, so a replay takes no
    argument. Every buffer the chain touches is owned here and static:
    the complexes ``cx`` / ``cf``, the candidates ``theta``, the NMLL side
    buffers, and one int32 control block [step (2) | act (S) | icall (S) |
    schedule (nspl, nps + 2)] that the host ships in ONE H2D per shuffle.
    The shuffle boundary (un-partition, global sort, partition, termination
    pack) runs on the same buffers with two native launches around
    torch.argsort and one pinned readback. X and the per-row y are bound as
    in _NmllGraph: copied only when the source object or its version
    changed."""

    def __init__(self, X, y, nu, anisotropic, jitter, S, G, npg, nps, nopt):
        dev = X.device
        N, B, npt, nspl = X.shape[0], 3 * S * G, G * npg, npg
        self.S, self.G, self.npg, self.nps, self.nopt = S, G, npg, nps, nopt
        self.nspl = nspl
        self.args = (nu, anisotropic, jitter)
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.Xb = X.contiguous().clone()
        self.yb = y.contiguous().clone()
        self._bound = {"X": (None, -1), "y": (None, -1)}
        self.bl = torch.zeros(nopt, **f32)
        self.bu = torch.zeros(nopt, **f32)
        self.cx = torch.zeros(S, G, npg, nopt, **f32)
        self.cf = torch.zeros(S, G, npg, **f32)
        self.x = torch.zeros(S, npt, nopt, **f32)  # un-partitioned, unsorted
        self.xf = torch.zeros(S, npt, **f32)
        self.xs = torch.zeros(S, npt, nopt, **f32)  # sorted population
        self.xfs = torch.zeros(S, npt, **f32)
        n_ctl = 2 + 2 * S + nspl * (nps + 2)
        self.ctl = torch.zeros(n_ctl, **i32)
        self.step = self.ctl[0:2]
        self.act = self.ctl[2 : 2 + S]
        self.icall = self.ctl[2 + S : 2 + 2 * S]
        self.sched = self.ctl[2 + 2 * S :].view(nspl, nps + 2)
        self._ctl_host = torch.zeros(n_ctl, dtype=torch.int32).pin_memory()
        self._ctl_np = self._ctl_host.numpy()
        self.theta = torch.zeros(B, nopt, **f32)
        self.K = torch.empty(B, N, N, **f32)
        self.Z = torch.empty(B, N, **f32)
        self.logdet = torch.empty(B, **f32)
        self.info = torch.empty(B, **i32)
        self.out = torch.empty(B, **f32)
        self.pack = torch.zeros(S, 2 + 2 * nopt, **f32)
        self._pack_host = torch.zeros(S, 2 + 2 * nopt).pin_memory()
        self._pack_np = self._pack_host.numpy()
        # warm-up and capture run on the zeroed buffers with act = 0: every
        # index is in range, accept leaves cx / cf alone, and each shuffle
        # re-ships the control block anyway
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._queue_stage()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._queue_stage()

    def _queue_stage(self):
        nu, anisotropic, jitter = self.args
        ops.sceua_propose_sched(
            self.cx, self.sched, self.step, self.bl, self.bu, self.theta
        )
        ops.gp_nmll_into(
            self.Xb, self.theta, self.yb, self.K, self.Z, self.logdet,
            self.info, self.out, nu, anisotropic, jitter,
        )
        ops.sceua_accept_sched(
            self.cx, self.cf, self.theta, self.out, self.sched, self.step,
            self.act, self.icall,
        )

    def bind(self, X, y, bl, bu):
        """Once per fit: X, the per-row y (skipped when already bound) and
        the search bounds."""
        for slot, buf, src in (("X", self.Xb, X), ("y", self.yb, y)):
            bound, version = self._bound[slot]
            if _nmll_bind_enabled() and bound is src and version == src._version:
                continue
            buf.copy_(src)
            self._bound[slot] = (src, src._version)
        self.bl.copy_(bl)
        self.bu.copy_(bu)

    def load_population(self, x, xf):
        """The sorted population (S,npt,nopt) / (S,npt) of the first shuffle,
        partitioned into the complexes: position p of complex g is row
        p*G + g."""
        S, G, npg, nopt = self.S, self.G, self.npg, self.nopt
        self.xs.copy_(x)
        self.xfs.copy_(xf)
        self.cx.copy_(x.view(S, npg, G, nopt).permute(0, 2, 1, 3))
        self.cf.copy_(xf.view(S, npg, G).permute(0, 2, 1))

    def begin_shuffle(self, act_np, lcs_np, seeds):
        """Ship one shuffle's control block: counter 0, the active-stream
        mask, zeroed icall, and per stage the simplex positions (nspl, nps)
        and the 64-bit seed."""
        S, nps = self.S, self.nps
        h = self._ctl_np
        h[: 2 + 2 * S] = 0
        h[2 : 2 + S] = act_np
        sched = h[2 + 2 * S :].reshape(self.nspl, nps + 2)
        sched[:, :nps] = lcs_np
        words = sched[:, nps:].view("uint32")
        for k, seed in enumerate(seeds):
            words[k, 0] = seed & 0xFFFFFFFF
            words[k, 1] = seed >> 32
        self.ctl.copy_(self._ctl_host, non_blocking=True)

    def stage(self):
        self.graph.replay()

    def end_shuffle(self):
        """Un-partition, global sort (torch.argsort, exactly the call of
        sceua.sort_pop: its tie order among failed candidates is part of the
        trajectory), partition back, and ONE blocking readback of the
        termination pack (S, 2 + 2 nopt): icall, best f, per-dimension max
        and min of the population. Afterwards xs / xfs hold the sorted
        population and cx / cf the next shuffle's complexes."""
        ops.sceua_unpartition(self.cx, self.cf, self.x, self.xf)
        order = torch.argsort(self.xf, dim=-1)
        ops.sceua_partition_pack(
            self.x, self.xf, order, self.icall, self.xs, self.xfs, self.cx,
            self.cf, self.pack,
        )
        self._pack_host.copy_(self.pack, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return self._pack_np


_nmll_graphs: dict = {}
_stage_graphs: dict = {}


def _evict_graphs_if_full():
    """Archives grow, so every epoch brings new shapes: both graph caches are
    dropped together once either holds 8 stale ones."""
    if len(_nmll_graphs) >= 8 or len(_stage_graphs) >= 8:
        _nmll_graphs.clear()
        _stage_graphs.clear()


def _nmll_graph_enabled() -> bool:
    import os

    return os.environ.get("DMOSOPT_NMLL_GRAPH", "1") == "1"


def _sceua_stage_enabled() -> bool:
    """DMOSOPT_SCEUA_STAGE=0 restores the per-stage propose / NMLL graph /
    accept path (same-process A/B; outputs are identical either way). Read
    per fit, not latched."""
    import os

    return os.environ.get("DMOSOPT_SCEUA_STAGE", "1") == "1"


def stage_graph(X, y, nu, anisotropic, jitter, S, G, npg, nps, nopt, bl, bu):
    """The captured CCE stage for this fit, bound to X (N,d), the per-row
    targets y (3*S*G, N) and the float32 bounds, or None where the native
    float32 gate does not hold or DMOSOPT_SCEUA_STAGE / DMOSOPT_NMLL_GRAPH
    switch it off. Cached on batched_nmll's shape key plus (S, G, npg, nps)."""
    if not (
        _sceua_stage_enabled()
        and _nmll_graph_enabled()
        and ops.native_fp32(X, y, bl, bu)
        and y.dim() == 2
        and y.shape[0] == 3 * S * G
    ):
        return None
    key = (
        y.shape[0], X.shape[0], X.shape[1], nopt, y.dim(), nu, anisotropic,
        float(jitter), S, G, npg, nps,
    )
    g = _stage_graphs.get(key)
    if g is None:
        _evict_graphs_if_full()
        g = _stage_graphs[key] = _StageGraph(
            X, y, nu, anisotropic, jitter, S, G, npg, nps, nopt
        )
    g.bind(X, y, bl, bu)
    return g


def _nmll_bind_enabled() -> bool:
    """DMOSOPT_NMLL_BIND=0 restores the unconditional input copies and the
    per-call y gather (same-box A/B; outputs are identical either way)."""
    import os

    return os.environ.get("DMOSOPT_NMLL_BIND", "1") == "1"


def batched_nmll(
    X: torch.Tensor,
    y: torch.Tensor,
    theta: torch.Tensor,
    nu: float = 2.5,
    anisotropic: bool = False,
    jitter: float = 1e-10,
    differentiable: bool = False,
) -> torch.Tensor:
    """Negative log marginal likelihood for a batch of theta.

    X: (N, d), y standardized targets: (N,) shared by all candidates, or
    (B, N) per-candidate rows (mixed-objective batches). theta: (B, p).
    Returns (B,). Failed factorizations get +inf (SCE-UA treats them as bad
    points). ``differentiable=True`` forces the autograd-capable torch path
    (Adam optimizer); the default dispatches to the fused gfx950 kernels.
    """
    with _single_threaded_cpu_math(not X.is_cuda):
        N = X.shape[0]
        B = theta.shape[0]

        def _yb():
            return (
                y[None, :, None].expand(B, N, 1) if y.dim() == 1 else y[:, :, None]
            ).contiguous()

        if differentiable:
            yb = _yb()
            K = build_kernel_torch(X, None, theta, nu=nu, anisotropic=anisotropic, jitter=jitter)
            L, info = torch.linalg.cholesky_ex(K)
            alpha = torch.cholesky_solve(yb, L)
            quad = (yb * alpha).sum(dim=(1, 2))
            logdet = 2.0 * torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(dim=-1)
        else:
            if ops.native_fp32(X) and _nmll_graph_enabled():
                key = (
                    B, N, X.shape[1], theta.shape[1], y.dim(), nu, anisotropic,
                    float(jitter),
                )
                g = _nmll_graphs.get(key)
                if g is None:
                    _evict_graphs_if_full()  # archives grow: drop stale shapes
                    g =_nmll_graphs[key] = _NmllGraph(
                        X.float(), y.float(), theta.float(), nu, anisotropic, jitter
                    )
                return g.run(X.float(), y.float(), theta.float())
            fused = ops.gp_nmll_fused(
                X, theta, y if y.dim() == 2 else y, nu, anisotropic, jitter
            )
            if fused is not None:
                return fused
            K = build_kernel(X, None, theta, nu=nu, anisotropic=anisotropic, jitter=jitter)
            L, half_logdet, info = ops.chol_factor_batched(K)
            # both paths return sum(log diag L)
            logdet = 2.0 * half_logdet
            z = ops.tri_solve_forward(L, _yb())  # L z = y
            quad = (z * z).sum(dim=(1, 2))
        nmll = 0.5 * quad + 0.5 * logdet + 0.5 * N * LOG2PI
        nmll = torch.where(info != 0, torch.full_like(nmll, float("inf")), nmll)
        nmll = torch.where(torch.isfinite(nmll), nmll, torch.full_like(nmll, float("inf")))
        return nmll


def batched_nmll_and_grad(
    X: torch.Tensor,
    y: torch.Tensor,
    theta: torch.Tensor,
    nu: float = 2.5,
    anisotropic: bool = False,
    jitter: float = 1e-10,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """NMLL and its analytic gradient in theta for a batch of theta.

    Arguments as in ``batched_nmll``: X (N, d), y (N,) shared or (B, N)
    per-candidate rows, theta (B, p) in log space. Returns (nmll (B,),
    grad (B, p)). With W = K^-1 - alpha alpha^T the gradient is the closed
    form 1/2 tr(W dK/dtheta) (docs/surrogates.md) — no autograd. A failed
    factorization or a non-finite value gives +inf, as in ``batched_nmll``,
    and a zero gradient row. Float32 GPU tensors run the fused gfx950
    pipeline (ops/hip/gp_nmll_grad.hip), whose nmll is bitwise that of the
    fused ``gp_nmll``; everything else runs ``torch_ref.gp_nmll_grad_ref``
    in the input dtype.
    """
    with _single_threaded_cpu_math(not X.is_cuda):
        return ops.gp_nmll_grad(X, theta, y, nu, anisotropic, jitter)


class FittedGP:
    """Posterior state for a batch of independent per-objective GPs sharing X.

    theta: (m, p) per-objective log-hyperparameters.
    """

    def __init__(
        self,
        X: torch.Tensor,
        Y: torch.Tensor,
        theta: torch.Tensor,
        y_mean: torch.Tensor,
        y_std: torch.Tensor,
        nu: float = 2.5,
        anisotropic: bool = False,
        jitter: float = 1e-10,
        compute: str = "fp32",
    ):
        self.X = X
        self.theta = theta
        self.nu = nu
        self.anisotropic = anisotropic
        self.y_mean = y_mean  # (m,)
        self.y_std = y_std  # (m,)
        # "bf16": posterior Cholesky uses bf16-MFMA trailing updates and
        # predictions use the bf16 cross kernel (BASELINE config #2); the
        # SCE-UA fit that produced theta is always fp32 (bit-stability)
        self.compute = compute if X.is_cuda else "fp32"
        m, N = theta.shape[0], X.shape[0]
        with _single_threaded_cpu_math(not X.is_cuda):
            self._build_posterior(X, Y, theta, y_mean, y_std, nu, anisotropic,
                                  jitter, m, N)

    def _build_posterior(self, X, Y, theta, y_mean, y_std, nu, anisotropic,
                         jitter, m, N):
        K = build_kernel(X, None, theta, nu=nu, anisotropic=anisotropic, jitter=jitter)
        if self.compute == "bf16":
            self.L, _, info = ops.chol_factor_batched_bf16(K)
        else:
            self.L, _, info = ops.chol_factor_batched(K)  # (m, N, N)
        # noise + the jitter each objective's L was actually factored with
        self.diag_add = torch.exp(theta[:, -1]) + jitter  # (m,)
        if int(info.sum()) != 0:
            # escalate jitter for failed objectives
            for _ in range(5):
                bad = info != 0
                if not bool(bad.any()):
                    break
                jitter *= 100.0
                K2 = build_kernel(
                    X, None, theta, nu=nu, anisotropic=anisotropic, jitter=jitter
                )
                L2, _, info = ops.chol_factor_batched(K2)
                self.L = torch.where(bad[:, None, None], L2, self.L)
                self.diag_add = torch.where(
                    bad, torch.exp(theta[:, -1]) + jitter, self.diag_add)
        Yn = (Y - y_mean[None, :]) / y_std[None, :]  # (N, m) standardized
        yb = Yn.T[:, :, None].contiguous()  # (m, N, 1)
        self.alpha = ops.chol_solve_batched(self.L, yb)  # (m, N, 1)
        # Kinv / Linv are built on the first variance request (properties
        # below): the default mean-only mode never reads either, and each
        # costs an N-right-hand-side solve per fit
        self._Kinv: Optional[torch.Tensor] = None
        self._Linv: Optional[torch.Tensor] = None

    def _eye(self) -> torch.Tensor:
        m, N = self.L.shape[0], self.L.shape[1]
        return torch.eye(N, dtype=self.L.dtype, device=self.L.device)[None].expand(
            m, N, N).contiguous()

    @property
    def Kinv(self) -> Optional[torch.Tensor]:
        """K^-1 on GPU (None on CPU), for the torch variance path: the
        quadratic term becomes a pair of batched GEMMs (rocBLAS/MFMA)
        instead of P triangular solves. Built lazily, cached."""
        if self._Kinv is None and self.X.is_cuda:
            self._Kinv = ops.chol_solve_batched(self.L, self._eye())
        return self._Kinv

    @property
    def Linv(self) -> torch.Tensor:
        """L^-1 (m, N, N), lower triangular, for the fused |Linv k*|^2
        variance kernel. Built lazily by the forward solve, cached."""
        if self._Linv is None:
            self._Linv = ops.tri_solve_forward(self.L, self._eye())
        return self._Linv

    def _destandardize(self, mean_n: torch.Tensor) -> torch.Tensor:
        """Standardized (m, P) posterior mean -> (P, m) in the units of Y."""
        return self.y_mean[None, :] + self.y_std[None, :] * mean_n.T

    def predict(self, Xq: torch.Tensor, return_var: bool = True):
        """Posterior mean and variance at Xq (P, d) -> ((P, m), (P, m)).

        Variance matches sklearn's return_std**2: diag K(x*,x*) [incl. noise
        from the White term] minus k*^T K^-1 k*, scaled by y_std^2. With
        ``return_var=False`` (the per-generation surrogate-evaluate path)
        the quadratic term is skipped and (mean, None) returned.
        """
        bf16 = self.compute == "bf16"
        if not return_var and not bf16:
            fused = ops.gp_predict_mean_fused(
                Xq, self.X, self.theta, self.alpha, self.y_mean, self.y_std,
                self.nu, self.anisotropic,
            )
            if fused is not None:
                return fused, None
        # deterministic CPU math (thread-team-independent): the replicated-
        # rank scheme compares these values across processes
        with _single_threaded_cpu_math(not Xq.is_cuda):
            if bf16:
                Ks = ops.matern_cross_bf16_kernel(
                    Xq.float(), self.X, self.theta, self.nu, self.anisotropic
                )
            else:
                Ks = build_kernel(Xq, self.X, self.theta, nu=self.nu,
                                  anisotropic=self.anisotropic)
            # The mean stays on this bmm chain with return_var=True as well:
            # evaluate() of a mean-only model comes through here (the inner
            # loop's initial population), and the fused gemv sums in another
            # order — last-bit differences there change every later
            # generation.
            mean_n = torch.bmm(Ks, self.alpha)[:, :, 0]  # (m, P)
            if not return_var:
                return self._destandardize(mean_n), None
            if self.compute == "fp32" and ops.native_fp32(Xq, self.X):
                mv = ops.gp_predict_mean_var_fused(
                    Xq, self.X, self.theta, self.alpha, self.Linv, self.y_mean,
                    self.y_std, self.nu, self.anisotropic,
                )
                return self._destandardize(mean_n), mv[:, self.theta.shape[0]:]
            return self._finish_var(Xq, Ks, mean_n)

    def predict_mean_grad(self, Xq: torch.Tensor):
        """Posterior mean and its gradient in the query point at normalized
        Xq (P, d) -> (mean (P, m), jac_u (P, m, d)), jac_u[p, b, k] =
        d mean[p, b] / d Xq[p, k] in unit-box input units and the units of Y.

        The closed form (docs/surrogates.md): float32 GPU fits run the fused
        kernels of ops/hip/gp_mean_grad.hip, everything else plain torch in
        the fit's dtype. It reads alpha and theta only, so a ``compute="bf16"``
        fit answers from the same float32 form."""
        with _single_threaded_cpu_math(not Xq.is_cuda):
            return ops.gp_predict_mean_grad(
                Xq, self.X, self.theta, self.alpha, self.y_mean, self.y_std,
                self.nu, self.anisotropic,
            )

    def sample_paths(self, n_paths: int = 1, n_features: int = 1024,
                     seed: Optional[int] = None) -> "GPPathSample":
        """Draw ``n_paths`` functions from the posterior of every objective
        (decoupled pathwise sampling, Wilson et al. 2020; formulas in
        docs/surrogates.md): a random-Fourier-feature prior draw with
        ``n_features`` cosines plus the Matheron update through the training
        data. Each draw is ONE consistent function that can be queried at
        new points any number of times.

        Batch row s * m + b is path s of objective b. Everything random comes
        from one CPU ``torch.Generator`` seeded with ``seed`` (unseeded: the
        generator's fixed default), in float64 and in this order, each block
        shaped (S, m, ...):

        1. ``randn(S, m, M, D)``   z, the spectral directions
        2. ``randn(S, m, M, 2 nu)`` n, whose mean square is g (Matern only;
           nothing is drawn for the RBF kernel, where g = 1)
        3. ``rand(S, m, M)``        tau, the phase offsets in turns
        4. ``randn(S, m, M)``       w, the feature weights
        5. ``randn(S, m, N)``       e, with eps = sqrt(diag_add) * e

        so CPU fits, GPU fits and every rank of one seed hold the same draws
        (a float32 fit differs from a float64 one only through its theta).
        Omega = z / (ell sqrt(g)) / (2 pi), tau and amp = sqrt(2 sf2 / M) w
        are stored rounded to float32, and the path is DEFINED by the stored
        values. A ``compute="bf16"`` fit answers from the float32 form: fp32
        cross kernel, and ``self.L`` as it is."""
        S, M = int(n_paths), int(n_features)
        if S < 1 or M < 1:
            raise ValueError("n_paths and n_features must be >= 1")
        m, (N, D) = self.theta.shape[0], self.X.shape
        g = torch.Generator(device="cpu")
        if seed is not None:
            g.manual_seed(int(seed))
        f64 = torch.float64
        theta = self.theta.detach().to("cpu", f64)
        z = torch.randn(S, m, M, D, generator=g, dtype=f64)
        if self.nu is None or self.nu == float("inf"):
            root_g = torch.ones(S, m, M, 1, dtype=f64)
        else:
            n = torch.randn(S, m, M, int(round(2 * self.nu)), generator=g, dtype=f64)
            root_g = torch.sqrt((n * n).mean(dim=-1, keepdim=True))
        tau = torch.rand(S, m, M, generator=g, dtype=f64)
        w = torch.randn(S, m, M, generator=g, dtype=f64)
        e = torch.randn(S, m, N, generator=g, dtype=f64)
        ell = torch.exp(theta[:, 1 : 1 + D] if self.anisotropic else theta[:, 1:2])
        Omega = z / (ell[None, :, None, :] * root_g) / (2.0 * math.pi)
        amp = torch.sqrt(2.0 * torch.exp(theta[:, 0]) / M)[None, :, None] * w
        dev, dt = self.X.device, self.X.dtype
        eps = (torch.sqrt(self.diag_add.detach().to("cpu", f64))[None, :, None] * e
               ).reshape(S * m, N).to(device=dev, dtype=dt)
        sample = GPPathSample(
            self, S,
            Omega.reshape(S * m, M, D).to(device=dev, dtype=torch.float32),
            tau.reshape(S * m, M).to(device=dev, dtype=torch.float32),
            amp.reshape(S * m, M).to(device=dev, dtype=torch.float32),
            eps,
        )
        with _single_threaded_cpu_math(not self.X.is_cuda):
            # f(X) through the routine the queries use, with no update term
            fX = sample._values(self.X, None, None, standardized=True).T  # (B, N)
            corr = ops.chol_solve_batched(
                self.L.repeat(S, 1, 1), (fX.to(dt) + eps)[:, :, None].contiguous()
            )
            # K^-1 (y_n - f(X) - eps), with K^-1 y_n the fit's alpha
            sample.alpha = (self.alpha[:, :, 0].repeat(S, 1) - corr[:, :, 0]).contiguous()
        return sample

    def _finish_var(self, Xq, Ks, mean_n):
        sf2 = torch.exp(self.theta[:, 0])
        noise = torch.exp(self.theta[:, -1])
        kss = (sf2 + noise)[:, None]  # (m, 1): k(x,x) = sf2*1 + noise
        if self.Kinv is not None:
            W = torch.bmm(Ks, self.Kinv)  # (m, P, N)
            quad = (Ks * W).sum(dim=2)  # (m, P)
        else:
            v = torch.linalg.solve_triangular(self.L, Ks.transpose(-1, -2), upper=False)
            quad = (v * v).sum(dim=1)
        var_n = (kss - quad).clamp_min(0.0)  # (m, P)
        var = (self.y_std[None, :] ** 2) * var_n.T
        return self._destandardize(mean_n), var


class GPPathSample:
    """``n_paths`` posterior sample paths of every objective of a FittedGP
    (FittedGP.sample_paths). Batch row s * m + b is path s of objective b:

        path(x) = y_mean_b + y_std_b (f(u) + k_b(u, X) alpha_row),
        f(u)    = sum_j amp_j cos(2 pi (tau_j + Omega_j . u)).

    Omega (B, M, D), tau (B, M) and amp (B, M) are float32 and define the
    path; eps (B, N) is the noise draw of the Matheron update and alpha
    (B, N) its weights K^-1 (y_n - f(X) - eps), both in the fit's dtype. At
    the training inputs path_n(X) = y_n - eps - diag_add * alpha holds
    whatever the number of features.
    """

    def __init__(self, fit: FittedGP, n_paths: int, Omega, tau, amp, eps):
        self.fit = fit
        self.n_paths = n_paths
        self.Omega, self.tau, self.amp, self.eps = Omega, tau, amp, eps
        S = n_paths
        self.theta = fit.theta.repeat(S, 1)
        self.y_mean = fit.y_mean.repeat(S)
        self.y_std = fit.y_std.repeat(S)
        self.alpha = torch.zeros_like(eps)
        self._pred: Optional[tuple] = None

    def _values(self, Xq, q_lb, q_invrg, standardized=False):
        """(P, B) path values at Xq (raw with q_lb / q_invrg, unit box
        without); ``standardized`` leaves y_mean / y_std out."""
        f = self.fit
        if standardized:
            y_mean, y_std = torch.zeros_like(self.y_mean), torch.ones_like(self.y_std)
        else:
            y_mean, y_std = self.y_mean, self.y_std
        if not standardized and ops.gp_mean_grad_native(Xq, f.X):
            if self._pred is None or self._pred[0] is not self.alpha:
                # per-draw arguments of the native call, converted once
                self._pred = (self.alpha, ops.gp_pred_args(
                    f.X, self.theta, self.alpha, y_mean, y_std, f.nu, f.anisotropic))
            return ops.gp_predict_path_cached(
                Xq.float().contiguous(), self._pred[1], self.Omega, self.tau,
                self.amp, q_lb, q_invrg,
            )
        return ops.gp_predict_path(
            Xq, f.X, self.theta, self.alpha, y_mean, y_std, f.nu, f.anisotropic,
            self.Omega, self.tau, self.amp, q_lb, q_invrg,
        )

    def _shape(self, vals: torch.Tensor) -> torch.Tensor:
        m = self.fit.theta.shape[0]
        return vals if self.n_paths == 1 else vals.reshape(-1, self.n_paths, m)

    def evaluate_normalized(self, Xq: torch.Tensor) -> torch.Tensor:
        """Path values at unit-box queries Xq (P, d) -> (P, S, m) in the units
        of Y, (P, m) when S = 1."""
        with _single_threaded_cpu_math(not Xq.is_cuda):
            return self._shape(self._values(Xq, None, None))

    def evaluate_affine(self, Xq, q_lb, q_invrg) -> torch.Tensor:
        """evaluate_normalized at u = (Xq - q_lb) * q_invrg for raw queries;
        on the native path the affine is applied inside the kernel loads."""
        with _single_threaded_cpu_math(not Xq.is_cuda):
            return self._shape(self._values(Xq, q_lb, q_invrg))
