"""GP surrogate models (surrogate duck-type: __init__(xin, yin, nInput,
nOutput, xlb, xub, **kw), predict(x) -> (mean, var), evaluate(x)).

GPRMatern ('gpr', the default) mirrors the reference GPR_Matern
(model.py:1182-1275): per-objective exact GP with ConstantKernel x
Matern(nu=2.5) + WhiteKernel, inputs normalized to [0,1], normalize_y,
hyperparameters from SCE-UA over the negative log marginal likelihood — but
all objectives fit as ONE batched SCE-UA run (models/sceua.py) and all
posterior math is batched over objectives (models/gp_core.py), targeting a
handful of large device launches per epoch.

EGPMatern ('egp') is the gradient-based alternative (reference
model_gpytorch.py:1929-2235's role): Adam on the exact MLL via autograd,
ARD lengthscales by default.
"""

from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from dmosopt_amd import ops
from dmosopt_amd.models.gp_core import (
    FittedGP,
    _nmll_bind_enabled,
    batched_nmll,
    batched_nmll_and_grad,
    stage_graph,
)
from dmosopt_amd.models.sceua import sceua_batched


def _top_k_mo(x: np.ndarray, y: np.ndarray, top_k):
    """Keep the top_k rows by non-dominated sort (reference MOEA.py:350-372)."""
    xt, yt = ops.top_k_mo(
        torch.as_tensor(x, dtype=torch.float64),
        torch.as_tensor(y, dtype=torch.float64),
        top_k,
    )
    return xt.numpy() if xt is not x else x, yt.numpy() if yt is not y else y


#: Thompson mode draws its path from a generator seeded with the model's
#: ``seed`` plus this offset
THOMPSON_SEED_OFFSET = 1


class GPPath:
    """Posterior sample paths of a GP model in the model's raw input units
    (``model.sample_paths``): every call of ``evaluate`` / ``evaluate_tensor``
    queries the SAME drawn functions. Values are (P, m), or (P, S, m) for
    S = n_paths > 1. ``sample`` is the gp_core.GPPathSample behind it."""

    def __init__(self, model, sample):
        self._model = model
        self.sample = sample

    def evaluate(self, x) -> np.ndarray:
        """Raw numpy x (P, d) or (d,) -> float64 path values."""
        mdl = self._model
        xin = np.asarray(x, dtype=np.float64)
        if xin.ndim == 1:
            xin = xin.reshape(1, mdl.nInput)
        xn = (xin - mdl.xlb[None, :]) / mdl.xrg[None, :]
        Xq = torch.as_tensor(xn, dtype=mdl.dtype, device=mdl.device)
        return self.sample.evaluate_normalized(Xq).cpu().numpy().astype(np.float64)

    def evaluate_tensor(self, x: torch.Tensor) -> torch.Tensor:
        """Raw device tensor x (P, d) -> device tensor, no host trip; on the
        native path the per-dimension normalization happens inside the
        kernel loads."""
        mdl = self._model
        xr = x.to(mdl.device, mdl.dtype)
        if ops.gp_mean_grad_native(xr, mdl._fitted.X):
            cache, _ = mdl._native_pred_cache(xr.device)
            return self.sample.evaluate_affine(xr.contiguous(), cache[1], cache[2])
        return self.sample.evaluate_normalized(mdl.normalize_query(xr))


class _GPRBase:
    nu: float = 2.5
    #: fitted state is fully determined by (archive, theta): the engine may
    #: run the hyperparameter search on rank 0 only and broadcast theta
    #: (core/engine.py train())
    supports_theta_broadcast = True

    def __init__(
        self,
        xin,
        yin,
        nInput,
        nOutput,
        xlb,
        xub,
        optimizer="sceua",
        seed=None,
        length_scale_bounds=(1e-3, 100.0),
        constant_kernel_bounds=(1e-4, 1e3),
        noise_level_bounds=(1e-9, 1e-2),
        anisotropic=False,
        return_mean_variance=False,
        nan="remove",
        top_k=None,
        adam_lr=0.08,
        adam_iters=150,
        grad_restarts=8,
        grad_iters=200,
        grad_lr=0.5,
        batch_size=None,
        device=None,
        dtype=None,
        compute="fp32",
        logger=None,
        theta_override=None,
        thompson=False,
        path_features=1024,
        **kwargs,
    ):
        if thompson and return_mean_variance:
            raise ValueError(
                "thompson=True optimizes one posterior sample path per "
                "objective; it cannot be combined with return_mean_variance=True"
            )
        #: Thompson-sampling mode: evaluate / evaluate_tensor answer from ONE
        #: posterior sample path drawn right after the fit (n_features =
        #: path_features, seed = THOMPSON_SEED_OFFSET + the model's seed);
        #: predict, gradient* and evaluate_mean_variance_tensor stay the
        #: posterior's
        self.thompson = bool(thompson)
        self.path_features = int(path_features)
        self._thompson_path: Optional[GPPath] = None
        self.nInput = nInput
        self.nOutput = nOutput
        self.xlb = np.asarray(xlb, dtype=np.float64)
        self.xub = np.asarray(xub, dtype=np.float64)
        self.xrg = self.xub - self.xlb
        self.xrg[self.xrg == 0] = 1.0
        self.logger = logger
        self.return_mean_variance = return_mean_variance
        self.anisotropic = anisotropic
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        )
        self.dtype = dtype or (torch.float64 if self.device.type == "cpu" else torch.float32)
        # "bf16": bf16-MFMA posterior path (predictions + trailing Cholesky
        # updates); the hyperparameter SEARCH below is always fp32
        self.compute = compute

        xin = np.asarray(xin, dtype=np.float64)
        yin = np.asarray(yin, dtype=np.float64)
        if yin.ndim == 1:
            yin = yin.reshape(-1, 1)
        if nan is not None:
            yt, xt = ops.filter_samples(
                torch.as_tensor(yin), torch.as_tensor(xin), nan=nan
            )
            xin, yin = xt.numpy(), yt.numpy()
        xin, yin = _top_k_mo(xin, yin, top_k)
        yin = np.nan_to_num(yin)

        xn = (xin - self.xlb[None, :]) / self.xrg[None, :]
        X = torch.as_tensor(xn, dtype=self.dtype, device=self.device)
        Y = torch.as_tensor(yin, dtype=self.dtype, device=self.device)
        y_mean = Y.mean(dim=0)
        y_std = Y.std(dim=0, unbiased=False).clamp_min(1e-12)

        m = nOutput
        n_ell = nInput if anisotropic else 1
        nopt = 1 + n_ell + 1
        bl = np.concatenate(
            [
                [math.log(constant_kernel_bounds[0])],
                [math.log(length_scale_bounds[0])] * n_ell,
                [math.log(noise_level_bounds[0])],
            ]
        )
        bu = np.concatenate(
            [
                [math.log(constant_kernel_bounds[1])],
                [math.log(length_scale_bounds[1])] * n_ell,
                [math.log(noise_level_bounds[1])],
            ]
        )
        Yn = (Y - y_mean[None, :]) / y_std[None, :]

        if theta_override is not None:
            # broadcast-received hyperparameters: skip the search, rebuild
            # the posterior (Cholesky + alpha) locally from the archive
            theta = torch.as_tensor(
                np.asarray(theta_override), dtype=self.dtype, device=self.device
            )
            assert theta.shape == (m, nopt), (theta.shape, (m, nopt))
            self._fitted = FittedGP(
                X, Y, theta, y_mean, y_std, nu=self.nu, anisotropic=anisotropic,
                jitter=1e-10 if self.dtype == torch.float64 else 1e-6,
                compute=self.compute,
            )
            self.theta = theta
            self._draw_thompson_path(seed)
            return

        if optimizer == "dlib" and logger is not None:
            logger.warning(
                "GP optimizer 'dlib' (reference model.py:1367-1416 optional "
                "dlib.find_min_global path) is served by the batched SCE-UA "
                "search here; dlib is not a dependency of this framework"
            )
        if optimizer in ("sceua", "dlib", None):
            YnT = Yn.T.contiguous()  # (m, N)

            # gathered per-row targets, cached per stream-id tensor: SCE-UA
            # passes the SAME tensor object on every stage call, so the
            # gather runs once per fit instead of once per call, and the
            # NMLL graph sees the same y tensor and skips its input copy
            y_rows: dict = {}

            def rows_for(stream: torch.Tensor) -> torch.Tensor:
                if not _nmll_bind_enabled():
                    return YnT[stream]
                hit = y_rows.get(id(stream))
                if hit is None or hit[0] is not stream or hit[1] != stream._version:
                    hit = y_rows[id(stream)] = (stream, stream._version, YnT[stream])
                return hit[2]

            def nmll_func(theta_batch: torch.Tensor, stream: torch.Tensor):
                # one fused batched call for ALL streams: per-row y targets
                return batched_nmll(
                    X, rows_for(stream), theta_batch.to(self.dtype),
                    nu=self.nu, anisotropic=anisotropic,
                )

            def stage_runner(sid3, S, G, npg, nps, nopt_, bl_f, bu_f):
                # the whole CCE stage as one captured launch chain where the
                # native float32 gate holds (None elsewhere: sceua_batched
                # then calls nmll_func per stage as before)
                return stage_graph(
                    X, rows_for(sid3), self.nu, anisotropic, 1e-10, S, G, npg,
                    nps, nopt_, bl_f, bu_f,
                )

            bestx, bestf, icall = sceua_batched(
                nmll_func, bl, bu, nopt, n_streams=m, seed=seed,
                device=self.device, dtype=self.dtype, logger=None,
                stage_runner=stage_runner,
            )
            theta = torch.as_tensor(bestx, dtype=self.dtype, device=self.device)
        elif optimizer == "adam":
            theta = self._fit_adam(X, Yn, bl, bu, nopt, m, adam_lr, adam_iters, seed)
        elif optimizer == "grad":
            theta = self._fit_grad(
                X, Yn, bl, bu, m, grad_restarts, grad_iters, grad_lr, seed
            )
        else:
            raise ValueError(f"Unknown GP optimizer {optimizer!r}")

        self._fitted = FittedGP(
            X, Y, theta, y_mean, y_std, nu=self.nu, anisotropic=anisotropic,
            jitter=1e-10 if self.dtype == torch.float64 else 1e-6,
            compute=self.compute,
        )
        self.theta = theta
        self._draw_thompson_path(seed)

    def _draw_thompson_path(self, seed):
        """Thompson mode: draw the path the inner optimizer will see. Its
        seed is ``seed + THOMPSON_SEED_OFFSET`` (None stays None), so the draw
        never shares a generator state with the hyperparameter search, which
        seeds its own streams with ``seed`` itself; archive, theta and seed
        are replicated, so every rank draws the same path."""
        if self.thompson:
            self._thompson_path = self.sample_paths(
                1, self.path_features,
                None if seed is None else int(seed) + THOMPSON_SEED_OFFSET,
            )

    def _fit_adam(self, X, Yn, bl, bu, nopt, m, lr, iters, seed):
        g = torch.Generator(device="cpu")
        if seed is not None:
            g.manual_seed(int(seed))
        bl_t = torch.as_tensor(bl, dtype=self.dtype, device=self.device)
        bu_t = torch.as_tensor(bu, dtype=self.dtype, device=self.device)
        init = self._adam_init(bl_t, bu_t, m)
        theta = init.clone().requires_grad_(True)
        opt = torch.optim.Adam([theta], lr=lr)
        best_theta = init.clone()
        best_loss = torch.full((m,), float("inf"), dtype=self.dtype, device=self.device)
        for _ in range(iters):
            opt.zero_grad(set_to_none=True)
            losses = []
            for s in range(m):
                nm = batched_nmll(
                    X, Yn[:, s], theta[s : s + 1], nu=self.nu,
                    anisotropic=self.anisotropic, jitter=1e-8,
                    differentiable=True,
                )
                losses.append(nm)
            loss_vec = torch.cat(losses)
            finite = torch.isfinite(loss_vec)
            if not bool(finite.any()):
                break
            with torch.no_grad():
                better = finite & (loss_vec < best_loss)
                best_loss = torch.where(better, loss_vec.detach(), best_loss)
                best_theta[better] = theta.detach()[better]
            loss_vec.masked_fill(~finite, 0.0).sum().backward()
            if not torch.isfinite(theta.grad).all():
                theta.grad.zero_()
            opt.step()
            with torch.no_grad():
                theta.clamp_(bl_t, bu_t)
                theta.nan_to_num_(nan=0.0)
        return best_theta

    def _adam_init(self, bl_t, bu_t, m):
        """_fit_adam's initial point (sf2=1, ell=0.5, noise=1e-6: the
        reference defaults), (m, p)."""
        init = 0.5 * (bl_t + bu_t)[None, :].repeat(m, 1)
        init[:, 0] = 0.0
        init[:, 1:-1] = math.log(0.5)
        init[:, -1] = math.log(1e-6)
        return init

    def _grad_starts(self, bl, bu, m, restarts, seed):
        """(restarts, m, p) start points of the multi-start gradient fit:
        start 0 is _fit_adam's initial point clipped to the box, the others
        are uniform in the box from a CPU generator seeded with ``seed``
        (drawn in float64 on the host, so CPU and GPU fits of one seed start
        from the same points)."""
        g = torch.Generator(device="cpu")
        if seed is not None:
            g.manual_seed(int(seed))
        bl64 = torch.as_tensor(bl, dtype=torch.float64)
        bu64 = torch.as_tensor(bu, dtype=torch.float64)
        starts = torch.empty(restarts, m, bl64.numel(), dtype=torch.float64)
        starts[0] = torch.minimum(
            torch.maximum(self._adam_init(bl64, bu64, m), bl64), bu64
        )
        if restarts > 1:
            u = torch.rand(restarts - 1, m, bl64.numel(), generator=g,
                           dtype=torch.float64)
            starts[1:] = bl64 + u * (bu64 - bl64)
        return starts.to(device=self.device, dtype=self.dtype)

    def _fit_grad(self, X, Yn, bl, bu, m, restarts, iters, lr, seed):
        """Multi-start projected Adam on the analytic NMLL gradient.

        All restarts x m candidates advance together: one
        batched_nmll_and_grad call (on the GPU one fused extension call:
        assemble, Cholesky, solves, gradient kernels) per iteration, then an
        Adam step in log space clamped to the SCE-UA box [bl, bu], with the
        learning rate on a cosine from ``lr`` to 0 over ``iters``. The best
        finite NMLL of every candidate over all iterations is tracked on the
        device (no host sync inside the loop); the result for an objective is
        its best candidate over the restarts. The search evaluates the same
        NMLL as the SCE-UA search (same jitter), so the two are comparable."""
        restarts, iters = int(restarts), int(iters)
        if restarts < 1 or iters < 0:
            raise ValueError("grad_restarts must be >= 1 and grad_iters >= 0")
        bl_t = torch.as_tensor(bl, dtype=self.dtype, device=self.device)
        bu_t = torch.as_tensor(bu, dtype=self.dtype, device=self.device)
        p = bl_t.numel()
        theta = self._grad_starts(bl, bu, m, restarts, seed).reshape(restarts * m, p)
        theta = torch.minimum(torch.maximum(theta, bl_t), bu_t)
        y_rows = Yn.T.contiguous().repeat(restarts, 1)  # row r*m+s -> objective s
        best_theta = theta.clone()
        best_f = torch.full((restarts * m,), float("inf"), dtype=self.dtype,
                            device=self.device)
        m1 = torch.zeros_like(theta)
        m2 = torch.zeros_like(theta)
        beta1, beta2, eps = 0.9, 0.999, 1e-8
        for t in range(iters + 1):
            f, g = batched_nmll_and_grad(
                X, y_rows, theta, nu=self.nu, anisotropic=self.anisotropic
            )
            better = torch.isfinite(f) & (f < best_f)
            best_f = torch.where(better, f, best_f)
            best_theta = torch.where(better[:, None], theta, best_theta)
            if t == iters:
                break
            g = torch.where(torch.isfinite(g), g, torch.zeros_like(g))
            m1 = beta1 * m1 + (1.0 - beta1) * g
            m2 = beta2 * m2 + (1.0 - beta2) * g * g
            step = 0.5 * lr * (1.0 + math.cos(math.pi * t / iters))
            upd = (m1 / (1.0 - beta1 ** (t + 1))) / (
                torch.sqrt(m2 / (1.0 - beta2 ** (t + 1))) + eps
            )
            theta = torch.minimum(torch.maximum(theta - step * upd, bl_t), bu_t)
        pick = torch.argmin(best_f.view(restarts, m), dim=0)  # (m,)
        cols = torch.arange(m, device=self.device)
        #: best NMLL found per objective (device tensor, search jitter)
        self.fit_nmll = best_f.view(restarts, m)[pick, cols]
        return best_theta.view(restarts, m, p)[pick, cols].contiguous()

    # ---------------------------------------------------------------- API
    def predict(self, xin):
        xin = np.asarray(xin, dtype=np.float64)
        if xin.ndim == 1:
            xin = xin.reshape(1, self.nInput)
        xn = (xin - self.xlb[None, :]) / self.xrg[None, :]
        Xq = torch.as_tensor(xn, dtype=self.dtype, device=self.device)
        mean, var = self._fitted.predict(Xq)
        return mean.cpu().numpy().astype(np.float64), var.cpu().numpy().astype(np.float64)

    def predict_tensor(self, Xq_normalized: torch.Tensor):
        """Device-resident predict for the inner MOEA loop: takes ALREADY
        normalized inputs on the model device, returns device tensors."""
        return self._fitted.predict(Xq_normalized)

    def normalize_query(self, xin: torch.Tensor) -> torch.Tensor:
        # cache the bounds tensors: re-uploading two tiny arrays is two H2D
        # transfers per surrogate evaluation (every generation)
        cache = getattr(self, "_nq_cache", None)
        key = (xin.dtype, xin.device)
        if cache is None or cache[0] != key:
            lb = torch.as_tensor(self.xlb, dtype=xin.dtype, device=xin.device)
            rg = torch.as_tensor(self.xrg, dtype=xin.dtype, device=xin.device)
            self._nq_cache = cache = (key, lb, rg)
        return (xin - cache[1]) / cache[2]

    def sample_paths(self, n_paths=1, n_features=1024, seed=None) -> GPPath:
        """Draw ``n_paths`` functions from every objective's posterior
        (FittedGP.sample_paths: ``n_features`` random Fourier features plus
        the Matheron update, everything random from one generator seeded with
        ``seed``). Returns a GPPath with ``evaluate(x)`` (raw numpy in,
        float64 out) and ``evaluate_tensor(x)`` (raw device tensor in, device
        tensor out). A ``compute="bf16"`` model answers from the float32
        form."""
        return GPPath(self, self._fitted.sample_paths(n_paths, n_features, seed))

    def evaluate(self, x):
        if self._thompson_path is not None:
            return self._thompson_path.evaluate(x)
        mean, var = self.predict(x)
        if self.return_mean_variance:
            return mean, var
        return mean

    def _native_pred_cache(self, device):
        """(affine cache, per-fit predict args) for the fused native predict
        calls. Raw queries: the per-dim normalization happens inside the
        cross-kernel load (two fewer launches per generation). The static
        per-fit args are cached once: the generation loop is host-dispatch-
        bound, and re-checking contiguity/dtype of six unchanged tensors
        every call costs ~8 us of host time."""
        cache = getattr(self, "_affine_cache", None)
        if cache is None or cache[0] != device:
            lb = torch.as_tensor(self.xlb, dtype=torch.float32, device=device)
            invrg = torch.as_tensor(
                1.0 / self.xrg, dtype=torch.float32, device=device
            )
            self._affine_cache = cache = (device, lb, invrg)
        f = self._fitted
        pa = getattr(f, "_pred_args", None)
        if pa is None:
            pa = f._pred_args = ops.gp_pred_args(
                f.X, f.theta, f.alpha, f.y_mean, f.y_std, f.nu, f.anisotropic
            )
        return cache, pa

    @property
    def supports_device_mean_variance(self) -> bool:
        """True when evaluate_mean_variance_tensor is available: a float32
        GPU model with fp32 compute on the native path."""
        return self.compute == "fp32" and ops.native_fp32(self._fitted.X)

    def evaluate_mean_variance_tensor(self, x: torch.Tensor) -> torch.Tensor:
        """Device-resident mean-variance evaluate: (P, 2m) float32 laid out
        [mean | round(var, 6)], no host trip. The variance is the fused
        |Linv k*|^2 form (ops/hip/gp_variance.hip); the mean columns are
        bitwise those of evaluate_tensor on a mean-only model."""
        if not self.supports_device_mean_variance:
            raise RuntimeError(
                "evaluate_mean_variance_tensor needs a float32 GPU model with "
                "fp32 compute and the native extension; use evaluate()"
            )
        xr = x.to(self.device, torch.float32)
        cache, pa = self._native_pred_cache(xr.device)
        f = self._fitted
        linv = getattr(f, "_pred_linv", None)
        if linv is None:
            linv = f._pred_linv = f.Linv.contiguous().float()
        return ops.gp_predict_mean_var_cached(
            xr.contiguous(), pa, linv, cache[1], cache[2], 6
        )

    def evaluate_tensor(self, x: torch.Tensor) -> torch.Tensor:
        """Device-resident evaluate: tensor in, tensor out, no host trip. In
        Thompson mode the values are those of the model's sample path."""
        if self._thompson_path is not None:
            return self._thompson_path.evaluate_tensor(x)
        xr = x.to(self.device, self.dtype)
        if (
            not self.return_mean_variance
            and self.compute != "bf16"
            and ops.native_fp32(self._fitted.X)
        ):
            cache, pa = self._native_pred_cache(xr.device)
            return ops.gp_predict_mean_cached(
                xr.contiguous(), pa, cache[1], cache[2]
            )
        xq = self.normalize_query(xr)
        mean, _ = self._fitted.predict(xq, return_var=self.return_mean_variance)
        return mean

    def native_mean_args(self, device):
        """The arguments evaluate_tensor gives the native posterior-mean call
        after the queries — (X, theta, alpha, y_mean, y_std, nu, anisotropic,
        q_lb, q_invrg) — for a caller that queues the same launches itself
        (the NSGA-II chunk driver); None where evaluate_tensor would not take
        the float32 native mean path on ``device`` (Thompson mode included:
        its evaluate_tensor is a sample path, not the mean)."""
        device = torch.device(device)
        if (
            self.return_mean_variance
            or self._thompson_path is not None
            or self.compute == "bf16"
            or self.dtype != torch.float32
            or device.type != "cuda"
            or torch.device(self.device) != device
            or not ops.native_fp32(self._fitted.X)
        ):
            return None
        cache, pa = self._native_pred_cache(device)
        return tuple(pa) + (cache[1], cache[2])

    def gradient_tensor(self, x: torch.Tensor) -> torch.Tensor:
        """Device-resident gradient of the posterior mean in the query point:
        raw x (P, d) -> (P, m, d), [p, b, k] = d mean_b(x_p) / d x_k in raw
        input units, no host trip. The analytic closed form
        (docs/surrogates.md); ``return_mean_variance`` changes nothing, and a
        ``compute="bf16"`` model answers from the float32 form."""
        xr = x.to(self.device, self.dtype)
        f = self._fitted
        if ops.gp_mean_grad_native(xr, f.X):
            cache, pa = self._native_pred_cache(xr.device)
            return ops.gp_predict_mean_grad_cached(
                xr.contiguous(), pa, cache[1], cache[2]
            )[1]
        _, jac_u = f.predict_mean_grad(self.normalize_query(xr))
        rg = torch.as_tensor(self.xrg, dtype=jac_u.dtype, device=jac_u.device)
        return jac_u / rg

    def gradient(self, x) -> np.ndarray:
        """Gradient of the posterior mean at raw x (P, d) or (d,) ->
        float64 (P, m, d) in raw input units (see gradient_tensor)."""
        xin = np.asarray(x, dtype=np.float64)
        if xin.ndim == 1:
            xin = xin.reshape(1, self.nInput)
        jac = self.gradient_tensor(torch.as_tensor(xin))
        return jac.cpu().numpy().astype(np.float64)


class GPRMatern(_GPRBase):
    """Registry name 'gpr' — Matern-5/2 exact GP (reference model.py:1182)."""

    nu = 2.5


class GPRRBF(_GPRBase):
    """RBF kernel variant (reference model.py:1278 GPR_RBF)."""

    nu = float("inf")


class EGPMatern(_GPRBase):
    """Registry name 'egp' — gradient-fit exact GP, ARD lengthscales.

    Plays the role of the reference's GPyTorch EGP_Matern
    (model_gpytorch.py:1929-2235): Adam on the exact marginal likelihood.
    """

    nu = 2.5

    def __init__(self, xin, yin, nInput, nOutput, xlb, xub, **kwargs):
        kwargs.setdefault("optimizer", "adam")
        kwargs.setdefault("anisotropic", True)
        super().__init__(xin, yin, nInput, nOutput, xlb, xub, **kwargs)


class MEGPMatern(_GPRBase):
    """Registry name 'megp' — multitask exact GP.

    Round-1 implementation: batched per-task exact GPs with shared ARD
    kernel hyperparameters fit jointly (sum of per-task MLLs), standing in
    for the reference's Kronecker multitask GP (model_gpytorch.py:1623-1928).
    Full task-covariance (ICM) model is planned.
    """

    nu = 2.5

    def __init__(self, xin, yin, nInput, nOutput, xlb, xub, **kwargs):
        kwargs.setdefault("optimizer", "adam")
        kwargs.setdefault("anisotropic", True)
        super().__init__(xin, yin, nInput, nOutput, xlb, xub, **kwargs)
