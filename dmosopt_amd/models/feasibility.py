"""Feasibility models (registry names 'logreg' and 'gp').

Interface parity with the reference LogisticFeasibilityModel
(feasibility.py:14-67): per-constraint classifier of P(c_i > 0) with
``predict``, ``predict_proba`` (stacked [P(infeasible), P(feasible)]) and
``rank`` (mean feasible probability — used as an x-distance metric by the
optimizers).

Implementation is torch-native instead of sklearn GridSearchCV pipelines:
standardize -> PCA (SVD) -> L1-regularized logistic regression fit with
batched full-gradient Adam + soft-threshold proximal step, with the
regularization strength chosen by a small validation grid — one batched fit
per constraint, device-capable.

GPFeasibilityModel ('gp') has no reference counterpart: a batched Matern GP
regressed on the constraint VALUES, whose posterior gives the probability of
feasibility Phi(mean / sd) of constrained Bayesian optimisation, with a
device-resident ``rank_tensor`` for the optimizers (docs/surrogates.md).
"""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch


class _TorchLogregBatch:
    """G independent L1-logistic fits as ONE batched Adam run: W is (G, d),
    the loss is the sum of per-column BCEs (gradients stay independent), the
    proximal soft-threshold applies per-column lambda. Replaces the former
    per-candidate sequential loop (the whole regularization grid now costs
    one optimization, with a plateau early stop)."""

    def __init__(self, X: torch.Tensor, c: torch.Tensor, l1s, iters: int = 300):
        n, d = X.shape
        l1s = torch.as_tensor(np.asarray(l1s, dtype=np.float64), dtype=X.dtype,
                              device=X.device)
        G = l1s.shape[0]
        W = torch.zeros(G, d, dtype=X.dtype, device=X.device, requires_grad=True)
        b = torch.zeros(G, dtype=X.dtype, device=X.device, requires_grad=True)
        opt = torch.optim.Adam([W, b], lr=0.1)
        lam = (l1s / n)[:, None]
        ct = c[:, None].expand(n, G)
        prev = None
        for it in range(iters):
            opt.zero_grad(set_to_none=True)
            logits = X @ W.T + b[None, :]
            loss = torch.nn.functional.binary_cross_entropy_with_logits(
                logits, ct, reduction="mean"
            )
            loss.backward()
            opt.step()
            with torch.no_grad():  # proximal soft-threshold for L1
                step = 0.1 * lam
                W.copy_(torch.sign(W) * (W.abs() - step).clamp_min(0.0))
            if it % 25 == 24:
                cur = float(loss.detach())
                if prev is not None and abs(prev - cur) < 1e-7:
                    break
                prev = cur
        self.W = W.detach()
        self.b = b.detach()

    def proba_all(self, X: torch.Tensor) -> torch.Tensor:
        """(n, G) feasibility probabilities per grid candidate."""
        return torch.sigmoid(X @ self.W.T + self.b[None, :])

    def select(self, g: int) -> "_TorchLogreg":
        return _TorchLogreg(self.W[g], self.b[g])


class _TorchLogreg:
    def __init__(self, w: torch.Tensor, b: torch.Tensor):
        self.w = w
        self.b = b

    def proba(self, X: torch.Tensor) -> torch.Tensor:
        return torch.sigmoid(X @ self.w + self.b)


class LogisticFeasibilityModel:
    def __init__(self, X, C, device=None, n_components: Optional[int] = None, seed=None):
        X = np.asarray(X, dtype=np.float64)
        C = np.asarray(C, dtype=np.float64)
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.dtype = torch.float64 if self.device.type == "cpu" else torch.float32
        Xt = torch.as_tensor(X, dtype=self.dtype, device=self.device)
        # standardize then PCA basis via SVD
        self.mu = Xt.mean(dim=0)
        self.sigma = Xt.std(dim=0, unbiased=False).clamp_min(1e-12)
        Xs = (Xt - self.mu) / self.sigma
        q = min(Xt.shape) if n_components is None else n_components
        U, S, Vh = torch.linalg.svd(Xs, full_matrices=False)
        self.components = Vh[:q]  # (q, d)
        Z = Xs @ self.components.T
        self.X = X
        self.n_constraints = C.shape[1]
        self.clfs = []
        rng = np.random.default_rng(seed)
        for i in range(self.n_constraints):
            c_i = torch.as_tensor(
                (C[:, i] > 0.0).astype(np.float64), dtype=self.dtype, device=self.device
            )
            if len(torch.unique(c_i)) > 1:
                clf = self._fit_with_grid(Z, c_i, rng)
            else:
                clf = None
            self.clfs.append(clf)

    def _fit_with_grid(self, Z, c, rng):
        n = Z.shape[0]
        if n >= 20:
            idx = rng.permutation(n)
            n_val = max(1, n // 5)
            val, tr = idx[:n_val], idx[n_val:]
            l1s = 1.0 / np.logspace(-4, 4, 4)
            batch = _TorchLogregBatch(Z[tr], c[tr], l1s)
            p = batch.proba_all(Z[val]).clamp(1e-7, 1 - 1e-7)  # (n_val, G)
            losses = torch.nn.functional.binary_cross_entropy(
                p, c[val][:, None].expand_as(p), reduction="none"
            ).mean(dim=0)
            return batch.select(int(losses.argmin()))
        batch = _TorchLogregBatch(Z, c, [1.0])
        return batch.select(0)

    # ------------------------------------------------------------- interface
    def _transform(self, x) -> torch.Tensor:
        xt = torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=self.dtype, device=self.device)
        if xt.ndim == 1:
            xt = xt[None, :]
        return ((xt - self.mu) / self.sigma) @ self.components.T

    def predict(self, x):
        Z = self._transform(x)
        ps = []
        for clf in self.clfs:
            if clf is not None:
                ps.append((clf.proba(Z) > 0.5).to(torch.int64).cpu().numpy())
            else:
                ps.append(np.ones(Z.shape[0], dtype=np.int64))
        return np.column_stack(ps)

    def predict_proba(self, x):
        Z = self._transform(x)
        probs = []
        for clf in self.clfs:
            if clf is not None:
                p1 = clf.proba(Z).cpu().numpy()
                probs.append(np.stack([1.0 - p1, p1], axis=1))
            else:
                probs.append(np.tile([0.0, 1.0], (Z.shape[0], 1)))
        return np.stack(probs)

    def rank(self, x):
        pr = self.predict_proba(x)
        return np.mean(pr[:, :, 1], axis=0)


class GPFeasibilityModel:
    """Registry name 'gp' — probability of feasibility from a GP regressed
    on the constraint values (Schonlau 1998; Gardner et al. 2014).

    One ``GPRMatern`` with one output per modelled constraint column is
    fitted on all rows of (X, C). With its standardised posterior mean mu_n
    and noise-inclusive variance var_n at a query,

        z_b   = (mu_n + y_mean_b / y_std_b) / sqrt(max(var_n, 1e-12))
        PoF_b = P(c_b(x) > 0) = 0.5 erfc(-z_b / sqrt 2)
        rank  = (1/C) sum_b PoF_b   over ALL C columns, in column order.

    A column with zero variance in the archive is not given to the GP: its
    PoF is the constant 1.0 where its value is > 0, else 0.0. A column whose
    sign never changes but whose values vary IS modelled. With no modelled
    column no GP is fitted (``gp`` and ``theta`` are None).

    ``seed`` defaults to 0, not None: the engine passes no seed to
    feasibility models and every rank fits its own copy, so an unseeded
    search would let the ranks diverge. Bounds default to the per-column
    min / max of X (queries outside are fine, the map is affine). Other
    keyword arguments go to ``GPRMatern``; ``return_mean_variance``,
    ``thompson`` and ``compute="bf16"`` are not offered.

    ``predict`` / ``predict_proba`` / ``rank`` take and return numpy, as
    LogisticFeasibilityModel does; ``pof_tensor`` / ``rank_tensor`` take a raw
    device tensor and return a device tensor of its dtype with no host trip.
    A float32 GPU model answers all five from the fused kernel of
    ops/hip/gp_pof.hip, everything else from torch_ref.gp_predict_pof_ref.
    """

    def __init__(self, X, C, device=None, seed=0, xlb=None, xub=None,
                 anisotropic=False, optimizer="sceua", **gp_kwargs):
        for key in ("return_mean_variance", "thompson"):
            if key in gp_kwargs:
                raise ValueError(f"GPFeasibilityModel does not offer {key}")
        if gp_kwargs.get("compute", "fp32") != "fp32":
            raise ValueError('GPFeasibilityModel does not offer compute="bf16"')
        from dmosopt_amd.models.gp import GPRMatern

        X = np.asarray(X, dtype=np.float64)
        C = np.asarray(C, dtype=np.float64)
        if C.ndim == 1:
            C = C.reshape(-1, 1)
        self.n_constraints = C.shape[1]
        # constant columns: PoF is their sign, the GP never sees them
        const = np.zeros(self.n_constraints)
        modelled = []
        for j in range(self.n_constraints):
            col = C[np.isfinite(C[:, j]), j]
            if col.size and col.max() > col.min():
                modelled.append(j)
            else:
                const[j] = 1.0 if col.size and col[0] > 0.0 else 0.0
        self.modelled = np.asarray(modelled, dtype=np.int64)
        self.constant = np.setdiff1d(np.arange(self.n_constraints), self.modelled)
        self._const_vals = const[self.constant]
        self.gp = None
        self.theta = None
        if len(modelled):
            xlb = X.min(axis=0) if xlb is None else np.asarray(xlb, dtype=np.float64)
            xub = X.max(axis=0) if xub is None else np.asarray(xub, dtype=np.float64)
            Cm = C[:, self.modelled]
            # nan="remove" drops the rows the GP cannot use
            Cm = np.where(np.isfinite(Cm), Cm, np.nan)
            self.gp = GPRMatern(
                X, Cm, X.shape[1], len(modelled), xlb, xub, optimizer=optimizer,
                seed=seed, anisotropic=anisotropic, device=device, **gp_kwargs,
            )
            self.theta = self.gp.theta
            self.device, self.dtype = self.gp.device, self.gp.dtype
        else:
            self.device = torch.device(device) if device is not None else (
                torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
            )
            self.dtype = gp_kwargs.get("dtype") or (
                torch.float64 if self.device.type == "cpu" else torch.float32)
        self._const_cache = None

    # ---------------------------------------------------------------- device
    def _gp_block(self, xr: torch.Tensor) -> torch.Tensor:
        """(P, B + 1) block [PoF of the modelled columns | their mean]."""
        from dmosopt_amd import ops
        from dmosopt_amd.models.gp_core import _single_threaded_cpu_math

        gp, f = self.gp, self.gp._fitted
        if xr.is_cuda and ops.native_fp32(f.X):
            cache, pa = gp._native_pred_cache(xr.device)
            linv = getattr(f, "_pred_linv", None)
            if linv is None:
                linv = f._pred_linv = f.Linv.contiguous().float()
            return ops.gp_predict_pof_cached(
                xr.contiguous(), pa, linv, cache[1], cache[2])
        # on the CPU the variance takes FittedGP.predict's triangular solve
        # (no explicit inverse), on a GPU the kernel's Linv form
        with _single_threaded_cpu_math(not xr.is_cuda):
            return ops.torch_ref.gp_predict_pof_ref(
                gp.normalize_query(xr), f.X, f.theta, f.alpha,
                f.Linv if xr.is_cuda else None, f.y_mean, f.y_std, f.nu,
                f.anisotropic, L=None if xr.is_cuda else f.L,
            )

    def _block(self, x: torch.Tensor):
        """PoF (P, C) and rank (P,) on the model's device, in its dtype."""
        from dmosopt_amd import ops

        xr = x.to(self.device, self.dtype)
        if xr.ndim == 1:
            xr = xr[None, :]
        B = len(self.modelled)
        if xr.shape[0] == 0:  # the native call takes P >= 1
            return (xr.new_empty(0, self.n_constraints), xr.new_empty(0))
        if B == self.n_constraints:  # the kernel's block is the answer
            blk = self._gp_block(xr)
            return blk[:, :B], blk[:, B]
        if self._const_cache is None:
            self._const_cache = (
                torch.as_tensor(self.modelled, device=self.device),
                torch.as_tensor(self.constant, device=self.device),
                torch.as_tensor(self._const_vals, dtype=self.dtype, device=self.device),
            )
        mod, con, vals = self._const_cache
        pof = torch.empty(xr.shape[0], self.n_constraints, dtype=self.dtype,
                          device=self.device)
        pof[:, con] = vals
        if B:
            pof[:, mod] = self._gp_block(xr)[:, :B]
        return pof, ops.torch_ref.mean_in_column_order(pof)

    def pof_tensor(self, x: torch.Tensor) -> torch.Tensor:
        """Raw device tensor x (P, d) -> PoF (P, C) on x's device, in x's
        dtype; no host trip where x is on the model's device."""
        return self._block(x)[0].to(device=x.device, dtype=x.dtype)

    def rank_tensor(self, x: torch.Tensor) -> torch.Tensor:
        """Raw device tensor x (P, d) -> rank (P,) on x's device, in x's
        dtype; no host trip where x is on the model's device."""
        return self._block(x)[1].to(device=x.device, dtype=x.dtype)

    # ------------------------------------------------------------- interface
    def _pof_numpy(self, x):
        pof, rank = self._block(torch.as_tensor(np.asarray(x, dtype=np.float64)))
        both = torch.cat([pof, rank[:, None]], dim=1).cpu().numpy().astype(np.float64)
        return both[:, :-1], both[:, -1]

    def predict(self, x):
        return (self._pof_numpy(x)[0] > 0.5).astype(np.int64)

    def predict_proba(self, x):
        p1 = self._pof_numpy(x)[0].T  # (C, P)
        return np.stack([1.0 - p1, p1], axis=2)

    def rank(self, x):
        return self._pof_numpy(x)[1]
