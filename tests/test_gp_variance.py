"""Fused on-device posterior variance (ops/hip/gp_variance.hip) and the
device-resident mean-variance mode built on it.

The variance is y_std^2 * max(sf2 + noise - |Linv k*|^2, 0). The oracle is
float64 on the CPU from the SAME float32-representable points and theta:
direct-difference kernel, torch.linalg.cholesky, triangular solve,
kss - |v|^2. Variances are compared in standardised units (divided by
y_std^2) against VAR_ATOL.

VAR_ATOL = 5e-5: about 8x the worst error of an fp32 emulation of the
whole pipeline (6.4e-6, profiles/README.md), which leaves room for __expf
and the MFMA accumulation order. The K^-1 form this replaces misses it by
1-3 orders of magnitude on the SEPARATING cases below.
"""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VAR_ATOL = 5e-5
JITTER = 1e-6
Y_STD = (2.5, 0.4, 1.7)
Y_MEAN = (0.3, -1.2, 4.0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dmosopt_amd import ops

    assert ops.native_available(), "native extension must be built on a GPU box"
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ helpers
def _theta(B, D, aniso, ell, noise, sf2, g):
    """(B, p) float32 log-hyperparameters; objective b scales ell by
    (1 + 0.15 b), anisotropic adds per-dimension factors in [0.7, 1.4]."""
    cols = [torch.full((B, 1), math.log(sf2))]
    scale = 1.0 + 0.15 * torch.arange(B, dtype=torch.float64)[:, None]
    if aniso:
        f = 0.7 + 0.7 * torch.rand(B, D, generator=g, dtype=torch.float64)
        cols.append(torch.log(ell * scale * f))
    else:
        cols.append(torch.log(ell * scale))
    cols.append(torch.full((B, 1), math.log(noise)))
    return torch.cat([c.double() for c in cols], dim=1).float()


def _problem(N, D, B, P, aniso=False, ell=0.5, noise=1e-3, sf2=1.0, seed=0,
             n_on_train=0):
    """Float32 CPU tensors: train X (N,D), Y (N,B) raw targets, theta,
    queries Xq (P,D) of which the first n_on_train sit on training rows and
    the next n_on_train right beside one."""
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(N, D, generator=g).float()
    w = torch.rand(D, B, generator=g).float()
    Yn = torch.sin(3.0 * (X @ w) / math.sqrt(D)) + 0.3 * torch.cos(X.sum(1, keepdim=True))
    y_mean = torch.tensor(Y_MEAN[:B])
    y_std = torch.tensor(Y_STD[:B])
    Y = y_mean[None, :] + y_std[None, :] * Yn
    Xq = torch.rand(P, D, generator=g).float()
    k = min(n_on_train, P, N)
    if k:
        rows = X[torch.arange(k) * (N // k)]
        Xq[:k] = rows
        # ... and as many 2e-4 beside one: r ~ 2e-4/ell is where a d2 formed
        # by cancellation (abs error ~1e-7) is all error, which a kernel
        # with a kink at r = 0 (nu = 1/2) passes on to the variance
        k2 = min(k, P - k)
        Xq[k:k + k2] = rows[:k2]
        Xq[k:k + k2, 0] += 2e-4
    theta = _theta(B, D, aniso, ell, noise, sf2, g)
    return X, Y, theta, y_mean, y_std, Xq


def _matern64(d2, nu):
    if nu == float("inf"):
        return torch.exp(-0.5 * d2)
    r = torch.sqrt(d2)
    if nu == 0.5:
        return torch.exp(-r)
    if nu == 1.5:
        s = math.sqrt(3.0) * r
        return (1.0 + s) * torch.exp(-s)
    s = math.sqrt(5.0) * r
    return (1.0 + s + (5.0 / 3.0) * d2) * torch.exp(-s)


def _oracle(X, Y, theta, y_mean, y_std, Xq, nu, aniso):
    """float64 posterior (mean (P,B), var (P,B)); var UNclamped, raw units."""
    X, Y, theta, Xq = X.double(), Y.double(), theta.double(), Xq.double()
    y_mean, y_std = y_mean.double(), y_std.double()
    N, D = X.shape
    means, vars_ = [], []
    for b in range(theta.shape[0]):
        sf2, noise = torch.exp(theta[b, 0]), torch.exp(theta[b, -1])
        ell = torch.exp(theta[b, 1:1 + D]) if aniso else torch.exp(theta[b, 1])
        xs, qs = X / ell, Xq / ell
        d2 = ((xs[:, None, :] - xs[None, :, :]) ** 2).sum(-1)
        K = sf2 * _matern64(d2, nu) + (noise + JITTER) * torch.eye(N, dtype=torch.float64)
        d2s = ((qs[:, None, :] - xs[None, :, :]) ** 2).sum(-1)
        Ks = sf2 * _matern64(d2s, nu)  # (P, N)
        L = torch.linalg.cholesky(K)
        yn = (Y[:, b] - y_mean[b]) / y_std[b]
        alpha = torch.cholesky_solve(yn[:, None], L)[:, 0]
        v = torch.linalg.solve_triangular(L, Ks.T, upper=False)  # (N, P)
        means.append(y_mean[b] + y_std[b] * (Ks @ alpha))
        vars_.append(y_std[b] ** 2 * (sf2 + noise - (v * v).sum(0)))
    return torch.stack(means, 1), torch.stack(vars_, 1)


def _fit(dev, X, Y, theta, y_mean, y_std, nu, aniso):
    from dmosopt_amd.models.gp_core import FittedGP

    return FittedGP(
        X.to(dev), Y.to(dev), theta.to(dev), y_mean.to(dev), y_std.to(dev),
        nu=nu, anisotropic=aniso, jitter=JITTER,
    )


def _check_var(var, want_var, y_std, label):
    err = ((var.double().cpu() - want_var) / y_std.double() ** 2).abs().max().item()
    print(f"{label}: max standardised variance error {err:.3e}")
    assert err <= VAR_ATOL, f"{label}: variance error {err:.3e} > {VAR_ATOL}"
    return err


# --------------------------------------------- 1. shapes the tiling can miss
# (N, P, B, D, nu, aniso): N at the 16/32 tile edges, one past, ragged last
# tile, workload size; P single / one past a tile / three ragged tiles;
# D = 1 and 30 are no multiple of the MFMA k = 4.
SHAPE_CASES = [
    (1, 1, 1, 1, 2.5, False),
    (1, 33, 3, 6, 1.5, True),
    (31, 70, 1, 6, 0.5, False),
    (32, 33, 3, 30, 2.5, True),
    (33, 1, 3, 1, float("inf"), False),
    (33, 70, 1, 6, 1.5, False),
    (97, 33, 3, 6, 2.5, True),
    (97, 70, 1, 30, float("inf"), True),
    (97, 1, 3, 1, 0.5, True),
    (300, 70, 3, 6, 2.5, False),
    (300, 33, 1, 30, 1.5, True),
    (300, 70, 3, 6, float("inf"), False),
    (300, 1, 1, 6, 0.5, True),
]


@pytest.mark.parametrize("N,P,B,D,nu,aniso", SHAPE_CASES)
def test_predict_var_shapes_match_oracle(dev, N, P, B, D, nu, aniso):
    prob = _problem(N, D, B, P, aniso=aniso, ell=0.4 * math.sqrt(D),
                    noise=1e-3, seed=100 + N + P, n_on_train=3)
    X, Y, theta, y_mean, y_std, Xq = prob
    fit = _fit(dev, X, Y, theta, y_mean, y_std, nu, aniso)
    mean, var = fit.predict(Xq.to(dev), return_var=True)
    assert mean.shape == (P, B) and var.shape == (P, B)
    want_mean, want_var = _oracle(X, Y, theta, y_mean, y_std, Xq, nu, aniso)
    assert np.allclose(mean.cpu().numpy(), want_mean.numpy(), rtol=1e-3, atol=1e-3)
    _check_var(var, want_var, y_std, f"N={N} P={P} B={B} D={D} nu={nu} aniso={aniso}")


# ------------------------------ 2. the cases that separate the two formulas
SEPARATING = [(1.0, 1e-6), (3.0, 1e-6), (1.0, 1e-9)]


@pytest.mark.parametrize("ell,noise", SEPARATING)
def test_predict_var_smooth_fit_accuracy(dev, ell, noise):
    """N=300, d=6 smooth fits, 5 of 70 queries on training rows. The fp32
    K^-1 form this replaced measured 6.9e-4 .. 1.5e-1 here in CPU
    emulation; GPU figures of both forms are in profiles/README.md."""
    B = 2
    X, Y, theta, y_mean, y_std, Xq = _problem(
        300, 6, B, 70, ell=ell, noise=noise, sf2=1.0, seed=7, n_on_train=5)
    theta[:, 1] = math.log(ell)  # both objectives at the stated ell
    fit = _fit(dev, X, Y, theta, y_mean, y_std, 2.5, False)
    _, var = fit.predict(Xq.to(dev), return_var=True)
    _, want_var = _oracle(X, Y, theta, y_mean, y_std, Xq, 2.5, False)
    _check_var(var, want_var, y_std, f"ell={ell} noise={noise}")


# ------------------------------------------------------------ 4. invariants
@pytest.fixture(scope="module")
def inv(dev):
    """One N=97 (ragged last tile), B=3 fit and its 70-query full call."""
    from dmosopt_amd import ops

    X, Y, theta, y_mean, y_std, Xq = _problem(
        97, 6, 3, 70, ell=0.8, noise=1e-4, seed=21, n_on_train=5)
    fit = _fit(dev, X, Y, theta, y_mean, y_std, 2.5, False)

    def call(xq, **kw):
        return ops.gp_predict_mean_var_fused(
            xq, fit.X, fit.theta, fit.alpha, fit.Linv, fit.y_mean, fit.y_std,
            fit.nu, fit.anisotropic, **kw)

    xq = Xq.to(dev)
    return dict(fit=fit, call=call, xq=xq, full=call(xq), theta=theta, y_std=y_std)


def test_var_bounds(inv):
    B = 3
    var = inv["full"][:, B:].cpu()
    sf2 = torch.exp(inv["theta"][:, 0].double())
    noise = torch.exp(inv["theta"][:, -1].double())
    hi = (inv["y_std"].double() ** 2 * (sf2 + noise)).float()
    assert bool((var >= 0).all())
    # the prior variance bounds it (1e-6 relative: the bound itself is
    # formed in float32 on the device, a handful of roundings)
    assert bool((var <= hi[None, :] * (1 + 1e-6)).all())
    assert bool((var[:5] < 1e-2 * hi[None, :]).all()), "on-train variance ~ noise"


def test_var_repeat_bitwise(inv):
    assert torch.equal(inv["call"](inv["xq"]), inv["full"])


def test_var_slice_bitwise(inv):
    """Rows [5:38] of the 70-query call == a 33-query call on that slice:
    a query's result does not depend on P or on its place in a tile."""
    part = inv["call"](inv["xq"][5:38].contiguous())
    assert torch.equal(part, inv["full"][5:38])


def test_var_strided_shards_bitwise(inv):
    """The rank-sharded predict ([r::2] shards, interleaved) reproduces the
    full-batch predict exactly."""
    xq, full = inv["xq"], inv["full"]
    out = torch.empty_like(full)
    out[0::2] = inv["call"](xq[0::2].contiguous())
    out[1::2] = inv["call"](xq[1::2].contiguous())
    assert torch.equal(out, full)


def test_var_decimals_rounding(inv):
    B = 3
    got = inv["call"](inv["xq"], var_decimals=6).cpu()
    raw = inv["full"].cpu()
    assert torch.equal(got[:, :B], raw[:, :B])
    want = torch.round(raw[:, B:] * 1e6) / 1e6  # float32, half-to-even = rintf
    assert torch.equal(got[:, B:], want)


def test_predict_mean_keeps_bmm_bits(inv):
    """predict(return_var=True) takes only the variance from the fused
    block: evaluate() of a mean-only model comes through it (the inner
    loop's initial population), so its mean stays the cross kernel + bmm
    chain bit for bit — the gemv's summation order would move every later
    generation."""
    from dmosopt_amd.models.gp_core import build_kernel

    f, xq = inv["fit"], inv["xq"]
    mean, var = f.predict(xq, return_var=True)
    Ks = build_kernel(xq, f.X, f.theta, nu=f.nu, anisotropic=f.anisotropic)
    want = f.y_mean[None, :] + f.y_std[None, :] * torch.bmm(Ks, f.alpha)[:, :, 0].T
    assert torch.equal(mean, want)
    assert torch.equal(var, inv["full"][:, 3:])


def test_mean_columns_equal_evaluate_tensor(dev):
    """Raw (un-normalised) queries through the in-kernel affine: the mean
    half of the mean-variance block is bitwise the mean-only evaluate."""
    from dmosopt_amd.models.gp import GPRMatern

    X, Y, theta, _, _, Xq = _problem(97, 6, 3, 70, ell=0.8, noise=1e-4, seed=22)
    lb, ub = -np.ones(6), 2.0 * np.ones(6)
    xin = (lb + (ub - lb) * X.double().numpy())
    xq = torch.as_tensor(lb + (ub - lb) * Xq.double().numpy(), dtype=torch.float32,
                         device=dev)
    kw = dict(theta_override=theta.numpy(), device=dev)
    gp_mv = GPRMatern(xin, Y.numpy(), 6, 3, lb, ub, return_mean_variance=True, **kw)
    gp_m = GPRMatern(xin, Y.numpy(), 6, 3, lb, ub, **kw)
    assert gp_mv.supports_device_mean_variance
    mv = gp_mv.evaluate_mean_variance_tensor(xq)
    assert mv.is_cuda and mv.shape == (70, 6) and mv.dtype == torch.float32
    assert torch.equal(mv[:, :3], gp_m.evaluate_tensor(xq))
    # [mean | round(var, 6)]: the variance half is the rounded fused value
    f = gp_mv._fitted
    from dmosopt_amd import ops

    raw = ops.gp_predict_mean_var_fused(
        xq, f.X, f.theta, f.alpha, f.Linv, f.y_mean, f.y_std, f.nu,
        f.anisotropic, gp_mv._affine_cache[1], gp_mv._affine_cache[2])
    assert torch.equal(mv[:, 3:].cpu(), torch.round(raw[:, 3:].cpu() * 1e6) / 1e6)


def test_sharded_objective_mean_variance(dev):
    """ShardedObjective at world 1 passes the block through and delegates
    the capability attribute."""
    from dmosopt_amd.models.gp import GPRMatern
    from dmosopt_amd.parallel.sharded import ShardedObjective

    class _Ctx:
        rank, world = 0, 1

        def all_gather_interleaved(self, t, P):
            return t[:P]

    X, Y, theta, _, _, Xq = _problem(33, 4, 2, 7, ell=0.8, noise=1e-4, seed=23)
    gp = GPRMatern(X.double().numpy(), Y.numpy(), 4, 2, np.zeros(4), np.ones(4),
                   return_mean_variance=True, theta_override=theta.numpy(), device=dev)
    sh = ShardedObjective(gp, _Ctx())
    assert sh.supports_device_mean_variance
    xq = Xq.to(dev)
    assert torch.equal(sh.evaluate_mean_variance_tensor(xq),
                       gp.evaluate_mean_variance_tensor(xq))


# ----------------------------------------------------------- 5. engine path
def test_engine_surrogate_eval_device_resident(dev):
    from dmosopt_amd.benchmarks.problems import zdt1
    from dmosopt_amd.core.engine import _surrogate_eval
    from dmosopt_amd.models.gp import GPRMatern
    from dmosopt_amd.models.model import Model

    rng = np.random.default_rng(3)
    X = rng.random((60, 6))
    Y = zdt1(X).numpy()
    gp = GPRMatern(X, Y, 6, 2, np.zeros(6), np.ones(6), optimizer="sceua",
                   seed=11, return_mean_variance=True, device=dev)
    mdl = Model(return_mean_variance=True, objective=gp)
    xq = torch.as_tensor(rng.random((33, 6)), dtype=torch.float32, device=dev)
    got = _surrogate_eval(mdl, xq, True)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    assert got.shape == (33, 4)
    got = got.cpu().numpy().astype(np.float64)
    want_mean, want_var = gp.evaluate(xq.cpu().numpy())  # host path
    assert np.allclose(got[:, :2], want_mean, rtol=1e-3, atol=1e-3)
    y_std2 = gp._fitted.y_std.double().cpu().numpy() ** 2
    err = np.abs(got[:, 2:] - want_var)
    assert (err <= VAR_ATOL * y_std2[None, :] + 1e-6).all(), err.max()


# ----------------------------------------------------------- 6. end to end
def test_mean_variance_run_end_to_end(dev):
    import dmosopt_amd

    def obj_fun(pp):
        x = np.array([pp[f"x{i}"] for i in range(4)])
        return np.array([np.sum(x**2), np.sum((x - 1) ** 2)])

    def run(opt_id):
        params = {
            "opt_id": opt_id,
            "obj_fun": obj_fun,
            "problem_parameters": {},
            "space": {f"x{i}": [0.0, 1.0] for i in range(4)},
            "objective_names": ["f1", "f2"],
            "population_size": 20,
            "num_generations": 6,
            "optimizer": "nsga2",
            "n_initial": 2,
            "n_epochs": 2,
            "random_seed": 7,
            "optimize_mean_variance": True,
            "surrogate_method_kwargs": {"anisotropic": False, "optimizer": "sceua"},
            "device": dev,
        }
        bestx, besty = dmosopt_amd.run(params, verbose=False)
        x = np.column_stack([v for _, v in bestx])
        y = np.column_stack([v for _, v in besty])
        return x, y

    x1, y1 = run("t_mv_gpu_a")
    assert y1.shape[1] == 2 and np.isfinite(y1).all()
    x2, y2 = run("t_mv_gpu_b")
    assert x1.tobytes() == x2.tobytes() and y1.tobytes() == y2.tobytes()
