"""Fused GP probability of feasibility (ops/hip/gp_pof.hip) and the
device-resident feasibility rank of the optimizers built on it.

PoF_b = 0.5 erfc(-z_b / sqrt 2), z_b = (mu_n + y_mean_b / y_std_b) /
sqrt(max(var_n, 1e-12)) with the standardised posterior mean mu_n and the
noise-inclusive variance var_n = max(sf2 + noise - |Linv k*|^2, 0); column C
of the (P, C + 1) block is the mean of the PoF columns in column order.

The oracle is the closed form in float64 on the CPU from the SAME float32
inputs: direct-difference kernel, torch.linalg.cholesky, triangular solves.

POF_TOL = 8 x the worst absolute error of an fp32 emulation of the closed
form (``gp_predict_pof_ref`` in float32 on the CPU, Cholesky and L^-1 in
float32 too; ``emulate_fp32`` below) against that oracle on these very
inputs, the margin VAR_ATOL, GRAD_TOL and JAC_TOL got:
  emulated: worst 1.52e-4 (N=65, D=30, nu=1/2, ARD), 5.6e-5 (N=300, D=2,
            RBF), 1.9e-5 (N=33, D=1), every other case <= 1.3e-6
            ->  POF_TOL = 1.2e-3
POF_FLOOR = 2.0 ** -20
  MI355X:   worst 3.85e-5 (N=300, D=2, RBF), 1.6e-5 (N=33, D=1), every other
            case <= 1.2e-6
One case sets that worst: the emulation's float32 norms-form distances at
D = 30, which the kernel's cross kernel does not share (1.5e-7 there). So
the oracle test holds every case to 8 x ITS OWN emulated error (the figure in
ORACLE_CASES), never less than POF_FLOOR = 8 float32 ulps of 1 (2^-20: PoF is
a float32 in [0, 1], and erfcf is good to a few ulps) and never more than
POF_TOL. No case is looser than the rule above, most are 10 .. 1000 times
tighter.
"""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POF_TOL = 1.2e-3
POF_FLOOR = 2.0 ** -20
JITTER = 1e-6
SF2, NOISE = 1.1, 1e-2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dmosopt_amd import ops

    assert ops.native_available(), "native extension must be built on a GPU box"
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ helpers
def _problem(N, D, C, P, aniso):
    """Float32 CPU tensors of the kernel-level tests: X (N, D) and Xq (P, D)
    uniform, theta (C, p) with ell = 0.5 (0.7 + 0.7 U) per constraint (per
    dimension too if ARD), sf2 = 1.1, noise = 1e-2, and raw targets
    sin(3 X w / sqrt D) + 0.3 cos(sum X) minus the column median, so every
    constraint crosses zero."""
    g = torch.Generator().manual_seed(1000 + N + D)
    X = torch.rand(N, D, generator=g).float()
    Xq = torch.rand(P, D, generator=g).float()
    w = torch.rand(D, C, generator=g).float()
    u = torch.rand(C, D if aniso else 1, generator=g, dtype=torch.float64)
    theta = torch.cat([
        torch.full((C, 1), math.log(SF2), dtype=torch.float64),
        torch.log(0.5 * (0.7 + 0.7 * u)),
        torch.full((C, 1), math.log(NOISE), dtype=torch.float64),
    ], dim=1).float()
    Y = torch.sin(3.0 * (X @ w) / math.sqrt(D)) + 0.3 * torch.cos(X.sum(1, keepdim=True))
    Y = Y - Y.median(dim=0).values[None, :]
    y_mean = Y.mean(dim=0)
    y_std = Y.std(dim=0, unbiased=False) if N > 1 else torch.ones(C)
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


def _pof64(mean_over_sd):
    return 0.5 * torch.special.erfc(-mean_over_sd.double() * math.sqrt(0.5))


def _oracle(X, Y, theta, y_mean, y_std, Xq, nu, aniso):
    """float64 PoF (P, C)."""
    X, Y, theta, Xq = X.double(), Y.double(), theta.double(), Xq.double()
    y_mean, y_std = y_mean.double(), y_std.double()
    N, D = X.shape
    cols = []
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
        var_n = (sf2 + noise - (v * v).sum(0)).clamp_min(0.0)
        z = (Ks @ alpha + y_mean[b] / y_std[b]) / torch.sqrt(var_n.clamp_min(1e-12))
        cols.append(_pof64(z))
    return torch.stack(cols, 1)


def _fit(device, X, Y, theta, y_mean, y_std, nu, aniso):
    from dmosopt_amd.models.gp_core import FittedGP

    return FittedGP(
        X.to(device), Y.to(device), theta.to(device), y_mean.to(device),
        y_std.to(device), nu=nu, anisotropic=aniso, jitter=JITTER,
    )


def _pof(fit, xq, q_lb=None, q_invrg=None):
    from dmosopt_amd import ops

    return ops.gp_predict_pof(
        xq, fit.X, fit.theta, fit.alpha, fit.Linv, fit.y_mean, fit.y_std, fit.nu,
        fit.anisotropic, q_lb, q_invrg)


def emulate_fp32(N, D, C, P, nu, aniso):
    """(worst |ref32 - oracle|, share of oracle PoF in (0.01, 0.99)) of one
    case: gp_predict_pof_ref on a float32 CPU fit. Not a test: the figures in
    the module docstring come from it."""
    from dmosopt_amd.ops import torch_ref

    prob = _problem(N, D, C, P, aniso)
    X, Y, theta, y_mean, y_std, Xq = prob
    want = _oracle(*prob, nu, aniso)
    f = _fit("cpu", X, Y, theta, y_mean, y_std, nu, aniso)
    got = torch_ref.gp_predict_pof_ref(
        Xq, f.X, f.theta, f.alpha, f.Linv, f.y_mean, f.y_std, nu, aniso)
    share = ((want > 0.01) & (want < 0.99)).double().mean().item()
    return (got[:, :C].double() - want).abs().max().item(), share


# ------------------------------------------------ 1. against the float64 oracle
# (N, D, C, P, nu, aniso): one short of a 32-row tile, exactly one, one past
# it, a ragged third tile, the D ceiling of the gradient kernels, and the
# workload's shape; last the case's emulated fp32 error (emulate_fp32)
ORACLE_CASES = [
    (1, 1, 1, 1, 2.5, False, 0.0),
    (2, 3, 2, 31, 0.5, True, 2.05e-7),
    (31, 6, 3, 33, 1.5, False, 1.26e-6),
    (33, 1, 1, 200, 2.5, True, 1.88e-5),
    (65, 30, 6, 200, 0.5, True, 1.52e-4),
    (97, 128, 2, 64, 2.5, True, 4.44e-8),
    (300, 30, 2, 200, 2.5, False, 5.40e-7),
    (300, 2, 2, 200, float("inf"), False, 5.64e-5),
]


@pytest.mark.parametrize("N,D,C,P,nu,aniso,emulated", ORACLE_CASES)
def test_pof_matches_float64_oracle(dev, N, D, C, P, nu, aniso, emulated):
    tol = min(max(8.0 * emulated, POF_FLOOR), POF_TOL)
    prob = _problem(N, D, C, P, aniso)
    X, Y, theta, y_mean, y_std, Xq = prob
    want = _oracle(*prob, nu, aniso)
    if N > 1:
        # a test on saturated probabilities proves nothing
        share = ((want > 0.01) & (want < 0.99)).double().mean().item()
        assert share >= 0.15, f"only {share:.2f} of the oracle's PoF unsaturated"
    fit = _fit(dev, X, Y, theta, y_mean, y_std, nu, aniso)
    got = _pof(fit, Xq.to(dev))
    assert got.shape == (P, C + 1) and got.dtype == torch.float32 and got.is_cuda
    err = (got[:, :C].double().cpu() - want).abs().max().item()
    print(f"N={N} D={D} C={C} P={P} nu={nu} aniso={aniso}: max PoF error {err:.3e}")
    assert err <= tol, f"PoF error {err:.3e} > {tol:.3e}"
    rank_err = (got[:, C].double().cpu() - want.mean(1)).abs().max().item()
    assert rank_err <= tol


# ------------------------------------------------------------ the invariants
@pytest.fixture(scope="module")
def inv(dev):
    """One N=97 (ragged last tile), C=3 fit and its 70-query block."""
    X, Y, theta, y_mean, y_std, Xq = _problem(97, 6, 3, 70, False)
    fit = _fit(dev, X, Y, theta, y_mean, y_std, 2.5, False)
    xq = Xq.to(dev)
    return dict(fit=fit, xq=xq, full=_pof(fit, xq))


def test_pof_sees_the_mean_and_variance_of_mean_var(inv):
    """PoF recomputed in float64 from gp_predict_mean_var's float32 mean and
    unrounded variance: erfcf is good to a few ulp and |z phi(z)| <= 0.25
    bounds what the roundings of z (~1e-7 relative) can move, so 1e-6
    absolute means both calls saw the same mu and sigma^2."""
    from dmosopt_amd import ops

    f, C = inv["fit"], 3
    mv = ops.gp_predict_mean_var_fused(
        inv["xq"], f.X, f.theta, f.alpha, f.Linv, f.y_mean, f.y_std, f.nu,
        f.anisotropic).double().cpu()
    y_std = f.y_std.double().cpu()
    want = _pof64(mv[:, :C] / torch.sqrt(mv[:, C:].clamp_min(1e-12 * y_std[None, :] ** 2)))
    err = (inv["full"][:, :C].double().cpu() - want).abs().max().item()
    print(f"max |PoF - PoF(mean_var)| = {err:.3e}")
    assert err <= 1e-6


def test_rank_column_is_the_fixed_order_mean(inv):
    pof = inv["full"].cpu()
    s = pof[:, 0].clone()
    for b in range(1, 3):
        s = s + pof[:, b]
    assert torch.equal(pof[:, 3], s / torch.full_like(s, 3.0))


def test_pof_batch_invariant_and_repeatable(inv):
    fit, xq, full = inv["fit"], inv["xq"], inv["full"]
    assert torch.equal(_pof(fit, xq), full)
    assert torch.equal(_pof(fit, xq[40:41].contiguous()), full[40:41])
    seven = _pof(fit, xq[36:43].contiguous())  # row 40 at position 4
    assert torch.equal(seven, full[36:43])
    moved = torch.cat([xq[40:41], xq[:6]]).contiguous()  # row 40 at position 0
    assert torch.equal(_pof(fit, moved)[0], full[40])
    assert torch.equal(_pof(fit, xq[5:38].contiguous()), full[5:38])


@pytest.mark.parametrize("nu", [2.5, 0.5])
def test_pof_affine_in_the_load(dev, nu):
    """Raw queries with the per-dimension affine applied inside the kernel
    load against queries normalised beforehand with the kernel's own two
    float32 operations, (raw - lb) * invrg: the whole block is bitwise the
    same, as test_gp_variance.py and test_gp_path.py expect of their affine
    paths. nu = 1/2 is the one case where the binding assembles a second,
    direct-difference cross kernel for the variance, with the same affine."""
    X, Y, theta, y_mean, y_std, Xq = _problem(97, 6, 3, 70, False)
    fit = _fit(dev, X, Y, theta, y_mean, y_std, nu, False)
    xq = Xq.to(dev)
    lb = torch.linspace(-1.0, 0.5, 6, device=dev)
    rg = torch.linspace(1.5, 3.0, 6, device=dev)
    raw = (lb + rg * xq).contiguous()
    invrg = (1.0 / rg).contiguous()
    got = _pof(fit, raw, lb.contiguous(), invrg)
    want = _pof(fit, ((raw - lb) * invrg).contiguous())
    assert torch.equal(got, want)
    # and the affine is not a no-op: the raw queries alone answer differently
    assert not torch.equal(_pof(fit, raw), want)


# ------------------------------------------------------------- 6. the model
def _tnk_archive(n, seed):
    from dmosopt_amd.benchmarks import problems as bp

    rng = np.random.default_rng(seed)
    x = 1e-9 + (np.pi - 1e-9) * rng.random((n, 2))
    f, c = bp.tnk(x)
    return x, f.numpy(), c.numpy()


def test_model_device_entries(dev):
    import os
    import subprocess
    import sys
    import tempfile

    from dmosopt_amd.models.feasibility import GPFeasibilityModel

    x, _, c = _tnk_archive(33, 31)
    xq = _tnk_archive(45, 32)[0]
    model = GPFeasibilityModel(x, c, device=dev, seed=1)
    xt = torch.as_tensor(xq, dtype=torch.float32, device=dev)
    pof, rank = model.pof_tensor(xt), model.rank_tensor(xt)
    assert pof.is_cuda and rank.is_cuda
    assert pof.shape == (45, 2) and rank.shape == (45,)
    assert pof.dtype == torch.float32 and rank.dtype == torch.float32
    # the numpy methods go through the same kernel
    assert np.abs(model.rank(xq) - rank.double().cpu().numpy()).max() <= 1e-6
    assert np.abs(model.predict_proba(xq)[:, :, 1].T
                  - pof.double().cpu().numpy()).max() <= 1e-6
    # a CPU model under a GPU population answers on the population's device
    cpu_model = GPFeasibilityModel(x, c, device="cpu",
                                   theta_override=model.theta.cpu().numpy())
    r_cpu = cpu_model.rank_tensor(xt)
    assert r_cpu.is_cuda and r_cpu.dtype == torch.float32
    assert (r_cpu - rank).abs().max().item() <= POF_TOL
    # a constant column joins on the device
    cc = np.column_stack([c, np.full(len(c), -1.0)])
    m3 = GPFeasibilityModel(x, cc, device=dev, theta_override=model.theta.cpu().numpy())
    p3 = m3.pof_tensor(xt)
    assert torch.equal(p3[:, :2], pof) and bool((p3[:, 2] == 0).all())
    assert torch.equal(m3.rank_tensor(xt),
                       (pof[:, 0] + pof[:, 1] + p3[:, 2]) / torch.full_like(rank, 3.0))
    # the same fit answered by plain torch in a process with the torch path
    # forced (the switch is read at import)
    code = (
        "import sys, numpy as np, torch\n"
        "from dmosopt_amd.models.feasibility import GPFeasibilityModel\n"
        "d = np.load(sys.argv[1])\n"
        "m = GPFeasibilityModel(d['x'], d['c'], device='cuda', theta_override=d['theta'])\n"
        "xt = torch.as_tensor(d['xq'], dtype=torch.float32, device='cuda')\n"
        "np.save(sys.argv[2], m.pof_tensor(xt).cpu().numpy())\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npy")
        np.savez(src, x=x, c=c, xq=xq, theta=model.theta.cpu().numpy())
        env = dict(os.environ, DMOSOPT_AMD_FORCE_TORCH="1", PYTHONPATH=root)
        subprocess.run([sys.executable, "-c", code, src, dst], check=True, env=env,
                       cwd=root, timeout=300)
        forced = np.load(dst)
    err = np.abs(forced - pof.cpu().numpy()).max()
    print(f"forced-torch model vs kernel: {err:.3e}")
    assert err <= POF_TOL


# --------------------------------------------------------- 7. the optimizers
def _counting_model():
    from dmosopt_amd.models.feasibility import GPFeasibilityModel

    class Counting(GPFeasibilityModel):
        calls = {"rank": 0, "rank_tensor": 0}

        def rank(self, x):
            Counting.calls["rank"] += 1
            return super().rank(x)

        def rank_tensor(self, x):
            Counting.calls["rank_tensor"] += 1
            return super().rank_tensor(x)

    return Counting


def _epoch(dev, optimizer, feasibility):
    from dmosopt_amd.core import engine

    x, y, c = _tnk_archive(40, 33)
    lb, ub = np.full(2, 1e-9), np.full(2, np.pi)
    res = engine.run_epoch(
        5, ["x1", "x2"], ["f1", "f2"], lb, ub, 0.25, x, y, c, pop=64,
        optimizer_name=optimizer, feasibility_method_name=feasibility,
        surrogate_method_kwargs={"anisotropic": False, "optimizer": "sceua", "seed": 3},
        local_random=np.random.default_rng(4), device=dev,
    )
    xr = res["x_resample"]
    assert xr.shape[0] > 0 and np.isfinite(xr).all()
    assert (xr >= lb - 1e-6).all() and (xr <= ub + 1e-6).all()
    return res


@pytest.mark.parametrize("optimizer", ["nsga2", "age", "smpso", "cmaes", "trs"])
def test_optimizers_rank_on_the_device(dev, optimizer):
    Counting = _counting_model()
    res = _epoch(dev, optimizer, Counting)
    assert isinstance(res["optimizer"].model.feasibility, Counting)
    assert Counting.calls["rank"] == 0, "the numpy route ran during the generations"
    assert Counting.calls["rank_tensor"] > 0
    # logreg has no rank_tensor: today's host route, a smoke check only
    from dmosopt_amd.models.feasibility import LogisticFeasibilityModel

    res = _epoch(dev, optimizer, "logreg")
    assert isinstance(res["optimizer"].model.feasibility, LogisticFeasibilityModel)


# ------------------------------------------------------------ 8. end to end
def _tnk_obj(pp):
    from dmosopt_amd.benchmarks import problems as bp

    f, c = bp.tnk(np.array([[pp["x1"], pp["x2"]]]))
    return f.numpy()[0], c.numpy()[0]


def test_run_tnk_cmaes_gp_feasibility(dev, monkeypatch):
    import dmosopt_amd
    from dmosopt_amd.benchmarks import problems as bp
    from dmosopt_amd.models.feasibility import GPFeasibilityModel

    # the engine logs and skips a feasibility model that fails to build, and
    # the best set is filtered on the true constraints either way: record
    # what was built and what ranked the populations
    built, ranked = [], []
    init, rank_tensor = GPFeasibilityModel.__init__, GPFeasibilityModel.rank_tensor

    def counting_init(self, *a, **kw):
        init(self, *a, **kw)
        built.append(self)

    def counting_rank_tensor(self, x):
        ranked.append(x.shape[0])
        return rank_tensor(self, x)

    monkeypatch.setattr(GPFeasibilityModel, "__init__", counting_init)
    monkeypatch.setattr(GPFeasibilityModel, "rank_tensor", counting_rank_tensor)

    params = {
        "opt_id": "t_gp_feas_gpu",
        "obj_fun": _tnk_obj,
        "problem_parameters": {},
        "space": {"x1": [1e-9, float(np.pi)], "x2": [1e-9, float(np.pi)]},
        "objective_names": ["f1", "f2"],
        "constraint_names": ["c1", "c2"],
        "population_size": 32,
        "num_generations": 5,
        "optimizer": "cmaes",
        "feasibility_method_name": "gp",
        "n_initial": 10,
        "n_epochs": 2,
        "random_seed": 23,
        "device": dev,
    }
    bestx, _ = dmosopt_amd.run(params, verbose=False)
    assert len(built) == 2, "one model per epoch"
    assert all(m.gp is not None and m.gp._fitted.X.is_cuda for m in built)
    assert len(ranked) > 0, "the optimizer never asked for the device rank"
    x = np.column_stack([v for _, v in bestx])
    assert x.shape[0] > 0
    assert (bp.tnk(x)[1].numpy() > 0).all()
