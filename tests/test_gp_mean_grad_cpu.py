"""Input gradient of the GP posterior mean on the CPU: the closed form
(``torch_ref.gp_predict_mean_grad_ref``) against float64 autograd, the units
of ``GPRMatern.gradient``, the ``dgsm_grad`` sensitivity entry against the
finite-difference ``dgsm``, its fallback and registry wiring, and the
rank-sharded route on gloo.

Measured on the CPU (float64): closed form vs autograd worst 5.8e-15
(bound 1e-9); gradient() vs central differences 9.3e-10 (bound 1e-6);
dgsm_grad vs dgsm 1.2e-6 and 1.6e-8 for the two objectives (bound 1e-4).
"""

import logging
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")

# the box of the units tests: ranges 2, 3, 0.5, 10
XLB = np.array([-1.0, 0.0, 2.0, -5.0])
XUB = np.array([1.0, 3.0, 2.5, 5.0])
THETA = np.array([[0.1, math.log(0.6), math.log(1e-3)],
                  [0.0, math.log(0.9), math.log(1e-3)]])


def _box_model(**kw):
    """float64 CPU GPRMatern, N = 40, m = 2, on the box above with given
    hyperparameters (no search)."""
    from dmosopt_amd.models.gp import GPRMatern

    rng = np.random.default_rng(0)
    u = rng.random((40, 4))
    x = XLB + u * (XUB - XLB)
    y = np.column_stack([np.sin(3.0 * u[:, 0]) + u[:, 1] ** 2,
                         np.cos(2.0 * u[:, 2]) + 0.1 * u[:, 3]])
    kw.setdefault("device", "cpu")
    kw.setdefault("dtype", torch.float64)
    return GPRMatern(x, y, 4, 2, XLB, XUB, theta_override=THETA, **kw)


# ------------------------------------------- 1. closed form vs float64 autograd
def _problem64(N, P, D, B, aniso, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(N, D, generator=g, dtype=torch.float64)
    Xq = torch.rand(P, D, generator=g, dtype=torch.float64)
    n_ell = D if aniso else 1
    ell = 0.5 * (0.7 + 0.7 * torch.rand(B, n_ell, generator=g, dtype=torch.float64))
    theta = torch.cat([
        torch.full((B, 1), math.log(1.1), dtype=torch.float64), torch.log(ell),
        torch.full((B, 1), math.log(1e-3), dtype=torch.float64),
    ], dim=1)
    alpha = torch.randn(B, N, generator=g, dtype=torch.float64)
    y_mean = torch.randn(B, generator=g, dtype=torch.float64)
    y_std = 0.5 + torch.rand(B, generator=g, dtype=torch.float64)
    return Xq, X, theta, alpha, y_mean, y_std


@pytest.mark.parametrize("aniso", [False, True], ids=["iso", "ard"])
@pytest.mark.parametrize("nu", [0.5, 1.5, 2.5, INF])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (33, 5, 6, 3), (40, 17, 4, 2)],
                         ids=lambda s: "N%d-P%d-D%d-B%d" % s)
def test_closed_form_matches_float64_autograd(shape, nu, aniso):
    from dmosopt_amd.models.gp_core import build_kernel_torch
    from dmosopt_amd.ops.torch_ref import gp_predict_mean_grad_ref

    N, P, D, B = shape
    Xq, X, theta, alpha, y_mean, y_std = _problem64(N, P, D, B, aniso, seed=N + D)
    mean, jac = gp_predict_mean_grad_ref(Xq, X, theta, alpha, y_mean, y_std, nu, aniso)
    assert mean.shape == (P, B) and jac.shape == (P, B, D)
    assert mean.dtype == torch.float64 and jac.dtype == torch.float64

    xq = Xq.clone().requires_grad_(True)
    Ks = build_kernel_torch(xq, X, theta, nu=nu, anisotropic=aniso)  # (B, P, N)
    mean_ad = y_mean[None, :] + y_std[None, :] * (Ks * alpha[:, None, :]).sum(-1).T
    jac_ad = torch.stack([
        torch.autograd.grad(mean_ad[:, b].sum(), xq, retain_graph=True)[0]
        for b in range(B)
    ], dim=1)  # (P, B, D): row p of mean[:, b].sum()'s gradient is d mean[p, b]/d x_p
    merr = ((mean - mean_ad.detach()).abs().max() / mean_ad.abs().max().clamp_min(1.0)).item()
    err = ((jac - jac_ad).abs().max() / jac_ad.abs().max().clamp_min(1.0)).item()
    print(f"{shape} nu={nu} aniso={aniso}: jac err {err:.3e}, mean err {merr:.3e}")
    assert merr <= 1e-9
    assert err <= 1e-9


def test_closed_form_affine_and_nu_half_on_training_point():
    """Raw queries with q_lb / q_invrg give the unit-box Jacobian times
    1/xrg; a nu = 1/2 query ON a training point drops that point's term and
    stays finite."""
    from dmosopt_amd.ops.torch_ref import gp_predict_mean_grad_ref

    Xq, X, theta, alpha, y_mean, y_std = _problem64(40, 17, 4, 2, True, seed=3)
    Xq[0] = X[7]
    lb, rg = torch.as_tensor(XLB), torch.as_tensor(XUB - XLB)
    m_u, j_u = gp_predict_mean_grad_ref(Xq, X, theta, alpha, y_mean, y_std, 0.5, True)
    m_r, j_r = gp_predict_mean_grad_ref(lb + Xq * rg, X, theta, alpha, y_mean, y_std,
                                        0.5, True, lb, 1.0 / rg)
    assert torch.isfinite(j_u).all()
    assert torch.allclose(m_r, m_u, rtol=0, atol=1e-12)
    # row 0 apart: the affine round trip leaves r ~ 1e-16 where the unit-box
    # query has r = 0 exactly, and the nu = 1/2 term of that point returns
    assert torch.allclose(j_r[1:], (j_u / rg)[1:], rtol=1e-9, atol=1e-12)
    # the dropped term: the same query against the other 39 points
    keep = torch.arange(40) != 7
    _, j_wo = gp_predict_mean_grad_ref(Xq[:1], X[keep], theta, alpha[:, keep], y_mean,
                                       y_std, 0.5, True)
    assert torch.allclose(j_u[:1], j_wo, rtol=1e-12, atol=1e-14)


# ------------------------------------------------------- 2. gradient() units
def test_gradient_units_against_central_differences():
    gp = _box_model()
    rng = np.random.default_rng(1)
    P, d, m = 9, 4, 2
    x = XLB + (0.1 + 0.8 * rng.random((P, d))) * (XUB - XLB)  # interior
    jac = gp.gradient(x)
    assert jac.shape == (P, m, d) and jac.dtype == np.float64
    h = 1e-6 * (XUB - XLB)
    fd = np.empty_like(jac)
    for k in range(d):
        e = np.zeros(d)
        e[k] = h[k]
        fd[:, :, k] = (gp.evaluate(x + e) - gp.evaluate(x - e)) / (2.0 * h[k])
    err = np.abs(jac - fd).max() / np.abs(jac).max()
    print(f"gradient() vs central differences: {err:.3e}, max |jac| {np.abs(jac).max():.3f}")
    assert err <= 1e-6
    one = gp.gradient(x[3])  # 1-D input
    assert one.shape == (1, m, d) and np.array_equal(one[0], jac[3])
    # device-resident form: same numbers, tensor in and out
    jt = gp.gradient_tensor(torch.as_tensor(x))
    assert isinstance(jt, torch.Tensor) and np.array_equal(jt.numpy(), jac)
    # the gradient of the MEAN: mean-variance mode changes nothing
    gv = _box_model(return_mean_variance=True)
    assert np.array_equal(gv.gradient(x), jac)
    # unit-box form of the fitted posterior: raw = unit / range
    mean_u, jac_u = gp._fitted.predict_mean_grad(
        torch.as_tensor((x - XLB) / (XUB - XLB)))
    assert mean_u.shape == (P, m)
    assert np.allclose(mean_u.numpy(), gp.evaluate(x), rtol=1e-9, atol=1e-12)
    assert np.allclose(jac_u.numpy() / (XUB - XLB), jac, rtol=1e-12, atol=0)


# ---------------------------------------------------------- 3. dgsm_grad vs dgsm
def test_dgsm_grad_matches_finite_difference_dgsm():
    from dmosopt_amd.models.sa import SA_DGSM, SA_DGSM_Grad

    gp = _box_model()
    names = [f"x{i}" for i in range(4)]
    fd = SA_DGSM(XLB, XUB, names, ["f1", "f2"]).analyze(gp, 256)["S1"]
    an = SA_DGSM_Grad(XLB, XUB, names, ["f1", "f2"]).analyze(gp, 256)["S1"]
    assert list(an) == ["f1", "f2"]
    for name in ("f1", "f2"):
        assert an[name].shape == (4,)
        err = np.abs(an[name] - fd[name]).max() / an[name].max()
        print(f"{name}: S1 grad {an[name]} fd {fd[name]} rel diff {err:.3e}")
        assert err <= 1e-4


# ------------------------------------------------------ 4. fallback and registry
def test_fallback_without_gradient_and_registry(caplog):
    from dmosopt_amd import config as cfg
    from dmosopt_amd.models.sa import SA_DGSM, SA_DGSM_Grad

    class M:
        def evaluate(self, x):
            x = np.atleast_2d(x)
            return np.column_stack([3.0 * x[:, 0], 2.0 * x[:, 1]])

    args = (np.zeros(4), np.ones(4), [f"x{i}" for i in range(4)], ["f1", "f2"])
    want = SA_DGSM(*args).analyze(M(), 2048)["S1"]
    with caplog.at_level(logging.INFO):
        got = SA_DGSM_Grad(*args).analyze(M(), 2048)["S1"]
    assert any("falling back" in r.getMessage() for r in caplog.records)
    assert list(got) == list(want)
    for name in want:
        assert np.array_equal(got[name], want[name])
    assert np.argmax(got["f1"]) == 0 and np.argmax(got["f2"]) == 1
    assert cfg.resolve(cfg.sensitivity_registry, "dgsm_grad") is SA_DGSM_Grad


def test_dgsm_grad_through_run():
    import dmosopt_amd

    def sphere2(pp):
        x = np.array([pp[k] for k in sorted(pp.keys())])
        return np.array([np.sum(x**2), np.sum((x - 1.0) ** 2)])

    params = {
        "opt_id": "m_sa_dgsm_grad",
        "obj_fun": sphere2,
        "problem_parameters": {},
        "space": {f"x{i}": [0.0, 1.0] for i in range(4)},
        "objective_names": ["f1", "f2"],
        "population_size": 16,
        "num_generations": 3,
        "initial_maxiter": 2,
        "n_initial": 2,
        "n_epochs": 2,
        "surrogate_method_name": "gpr",
        "surrogate_method_kwargs": {"anisotropic": False, "optimizer": "sceua"},
        "sensitivity_method_name": "dgsm_grad",
        "random_seed": 5,
    }
    assert dmosopt_amd.run(params, verbose=False) is not None


# ------------------------------------------------------------- 5. world-2 gloo
def _shard_grad_worker(rank, world_size, port, out_q):
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world_size)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, _ROOT)
    import torch.distributed as dist

    from dmosopt_amd.parallel import comm
    from dmosopt_amd.parallel.context import get_context
    from dmosopt_amd.parallel.sharded import ShardedObjective

    comm.init_from_env()
    ctx = get_context()
    gp = _box_model()
    obj = ShardedObjective(gp, ctx)
    rng = np.random.default_rng(3)
    xq = XLB + rng.random((7, 4)) * (XUB - XLB)  # odd count exercises the pad row
    got = obj.gradient(xq)
    want = gp.gradient(xq)  # single-model reference on every rank

    class NoGrad:
        def evaluate(self, x):
            return np.atleast_2d(x)[:, :2]

    ok = (got.shape == (7, 2, 4) and got.dtype == np.float64
          and np.array_equal(got, want) and hasattr(obj, "gradient")
          and not hasattr(ShardedObjective(NoGrad(), ctx), "gradient"))
    dist.destroy_process_group()
    out_q.put((rank, bool(ok), float(np.abs(got - want).max())))


def test_sharded_gradient_matches_single_rank_bitwise():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_shard_grad_worker, args=(r, 2, 29823, q))
             for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == [0, 1]
    assert all(r[1] for r in res), res
