"""Fused input-gradient kernels of the GP posterior mean
(ops/hip/gp_mean_grad.hip, binding ``_hipops.gp_predict_mean_grad``), the
``ops`` dispatch, ``GPRMatern.gradient`` on the GPU and ``dgsm_grad`` on it.

The oracle is the float64 closed form on the CPU
(``torch_ref.gp_predict_mean_grad_ref``), evaluated from the SAME
float32-representable X, Xq, theta and the same float32 alpha the kernel
receives, so the test measures the kernel and not the conditioning of the
solve. A case's error is max |delta| / max(1, max |jac64|) per objective, in
unit-box and standardised units (y_std = 1, no affine); the worst objective
counts. Every case asserts max |jac64| >= 0.1 per objective, so the clamp at
1 never hides a vanishing gradient.

JAC_TOL = 8 x the worst error of an fp32 emulation of the closed form
(``gp_predict_mean_grad_ref`` in float32 on the CPU) on these very inputs, the
margin VAR_ATOL and GRAD_TOL got, which leaves room for __expf and the
summation order:
  emulated: worst 3.12e-7 (N=32, P=32, D=3, nu=3/2), N=300, D=30: 3.11e-7, every
            other case <= 2.4e-7 (D=129 fallback case 5.4e-8, nu=1/2 on a
            training row 1.3e-7)  ->  JAC_TOL = 2.50e-6
  observed on the MI355X: worst 1.12e-6 (N=300, P=97, D=30, nu=5/2), every
            other case <= 3.9e-7 (D=129 fallback 4.1e-8, nu=1/2 on a training
            row 1.1e-7)

MODEL_TOL (test 7) is measured the same way one level up: ``gradient(x)`` of a
float32 CPU model against the float64 CPU model of the same archive and
theta, x 8. This one includes the float32 solve for alpha:
  emulated: gradient 3.32e-6, relative S1 4.0e-6  ->  MODEL_TOL = 2.66e-5,
            S1 judged against 2 x MODEL_TOL (S1 is a mean of squares)
  observed on the MI355X: gradient 3.63e-6, relative S1 3.7e-6
"""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INF = float("inf")
EMULATED_WORST = 3.12e-7  # fp32 closed form on the CPU, worst of emulated_errors()
JAC_TOL = 8 * EMULATED_WORST
MODEL_EMULATED = 3.32e-6  # float32 vs float64 CPU model, emulated_model_error()
MODEL_TOL = 8 * MODEL_EMULATED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dmosopt_amd import ops

    assert ops.native_available(), "native extension must be built on a GPU box"
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ helpers
def _problem(N, P, B, D, aniso, seed, on_train=False):
    """float32 CPU inputs in unit-box, standardised units: X (N,D) and Xq
    (P,D) uniform, theta (B,p) with ell = 0.5 * U(0.7, 1.4), times sqrt(D/6)
    for D > 6 (a fixed ell in a wide box leaves no gradient to measure),
    sf2 = 1.1, noise = 1e-3, and alpha (B,N) = K^-1 y of smooth targets,
    solved in float64 and rounded to float32. ``on_train`` puts query 0 on a
    training row."""
    from dmosopt_amd.models.gp_core import build_kernel_torch

    g = torch.Generator().manual_seed(seed)
    X = torch.rand(N, D, generator=g).float()
    Xq = torch.rand(P, D, generator=g).float()
    if on_train:
        Xq[0] = X[N // 2]
    n_ell = D if aniso else 1
    ell = 0.5 * (0.7 + 0.7 * torch.rand(B, n_ell, generator=g))
    if D > 6:
        ell = ell * math.sqrt(D / 6.0)
    theta = torch.cat([
        torch.full((B, 1), math.log(1.1)), torch.log(ell),
        torch.full((B, 1), math.log(1e-3)),
    ], dim=1).float()
    w = torch.rand(D, B, generator=g).double()
    X64 = X.double()
    Y = torch.sin(3.0 * (X64 @ w) / math.sqrt(D)) + 0.3 * torch.cos(
        X64.sum(1, keepdim=True))
    nu_solve = 2.5  # alpha is an input of the kernel under test: any SPD K does
    K = build_kernel_torch(X64, None, theta.double(), nu=nu_solve,
                           anisotropic=aniso, jitter=1e-6)
    alpha = torch.linalg.solve(K, Y.T[:, :, None])[:, :, 0].float().contiguous()
    return Xq, X, theta, alpha


def _oracle(Xq, X, theta, alpha, nu, aniso):
    """float64 (mean (P,B), jac (P,B,D)), y_mean = 0, y_std = 1."""
    from dmosopt_amd.ops.torch_ref import gp_predict_mean_grad_ref

    B = theta.shape[0]
    mean, jac = gp_predict_mean_grad_ref(
        Xq.double(), X.double(), theta.double(), alpha.double(),
        torch.zeros(B, dtype=torch.float64), torch.ones(B, dtype=torch.float64),
        nu, aniso)
    assert torch.isfinite(jac).all()
    amax = jac.abs().amax(dim=(0, 2))
    assert (amax >= 0.1).all(), f"vacuous case: max |jac64| per objective {amax}"
    return mean, jac


def _jac_error(jac, jac64):
    scale = jac64.abs().amax(dim=(0, 2)).clamp_min(1.0)  # per objective
    return ((jac.double().cpu() - jac64).abs().amax(dim=(0, 2)) / scale).max().item()


def _std(B, dev=None):
    return torch.zeros(B, device=dev), torch.ones(B, device=dev)


def _native(dev, Xq, X, theta, alpha, nu, aniso, y_mean=None, y_std=None,
            q_lb=None, q_invrg=None):
    from dmosopt_amd import _hipops

    B = theta.shape[0]
    if y_mean is None:
        y_mean, y_std = _std(B)
    to = lambda t: None if t is None else t.to(dev)
    return _hipops.gp_predict_mean_grad(
        Xq.to(dev), X.to(dev), theta.to(dev), alpha.to(dev), y_mean.to(dev),
        y_std.to(dev), 0.0 if nu == INF else nu, aniso, to(q_lb), to(q_invrg))


# ------------------------------------------- 1. shapes the tiling can miss
# (N, P, B, D, nu, aniso)
JAC_CASES = [
    (1, 1, 1, 1, 2.5, False),      # single point, single query
    (31, 5, 2, 1, 0.5, True),      # one short of a tile, points on a line
    (32, 32, 1, 3, 1.5, False),    # exactly one tile each way
    (33, 33, 3, 6, INF, True),     # one past a tile each way
    (64, 65, 2, 30, 0.5, False),   # two N-splits, ragged third query tile
    (97, 1, 2, 7, 1.5, True),      # four N-splits, one query
    (300, 97, 2, 30, 2.5, False),  # the workload's N and D
    (65, 40, 2, 128, 2.5, True),   # the D bound
]
ON_TRAIN_CASE = (40, 9, 2, 5, 0.5, True)   # test 5
FALLBACK_CASE = (33, 7, 2, 129, 2.5, True)  # test 6


def _case_inputs(case, on_train=False):
    N, P, B, D, nu, aniso = case
    return _problem(N, P, B, D, aniso, seed=2000 + N + D, on_train=on_train)


def emulated_errors():
    """Error of the closed form in float32 on the CPU against the float64
    oracle on the test's own inputs, per case (tests 1, 5 and 6)."""
    from dmosopt_amd.ops.torch_ref import gp_predict_mean_grad_ref

    out = {}
    for case in JAC_CASES + [ON_TRAIN_CASE, FALLBACK_CASE]:
        N, P, B, D, nu, aniso = case
        Xq, X, theta, alpha = _case_inputs(case, on_train=case is ON_TRAIN_CASE)
        _, j64 = _oracle(Xq, X, theta, alpha, nu, aniso)
        _, j32 = gp_predict_mean_grad_ref(Xq, X, theta, alpha, *_std(B), nu, aniso)
        assert j32.dtype == torch.float32
        out[case] = _jac_error(j32, j64)
    return out


@pytest.mark.parametrize(
    "case", JAC_CASES,
    ids=lambda c: f"N{c[0]}-P{c[1]}-B{c[2]}-D{c[3]}-nu{c[4]}-{'ard' if c[5] else 'iso'}")
def test_jacobian_matches_float64_oracle(dev, case):
    N, P, B, D, nu, aniso = case
    Xq, X, theta, alpha = _case_inputs(case)
    m64, j64 = _oracle(Xq, X, theta, alpha, nu, aniso)
    mean, jac = _native(dev, Xq, X, theta, alpha, nu, aniso)
    assert mean.shape == (P, B) and jac.shape == (P, B, D)
    assert mean.dtype == torch.float32 and jac.dtype == torch.float32
    assert torch.isfinite(jac).all()
    err = _jac_error(jac, j64)
    print(f"N={N} P={P} B={B} D={D} nu={nu} aniso={aniso}: jac err {err:.3e} "
          f"(tol {JAC_TOL:.3e}), max |jac64| {j64.abs().max():.3f}")
    assert err <= JAC_TOL


# ------------------------------------------------- 2. mean columns, bitwise
@pytest.mark.parametrize("affine", [False, True])
def test_mean_bitwise_equal_to_gp_predict_mean(dev, affine):
    from dmosopt_amd import _hipops

    Xq, X, theta, alpha = _problem(97, 65, 3, 7, True, seed=11)
    y_mean, y_std = torch.tensor([0.3, -1.2, 4.0]), torch.tensor([2.5, 0.4, 1.7])
    q_lb = q_invrg = None
    if affine:
        q_lb = torch.linspace(-1.0, 2.0, 7)
        q_invrg = 1.0 / torch.linspace(0.5, 10.0, 7)
        Xq = (q_lb + Xq / q_invrg).float()
    mean, _ = _native(dev, Xq, X, theta, alpha, 2.5, True, y_mean, y_std, q_lb, q_invrg)
    to = lambda t: None if t is None else t.to(dev)
    want = _hipops.gp_predict_mean(
        Xq.to(dev), X.to(dev), theta.to(dev), alpha.to(dev), y_mean.to(dev),
        y_std.to(dev), 2.5, True, to(q_lb), to(q_invrg))
    assert torch.isfinite(want).all()
    assert torch.equal(mean, want)


# ------------------------------------------------------------ 3. affine path
def test_affine_path_scales_the_unit_box_jacobian(dev):
    xlb = torch.tensor([-1.0, 0.0, 2.0, -5.0])
    xrg = torch.tensor([2.0, 3.0, 0.5, 10.0])
    invrg = (1.0 / xrg.double()).float()
    U, X, theta, alpha = _problem(40, 33, 2, 4, True, seed=5)
    raw = (xlb + U * xrg).float()
    u32 = (raw - xlb) * invrg  # the kernel's own normalisation, same two ops
    y_mean, y_std = torch.tensor([0.3, -1.2]), torch.tensor([2.5, 0.4])
    _, j_unit = _native(dev, u32, X, theta, alpha, 1.5, True)
    _, j_raw = _native(dev, raw, X, theta, alpha, 1.5, True, y_mean, y_std, xlb, invrg)
    want = j_unit.double().cpu() * y_std.double()[None, :, None] / xrg.double()
    rel = ((j_raw.double().cpu() - want).abs() / want.abs()).max().item()
    print(f"affine epilogue: worst relative difference {rel:.3e}")
    assert rel <= 1e-6


# ------------------------------------- 4. batch invariance and repeatability
@pytest.mark.parametrize("D,nu,aniso", [(7, 2.5, True), (30, 0.5, False)])
def test_batch_invariance_and_repeatability(dev, D, nu, aniso):
    Xq, X, theta, alpha = _problem(97, 65, 2, D, aniso, seed=17 + D)
    m_full, j_full = _native(dev, Xq, X, theta, alpha, nu, aniso)
    m_again, j_again = _native(dev, Xq, X, theta, alpha, nu, aniso)
    assert torch.equal(j_full, j_again) and torch.equal(m_full, m_again)
    for rows in (slice(0, 1), slice(5, 38), slice(None, None, 3)):
        _, j = _native(dev, Xq[rows].contiguous(), X, theta, alpha, nu, aniso)
        assert torch.equal(j, j_full[rows]), rows


# --------------------------------------------- 5. nu = 1/2 on a training row
def test_nu_half_query_on_training_row(dev):
    N, P, B, D, nu, aniso = ON_TRAIN_CASE
    Xq, X, theta, alpha = _case_inputs(ON_TRAIN_CASE, on_train=True)
    assert torch.equal(Xq[0], X[N // 2])
    _, j64 = _oracle(Xq, X, theta, alpha, nu, aniso)
    _, jac = _native(dev, Xq, X, theta, alpha, nu, aniso)
    assert torch.isfinite(jac).all()
    err = _jac_error(jac, j64)
    err0 = _jac_error(jac[:1], j64[:1])
    print(f"nu=1/2, query 0 on a training row: err {err:.3e}, row 0 {err0:.3e}")
    assert err <= JAC_TOL


# ------------------------------------------------------ 6. D = 129 falls back
def test_d129_falls_back_to_closed_form(dev):
    from dmosopt_amd import ops
    from dmosopt_amd.ops.torch_ref import gp_predict_mean_grad_ref

    N, P, B, D, nu, aniso = FALLBACK_CASE
    Xq, X, theta, alpha = _case_inputs(FALLBACK_CASE)
    _, j64 = _oracle(Xq, X, theta, alpha, nu, aniso)
    g = [t.to(dev) for t in (Xq, X, theta, alpha, *_std(B))]
    mean, jac = ops.gp_predict_mean_grad(*g, nu, aniso)
    assert jac.is_cuda and jac.shape == (P, B, D) and jac.dtype == torch.float32
    m_ref, j_ref = gp_predict_mean_grad_ref(*g, nu, aniso)
    assert torch.equal(jac, j_ref) and torch.equal(mean, m_ref)
    err = _jac_error(jac, j64)
    print(f"D=129 fallback: err {err:.3e}")
    assert err <= JAC_TOL
    with pytest.raises(RuntimeError, match="launch bounds"):
        _native(dev, Xq, X, theta, alpha, nu, aniso)
    # one dimension fewer takes the native path through the same entry point
    # (theta cut to width 130: its last column is never read by the gradient)
    g128 = [g[0][:, :128].contiguous(), g[1][:, :128].contiguous(),
            g[2][:, :130].contiguous(), *g[3:]]
    _, j_nat = ops.gp_predict_mean_grad(*g128, nu, aniso)
    _, j_dir = _native(dev, *[t.cpu() for t in g128[:4]], nu, aniso)
    assert torch.equal(j_nat, j_dir)


# ------------------------------------------------------------ 7. model level
M_LB = np.array([-1.0, 0.0, 2.0, -5.0, 0.0, 10.0])
M_UB = np.array([1.0, 3.0, 2.5, 5.0, 1.0, 20.0])
M_THETA = np.array([[0.1, math.log(0.6), math.log(1e-3)],
                    [0.0, math.log(0.9), math.log(1e-3)]])


def _model(device, dtype, **kw):
    """GPRMatern with given hyperparameters on a smooth target, N = 60,
    d = 6, m = 2, from an archive of float32-representable points."""
    from dmosopt_amd.models.gp import GPRMatern

    rng = np.random.default_rng(0)
    u = rng.random((60, 6)).astype(np.float32).astype(np.float64)
    x = (M_LB + u * (M_UB - M_LB)).astype(np.float32).astype(np.float64)
    y = np.column_stack([np.sin(3.0 * u[:, 0]) + u[:, 1] ** 2 + 0.5 * u[:, 4],
                         np.cos(2.0 * u[:, 2]) + 0.1 * u[:, 3] + u[:, 5] ** 3])
    y = y.astype(np.float32).astype(np.float64)
    return GPRMatern(x, y, 6, 2, M_LB, M_UB, theta_override=M_THETA,
                     device=device, dtype=dtype, **kw)


def _model_queries():
    rng = np.random.default_rng(1)
    u = 0.05 + 0.9 * rng.random((33, 6))
    return (M_LB + u * (M_UB - M_LB)).astype(np.float32).astype(np.float64)


def _model_error(jac, jac64):
    scale = np.maximum(np.abs(jac64).max(axis=(0, 2)), 1.0)
    return (np.abs(jac - jac64).max(axis=(0, 2)) / scale).max()


def _s1_error(model, model64):
    from dmosopt_amd.models.sa import SA_DGSM_Grad

    names = [f"x{i}" for i in range(6)]
    a = SA_DGSM_Grad(M_LB, M_UB, names, ["f1", "f2"]).analyze(model, 512)["S1"]
    b = SA_DGSM_Grad(M_LB, M_UB, names, ["f1", "f2"]).analyze(model64, 512)["S1"]
    return max(np.abs(a[k] - b[k]).max() / b[k].max() for k in ("f1", "f2"))


def emulated_model_error():
    """(gradient error, relative S1 error) of a float32 CPU model against
    the float64 CPU model of the same archive and theta."""
    m64 = _model("cpu", torch.float64)
    m32 = _model("cpu", torch.float32)
    x = _model_queries()
    return _model_error(m32.gradient(x), m64.gradient(x)), _s1_error(m32, m64)


def test_model_gradient_and_dgsm_grad(dev):
    m64 = _model("cpu", torch.float64)
    mg = _model("cuda", torch.float32)
    x = _model_queries()
    j64 = m64.gradient(x)
    assert (np.abs(j64).max(axis=(0, 2)) >= 0.1).all()
    jac = mg.gradient(x)
    assert jac.shape == (33, 2, 6) and jac.dtype == np.float64
    jt = mg.gradient_tensor(torch.as_tensor(x, dtype=torch.float32, device=dev))
    assert jt.is_cuda and jt.dtype == torch.float32
    assert np.array_equal(jt.cpu().numpy().astype(np.float64), jac)
    err = _model_error(jac, j64)
    s1 = _s1_error(mg, m64)
    print(f"model gradient err {err:.3e} (tol {MODEL_TOL:.3e}), "
          f"dgsm_grad S1 rel err {s1:.3e} (tol {2 * MODEL_TOL:.3e})")
    assert err <= MODEL_TOL
    assert s1 <= 2 * MODEL_TOL
    # mean-variance mode changes nothing; a bf16 model answers from the
    # float32 closed form of its own alpha (no bf16 kernel on this path)
    mv = _model("cuda", torch.float32, return_mean_variance=True)
    assert np.array_equal(mv.gradient(x), jac)
    mb = _model("cuda", torch.float32, compute="bf16")
    jb = mb.gradient_tensor(torch.as_tensor(x, dtype=torch.float32, device=dev))
    from dmosopt_amd import _hipops

    cache, pa = mb._native_pred_cache(dev)
    want = _hipops.gp_predict_mean_grad(
        torch.as_tensor(x, dtype=torch.float32, device=dev), *pa, cache[1], cache[2])[1]
    assert torch.isfinite(jb).all() and torch.equal(jb, want)
