"""Random-feature kernels of the GP posterior sample path
(ops/hip/gp_path.hip, binding ``_hipops.gp_predict_path``), the ``ops``
dispatch, ``GPRMatern(thompson=True)`` on the GPU and a short Thompson run.

The oracle is the float64 closed form on the CPU (``ops.gp_predict_path`` on
float64 CPU tensors: torch cross kernel, bmm and
``torch_ref.gp_path_features_ref``), evaluated from the SAME
float32-representable X, Xq, theta, alpha', Omega, tau and amp the kernel
receives, in unit-box and standardised units (no affine, y_std = 1). A case's
error is max |delta| / max(1, max |path64|) per batch row; the worst row
counts. Every case asserts max |path64| >= 0.1 per row.

PATH_TOL = 8 x the worst error of the fp32 emulation on these very inputs
(the same composition in float32 on the CPU), the rule JAC_TOL, VAR_ATOL and
GRAD_TOL were set by:
  emulated: worst 2.13e-5 (N=33, P=33, D=3, M=130, RBF, ARD), the other
            D = 3 cases 2.6e-6 .. 1.7e-5, N=300, D=30: 2.3e-6, D=128: 1.6e-6,
            large phases 1.4e-7, D=129 fallback 4.3e-7  ->  PATH_TOL = 1.71e-4
  observed on the MI355X: worst 2.02e-5 (the same case), the other D = 3
            cases 1.6e-6 .. 9.7e-6, N=300, D=30: 2.0e-6, D=128: 1.5e-6, large
            phases (5.8e5 turns) 1.0e-7, D=129 fallback 6.6e-7
Both are the float32 cancellation in k(u, X) alpha' (max |alpha'| ~ 1e2 at
noise 1e-3), not the feature term: the large-phase case, where the update
term vanishes (ell = 1e-3), sits at 1e-7.

MODEL_TOL (test 7) is measured the same way one level up:
``evaluate_tensor(x)`` of a float32 CPU Thompson model against the float64 CPU
model of the same archive, theta and seed, x 8. This one includes the float32
solve for alpha':
  emulated: path 3.25e-5, identity of the float32 CPU model 1.39e-5 (float64:
            3.6e-14)  ->  MODEL_TOL = 2.60e-4
  observed on the MI355X: path 2.38e-5, identity 2.95e-5
"""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INF = float("inf")
F64 = torch.float64
EMULATED_WORST = 2.14e-5  # fp32 composition on the CPU, worst of emulated_errors()
PATH_TOL = 8 * EMULATED_WORST
MODEL_EMULATED = 3.25e-5  # float32 vs float64 CPU model, emulated_model_error()
MODEL_TOL = 8 * MODEL_EMULATED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dmosopt_amd import ops

    assert ops.native_available(), "native extension must be built on a GPU box"
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ helpers
_CACHE = {}


def _problem(N, P, D, M, B, nu, aniso, ell_fixed=None):
    """float32 CPU inputs (Xq, X, theta, alpha', Omega, tau, amp) of one path
    per batch row: X (N,D) and Xq (P,D) uniform in the unit box, theta (B,p)
    with ell = 0.5 * U(0.7, 1.4), times sqrt(D/6) for D > 6 (``ell_fixed``
    overrides), sf2 = 1.1, noise = 1e-3, smooth targets, and the path drawn by
    a float64 CPU fit of exactly these values (FittedGP.sample_paths), its
    alpha' rounded to float32. Built once per case and never modified."""
    key = (N, P, D, M, B, nu, aniso, ell_fixed)
    if key in _CACHE:
        return _CACHE[key]
    from dmosopt_amd.models.gp_core import FittedGP

    g = torch.Generator().manual_seed(3000 + N + D + M)
    X = torch.rand(N, D, generator=g).float()
    Xq = torch.rand(P, D, generator=g).float()
    n_ell = D if aniso else 1
    ell = 0.5 * (0.7 + 0.7 * torch.rand(B, n_ell, generator=g))
    if D > 6:
        ell = ell * math.sqrt(D / 6.0)
    if ell_fixed is not None:
        ell = torch.full((B, n_ell), ell_fixed)
    theta = torch.cat([
        torch.full((B, 1), math.log(1.1)), torch.log(ell),
        torch.full((B, 1), math.log(1e-3)),
    ], dim=1).float()
    w = torch.rand(D, B, generator=g).double()
    X64 = X.double()
    Y = torch.sin(3.0 * (X64 @ w) / math.sqrt(D)) + 0.3 * torch.cos(
        X64.sum(1, keepdim=True))
    fit = FittedGP(X64, Y, theta.double(), torch.zeros(B, dtype=F64),
                   torch.ones(B, dtype=F64), nu=nu, anisotropic=aniso)
    s = fit.sample_paths(1, M, seed=N + M)
    out = (Xq, X, theta, s.alpha.float().contiguous(), s.Omega, s.tau, s.amp)
    _CACHE[key] = out
    return out


def _std(B, dev=None, dtype=torch.float32):
    return (torch.zeros(B, device=dev, dtype=dtype),
            torch.ones(B, device=dev, dtype=dtype))


def _composition(prob, nu, aniso, dtype):
    """ops.gp_predict_path on CPU tensors of ``dtype`` (the torch composition):
    float64 is the oracle, float32 the emulation."""
    from dmosopt_amd import ops

    Xq, X, theta, alpha, Omega, tau, amp = prob
    B = theta.shape[0]
    return ops.gp_predict_path(
        Xq.to(dtype), X.to(dtype), theta.to(dtype), alpha.to(dtype),
        *_std(B, dtype=dtype), nu, aniso, Omega, tau, amp)


def _oracle(prob, nu, aniso):
    p64 = _composition(prob, nu, aniso, F64)
    assert p64.dtype == F64 and torch.isfinite(p64).all()
    amax = p64.abs().amax(dim=0)
    assert (amax >= 0.1).all(), f"vacuous case: max |path64| per row {amax}"
    return p64


def _path_error(path, p64):
    scale = p64.abs().amax(dim=0).clamp_min(1.0)  # per batch row
    return ((path.double().cpu() - p64).abs().amax(dim=0) / scale).max().item()


def _native(dev, prob, nu, aniso, y_mean=None, y_std=None, q_lb=None,
            q_invrg=None, Xq=None):
    from dmosopt_amd import _hipops

    Xq0, X, theta, alpha, Omega, tau, amp = prob
    Xq = Xq0 if Xq is None else Xq
    if y_mean is None:
        y_mean, y_std = _std(theta.shape[0])
    to = lambda t: None if t is None else t.to(dev)
    return _hipops.gp_predict_path(
        Xq.to(dev), X.to(dev), theta.to(dev), alpha.to(dev), y_mean.to(dev),
        y_std.to(dev), 0.0 if nu == INF else nu, aniso, Omega.to(dev),
        tau.to(dev), amp.to(dev), to(q_lb), to(q_invrg))


# (N, P, D, M, B)
SHAPES = [(32, 1, 1, 128, 1), (33, 33, 3, 130, 3), (300, 97, 30, 1024, 2),
          (64, 32, 128, 256, 2)]
# (N, P, D, M, B, nu, aniso)
PATH_CASES = [s + (2.5, an) for s in SHAPES for an in (False, True)] + [
    SHAPES[1] + (nu, an) for nu in (1.5, 0.5, INF) for an in (False, True)]
LARGE_PHASE_CASE = (40, 33, 3, 1024, 2, 0.5, False)  # ell = 1e-3, test 2
FALLBACK_CASE = (33, 7, 129, 96, 2, 2.5, True)       # test 6


def _case_inputs(case):
    N, P, D, M, B, nu, aniso = case
    return _problem(N, P, D, M, B, nu, aniso,
                    ell_fixed=1e-3 if case is LARGE_PHASE_CASE else None)


def emulated_errors():
    """Error of the float32 composition on the CPU against the float64 oracle
    on the test's own inputs, per case (tests 1, 2 and 6)."""
    out = {}
    for case in PATH_CASES + [LARGE_PHASE_CASE, FALLBACK_CASE]:
        prob = _case_inputs(case)
        p32 = _composition(prob, case[5], case[6], torch.float32)
        assert p32.dtype == torch.float32
        out[case] = _path_error(p32, _oracle(prob, case[5], case[6]))
    return out


# ------------------------------------------------------------ 1. oracle sweep
@pytest.mark.parametrize(
    "case", PATH_CASES,
    ids=lambda c: f"N{c[0]}-P{c[1]}-D{c[2]}-M{c[3]}-B{c[4]}-nu{c[5]}-"
                  f"{'ard' if c[6] else 'iso'}")
def test_path_matches_float64_oracle(dev, case):
    N, P, D, M, B, nu, aniso = case
    prob = _case_inputs(case)
    p64 = _oracle(prob, nu, aniso)
    path = _native(dev, prob, nu, aniso)
    assert path.shape == (P, B) and path.dtype == torch.float32
    assert torch.isfinite(path).all()
    err = _path_error(path, p64)
    print(f"N={N} P={P} D={D} M={M} B={B} nu={nu} aniso={aniso}: path err "
          f"{err:.3e} (tol {PATH_TOL:.3e}), max |path64| {p64.abs().max():.3f}")
    assert err <= PATH_TOL


# ------------------------------------------------------------ 2. large phases
def test_large_phases_keep_their_fraction(dev):
    """nu = 1/2 with ell = 1e-3: Cauchy-tailed frequencies. A phase summed in
    float32 has an error of ~1e-4 turns per 1e3 turns and fails PATH_TOL."""
    N, P, D, M, B, nu, aniso = LARGE_PHASE_CASE
    prob = _case_inputs(LARGE_PHASE_CASE)
    Xq, _, _, _, Omega, tau, _ = prob
    phase = tau.double()[:, None, :] + torch.einsum(
        "pd,bmd->bpm", Xq.double(), Omega.double())
    assert phase.abs().max().item() > 1e3
    p64 = _oracle(prob, nu, aniso)
    path = _native(dev, prob, nu, aniso)
    err = _path_error(path, p64)
    print(f"large phases: max |phase| {phase.abs().max():.3e} turns, path err "
          f"{err:.3e} (tol {PATH_TOL:.3e})")
    assert err <= PATH_TOL


# --------------------------------------------------------- 3. bitwise mean part
@pytest.mark.parametrize("affine", [False, True])
def test_zero_amplitude_is_gp_predict_mean_bitwise(dev, affine):
    from dmosopt_amd import _hipops

    Xq, X, theta, alpha, Omega, tau, amp = _problem(97, 65, 7, 200, 3, 2.5, True)
    y_mean, y_std = torch.tensor([0.3, -1.2, 4.0]), torch.tensor([2.5, 0.4, 1.7])
    q_lb = q_invrg = None
    if affine:
        q_lb = torch.linspace(-1.0, 2.0, 7)
        q_invrg = 1.0 / torch.linspace(0.5, 10.0, 7)
        Xq = (q_lb + Xq / q_invrg).float()
    prob = (Xq, X, theta, alpha, Omega, tau, torch.zeros_like(amp))
    got = _native(dev, prob, 2.5, True, y_mean, y_std, q_lb, q_invrg)
    to = lambda t: None if t is None else t.to(dev)
    want = _hipops.gp_predict_mean(
        Xq.to(dev), X.to(dev), theta.to(dev), alpha.to(dev), y_mean.to(dev),
        y_std.to(dev), 2.5, True, to(q_lb), to(q_invrg))
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)
    # and with the amplitudes back the features do contribute
    full = _native(dev, (Xq, X, theta, alpha, Omega, tau, amp), 2.5, True,
                   y_mean, y_std, q_lb, q_invrg)
    assert (full - want).abs().max().item() > 1e-3


# ------------------------------------- 4. batch invariance and repeatability
@pytest.mark.parametrize("D,nu,aniso", [(7, 2.5, True), (30, 0.5, False)])
def test_batch_invariance_and_repeatability(dev, D, nu, aniso):
    prob = _problem(97, 97, D, 200, 2, nu, aniso)
    Xq = prob[0]
    full = _native(dev, prob, nu, aniso)
    assert torch.equal(full, _native(dev, prob, nu, aniso))
    for rows in (slice(0, 1), slice(40, 41), slice(0, 32), slice(32, 97),
                 slice(None, None, 3)):
        part = _native(dev, prob, nu, aniso, Xq=Xq[rows].contiguous())
        assert torch.equal(part, full[rows]), rows


# ------------------------------------------------------------------ 5. affine
def test_affine_in_the_load_is_the_float32_normalisation(dev):
    xlb = torch.tensor([-1.0, 0.0, 2.0, -5.0])
    xrg = torch.tensor([2.0, 3.0, 0.5, 10.0])
    invrg = (1.0 / xrg.double()).float()
    prob = _problem(40, 33, 4, 130, 2, 1.5, True)
    raw = (xlb + prob[0] * xrg).float()
    u32 = (raw - xlb) * invrg  # the kernel's own normalisation, same two ops
    y_mean, y_std = torch.tensor([0.3, -1.2]), torch.tensor([2.5, 0.4])
    unit = _native(dev, prob, 1.5, True, y_mean, y_std, Xq=u32)
    got = _native(dev, prob, 1.5, True, y_mean, y_std, xlb, invrg, Xq=raw)
    assert torch.isfinite(got).all()
    assert torch.equal(got, unit)


# ------------------------------------------------------ 6. D = 129 falls back
def test_d129_falls_back_to_closed_form(dev):
    from dmosopt_amd import ops

    N, P, D, M, B, nu, aniso = FALLBACK_CASE
    prob = _case_inputs(FALLBACK_CASE)
    p64 = _oracle(prob, nu, aniso)
    g = [t.to(dev) for t in prob]
    path = ops.gp_predict_path(*g[:4], *_std(B, dev), nu, aniso, *g[4:])
    assert path.is_cuda and path.shape == (P, B) and path.dtype == torch.float32
    err = _path_error(path, p64)
    print(f"D=129 fallback: err {err:.3e} (tol {PATH_TOL:.3e})")
    assert err <= PATH_TOL
    with pytest.raises(RuntimeError, match="launch bounds"):
        _native(dev, prob, nu, aniso)
    # one dimension fewer takes the native path through the same entry point
    g128 = [g[0][:, :128].contiguous(), g[1][:, :128].contiguous(),
            torch.cat([g[2][:, :129], g[2][:, -1:]], dim=1).contiguous(), g[3],
            g[4][:, :, :128].contiguous(), g[5], g[6]]
    nat = ops.gp_predict_path(*g128[:4], *_std(B, dev), nu, aniso, *g128[4:])
    direct = _native(dev, [t.cpu() for t in g128], nu, aniso)
    assert torch.equal(nat, direct)


# ------------------------------------------------------------ 7. model level
M_LB = np.array([-1.0, 0.0, 2.0, -5.0])
M_UB = np.array([1.0, 3.0, 2.5, 5.0])
M_THETA = np.array([[0.1, math.log(0.6), math.log(1e-3)],
                    [0.0, math.log(0.9), math.log(1e-3)]])


def _model_archive():
    rng = np.random.default_rng(0)
    u = rng.random((60, 4)).astype(np.float32).astype(np.float64)
    x = (M_LB + u * (M_UB - M_LB)).astype(np.float32).astype(np.float64)
    y = np.column_stack([np.sin(3.0 * u[:, 0]) + u[:, 1] ** 2,
                         np.cos(2.0 * u[:, 2]) + 0.1 * u[:, 3]])
    return x, y.astype(np.float32).astype(np.float64)


def _model(device, dtype, **kw):
    """Thompson GPRMatern with given hyperparameters and seed, N = 60, d = 4,
    m = 2, from an archive of float32-representable points."""
    from dmosopt_amd.models.gp import GPRMatern

    x, y = _model_archive()
    return GPRMatern(x, y, 4, 2, M_LB, M_UB, theta_override=M_THETA, seed=12,
                     thompson=True, path_features=512, device=device,
                     dtype=dtype, **kw)


def _model_queries():
    rng = np.random.default_rng(1)
    u = 0.05 + 0.9 * rng.random((33, 4))
    return (M_LB + u * (M_UB - M_LB)).astype(np.float32).astype(np.float64)


def _model_error(v, v64):
    scale = np.maximum(np.abs(v64).max(axis=0), 1.0)
    return (np.abs(v - v64).max(axis=0) / scale).max()


def _model_identity_error(mdl):
    """max |path_n(X) - (y_n - eps - diag_add * alpha)| from the model's own
    draw, in standardised units."""
    f, s = mdl._fitted, mdl._thompson_path.sample
    x, y = _model_archive()
    to64 = lambda t: t.detach().double().cpu()
    yn = (torch.as_tensor(y) - to64(f.y_mean)) / to64(f.y_std)
    xt = torch.as_tensor(x, dtype=mdl.dtype, device=mdl.device)
    got = (to64(mdl.evaluate_tensor(xt)) - to64(f.y_mean)) / to64(f.y_std)
    want = yn - to64(s.eps).T - to64(f.diag_add)[None, :] * to64(s.alpha).T
    return (got - want).abs().max().item()


def emulated_model_error():
    """(path error, identity error) of a float32 CPU Thompson model, the
    first against the float64 CPU model of the same archive, theta and seed."""
    m64 = _model("cpu", F64)
    m32 = _model("cpu", torch.float32)
    x = _model_queries()
    return (_model_error(m32.evaluate(x), m64.evaluate(x)),
            _model_identity_error(m32), _model_identity_error(m64))


def test_thompson_model_on_the_gpu(dev):
    m64 = _model("cpu", F64)
    mg = _model("cuda", torch.float32)
    x = _model_queries()
    v64 = m64.evaluate(x)
    assert (np.abs(v64).max(axis=0) >= 0.1).all()
    xt = torch.as_tensor(x, dtype=torch.float32, device=dev)
    vt = mg.evaluate_tensor(xt)
    assert vt.is_cuda and vt.shape == (33, 2) and vt.dtype == torch.float32
    # the draw is the CPU model's: same generator, same order; Omega and amp
    # see theta, which the GPU model holds in float32
    sg, s64 = mg._thompson_path.sample, m64._thompson_path.sample
    assert torch.equal(sg.tau.cpu(), s64.tau)
    for name in ("Omega", "amp"):
        assert torch.allclose(getattr(sg, name).cpu(), getattr(s64, name),
                              rtol=1e-6, atol=1e-9), name
    err = _model_error(vt.double().cpu().numpy(), v64)
    ident = _model_identity_error(mg)
    print(f"model path err {err:.3e}, identity {ident:.3e} (tol {MODEL_TOL:.3e})")
    assert err <= MODEL_TOL
    assert ident <= MODEL_TOL
    # evaluate() is the same path through the numpy entry; predict() stays
    # the posterior's, and the chunk driver is off in this mode
    assert _model_error(mg.evaluate(x), v64) <= MODEL_TOL
    assert np.abs(mg.evaluate(x) - mg.predict(x)[0]).max() > 1e-3
    assert mg.native_mean_args(dev) is None
    # the native call behind evaluate_tensor, bitwise
    from dmosopt_amd import _hipops

    s = mg._thompson_path.sample
    cache, _ = mg._native_pred_cache(dev)
    f = mg._fitted
    want = _hipops.gp_predict_path(
        xt, f.X, f.theta, s.alpha, f.y_mean, f.y_std, 2.5, False, s.Omega,
        s.tau, s.amp, cache[1], cache[2])
    assert torch.equal(vt, want)


# ---------------------------------------------------------- 8. short GPU run
def _zdt1(pp):
    x = np.array([pp[k] for k in sorted(pp.keys())])
    g = 1.0 + 9.0 * x[1:].mean()
    return np.array([x[0], g * (1.0 - np.sqrt(x[0] / g))])


def _run_zdt1(tag):
    import dmosopt_amd

    params = {
        "opt_id": tag,
        "obj_fun": _zdt1,
        "problem_parameters": {},
        "space": {f"x{i:02d}": [0.0, 1.0] for i in range(6)},
        "objective_names": ["f1", "f2"],
        "population_size": 40,
        "num_generations": 8,
        "n_initial": 3,
        "initial_maxiter": 2,
        "n_epochs": 2,
        "surrogate_method_name": "gpr",
        "surrogate_method_kwargs": {"anisotropic": False, "optimizer": "sceua",
                                    "thompson": True, "path_features": 256},
        "optimizer": "nsga2",
        "random_seed": 31,
    }
    assert dmosopt_amd.run(params, verbose=False) is not None
    x, y = dmosopt_amd.sopt_dict[tag].optimizer_dict[0].get_evals()
    return x.copy(), y.copy()


def test_thompson_run_on_the_gpu(dev):
    xa, ya = _run_zdt1("t_path_gpu_a")
    xb, yb = _run_zdt1("t_path_gpu_b")
    assert np.isfinite(xa).all() and np.isfinite(ya).all()
    assert xa.shape[0] > 18  # the initial design and a resample batch
    assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
