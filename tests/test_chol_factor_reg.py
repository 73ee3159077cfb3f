"""Register-broadcast panel factor ("reg"): bitwise equality with the LDS
factor ("lds").

The reg factor moves pivots and multipliers through v_readlane, defers the
logdet term to one logf per lane and carries the rhs segment as row 32 of
the bordered diagonal block instead of solving it afterwards. Per element it
must run the lds factor's fmaf sequence, so L, logdet, info and z keep every
bit: SCE-UA accept decisions downstream are bit-sensitive. The explicit
factor= argument runs both factors inside one process; the env-selected
default is compared through fresh child processes (the switch is latched).
"""

import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N -> why the factor can go wrong there
SHAPES = {
    12: "a single partial panel: bs < 32 with the rhs lane",
    31: "a single partial panel one column short of full",
    32: "exactly one full panel",
    33: "a 1-column last panel",
    64: "exactly two panels",
    65: "two panels plus a 1-column panel",
    97: "a role-B tile beside the step panels",
    300: "the workload's own size, last panel bs = 12",
}
BATCHES = (1, 3, 18)
BMAX = max(BATCHES)
SCHEDULES = ("classic", "lookahead")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dmosopt_amd import ops

    assert ops.native_available(), "native extension must be built on a GPU box"
    return torch.device("cuda", 0)


def _spd_batch(N, B, dev, seed):
    """B Matern-5/2 kernel matrices of N random points in d=6, plus noise:
    per-matrix signal variance, length scale and noise level (the
    construction of test_chol_lookahead.py)."""
    from dmosopt_amd import _hipops

    g = torch.Generator().manual_seed(seed)
    X = torch.rand(N, 6, generator=g).float().to(dev)
    theta = torch.stack(
        [
            torch.rand(B, generator=g) - 0.5,                    # log sf2
            torch.rand(B, generator=g) * 1.5 - 1.0,              # log ell
            torch.full((B,), math.log(1e-3)),                    # log noise
        ],
        dim=1,
    ).float().to(dev)
    K = _hipops.matern_train(X, theta, 2.5, False, 1e-6)
    y = torch.randn(B, N, generator=g).float().to(dev)
    return K.contiguous(), y.contiguous()


_inputs: dict = {}


def _inputs_for(N, dev):
    """One (K, y) batch of BMAX matrices per N, built once and never
    written: the factor binding clones its inputs."""
    if N not in _inputs:
        _inputs[N] = _spd_batch(N, BMAX, dev, seed=2000 + N)
    return _inputs[N]


def _both(K, y, schedule):
    from dmosopt_amd import ops

    a = ops.chol_factor_multik(K, y, schedule=schedule, factor="lds")
    b = ops.chol_factor_multik(K, y, schedule=schedule, factor="reg")
    return a, b


def _assert_same(a, b, rows=None):
    La, lda, ia, za = a
    Lb, ldb, ib, zb = b
    sel = slice(None) if rows is None else rows
    assert torch.equal(ia, ib), (ia.tolist(), ib.tolist())
    assert torch.equal(La[sel].tril(), Lb[sel].tril())
    assert torch.equal(lda[sel], ldb[sel])
    if za is None:
        assert zb is None
    else:
        assert torch.equal(za[sel], zb[sel])


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("with_rhs", [False, True], ids=["norhs", "rhs"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", sorted(SHAPES))
def test_reg_bitwise_equals_lds(dev, N, B, with_rhs, schedule):
    K, y = _inputs_for(N, dev)
    K, y = K[:B].contiguous(), y[:B].contiguous()
    a, b = _both(K, y if with_rhs else None, schedule)
    assert (a[2] == 0).all(), f"lds failed on an SPD input: {a[2].tolist()}"
    assert torch.isfinite(a[1]).all()
    _assert_same(a, b)


@pytest.mark.parametrize("N", sorted(SHAPES))
def test_reg_factor_and_solve_against_float64(dev, N):
    """Independent of the lds path's bits: the reg factor is a real factor
    (backward error within test_chol_lookahead.py's bound: fp32 error
    ~ N * eps * max|K| = 300 * 6e-8 * 1.7 ~ 3e-5, bound 1e-3) and its z is
    the float64 forward solve to the accuracy the lds path reaches on the
    same inputs, times 2."""
    K, y = _inputs_for(N, dev)
    a, b = _both(K, y, "lookahead")
    Kd = K.double()
    Lr = b[0].tril().double()
    err = (Lr @ Lr.transpose(1, 2) - Kd).abs().max()
    assert err < 1e-3, float(err)
    L64 = torch.linalg.cholesky(Kd)
    z64 = torch.linalg.solve_triangular(
        L64, y.double().unsqueeze(-1), upper=False).squeeze(-1)
    err_lds = float((a[3].double() - z64).abs().max())
    err_reg = float((b[3].double() - z64).abs().max())
    scale = float(z64.abs().max())
    assert err_reg <= 2.0 * err_lds, (
        f"N={N}: max|z - z64| reg {err_reg:.3e}, lds {err_lds:.3e} "
        f"(bound 2 x lds), max|z64| {scale:.3e}")


# N = 75: panels [0, 32), [32, 64) and a partial last panel [64, 75)
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize(
    "col", [0, 40, 70],
    ids=["column0", "mid-second-panel", "last-partial-panel"])
def test_reg_same_failure_reporting(dev, col, schedule):
    """One matrix of the batch has a negative diagonal entry: info (first
    failing column, 1-based) is identical between the factors and the other
    matrices stay bitwise equal."""
    K, y = _spd_batch(75, 3, dev, seed=75)
    K = K.clone()
    K[1, col, col] = -1.0
    a, b = _both(K, y, schedule)
    assert a[2][0] == 0 and a[2][2] == 0
    assert a[2][1] == col + 1, a[2].tolist()
    assert b[2][1] == col + 1, b[2].tolist()
    _assert_same(a, b, rows=[0, 2])


_NMLL_CHILD = r"""
import math, sys, torch
from dmosopt_amd import _hipops
dev = torch.device("cuda", 0)
out = {}
for N in (97, 300):
    g = torch.Generator().manual_seed(7000 + N)
    B = 18
    X = torch.rand(N, 30, generator=g).float().to(dev)
    theta = torch.stack([torch.rand(B, generator=g) - 0.5,
                         torch.rand(B, generator=g) * 1.5 - 1.0,
                         torch.full((B,), math.log(1e-3))], dim=1).float().to(dev)
    y = torch.randn(B, N, generator=g).float().to(dev)
    out[N] = _hipops.gp_nmll(X.contiguous(), theta.contiguous(), y.contiguous(),
                             2.5, False, 1e-6).cpu()
torch.save(out, sys.argv[1])
"""


def test_gp_nmll_bitwise_across_factors(dev, tmp_path):
    """Fused NMLL (per-row y, B = 18) on the default route under
    DMOSOPT_CHOL_FACTOR=lds and =reg, each in a fresh child process: the
    switch is latched per process."""
    outs = {}
    for flag in ("lds", "reg"):
        path = tmp_path / f"nmll_{flag}.pt"
        env = dict(os.environ)
        env["DMOSOPT_CHOL_FACTOR"] = flag
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        subprocess.run([sys.executable, "-c", _NMLL_CHILD, str(path)],
                       check=True, env=env, cwd=ROOT, timeout=300)
        outs[flag] = torch.load(path)
    for N in (97, 300):
        assert torch.isfinite(outs["lds"][N]).all()
        assert torch.equal(outs["lds"][N], outs["reg"][N]), N
