"""Look-ahead Cholesky schedule: bitwise equality with the classic schedule.

The look-ahead schedule (one step launch per panel, trailing update beside
the next panel) must reproduce the classic panel + SYRK schedule bit for
bit — SCE-UA accept decisions downstream are bit-sensitive. The explicit-
schedule binding runs both schedules inside one process; the env-selected
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

# N -> why the schedule can go wrong there
SHAPES = {
    33: "one full panel plus a 1-column panel, no tiles",
    64: "exactly two panels",
    65: "step-1 strip has one row below its diagonal block; step-2 strip is one column",
    96: "step 1 is the first step with a role-B tile",
    97: "that tile plus a one-row tile",
    129: "last strip is one column",
    300: "the workload's own size",
}
BATCHES = (1, 3, 18)
BMAX = max(BATCHES)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dmosopt_amd import ops

    assert ops.native_available(), "native extension must be built on a GPU box"
    return torch.device("cuda", 0)


def _spd_batch(N, B, dev, seed):
    """B Matern-5/2 kernel matrices of N random points in d=6, plus noise:
    per-matrix signal variance, length scale and noise level."""
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
        _inputs[N] = _spd_batch(N, BMAX, dev, seed=1000 + N)
    return _inputs[N]


def _both(K, y):
    from dmosopt_amd import ops

    a = ops.chol_factor_multik(K, y, schedule="classic")
    b = ops.chol_factor_multik(K, y, schedule="lookahead")
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


@pytest.mark.parametrize("with_rhs", [False, True], ids=["norhs", "rhs"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", sorted(SHAPES))
def test_lookahead_bitwise_equals_classic(dev, N, B, with_rhs):
    K, y = _inputs_for(N, dev)
    K, y = K[:B].contiguous(), y[:B].contiguous()
    a, b = _both(K, y if with_rhs else None)
    assert (a[2] == 0).all(), f"classic failed on an SPD input: {a[2].tolist()}"
    # the factor is a real factor, not merely equal garbage: fp32 backward
    # error ~ N * eps * max|K| = 300 * 6e-8 * 1.7 ~ 3e-5, bound 1e-3
    L = a[0].tril().double()
    err = (L @ L.transpose(1, 2) - K.double()).abs().max()
    assert err < 1e-3, float(err)
    _assert_same(a, b)


@pytest.mark.parametrize("with_rhs", [False, True], ids=["norhs", "rhs"])
def test_lookahead_multi_chunk_panel(dev, with_rhs):
    """N = 481: step 1 has 417 rows below its diagonal block, more than one
    384-row TRSM chunk, so the strip update of a LATER chunk runs too."""
    K, y = _spd_batch(481, 3, dev, seed=481)
    a, b = _both(K, y if with_rhs else None)
    assert (a[2] == 0).all()
    _assert_same(a, b)


def test_lookahead_same_failure_reporting(dev):
    """One matrix of the batch is not positive definite (negative pivot in
    the second panel): info is identical between schedules and the other
    matrices stay bitwise equal."""
    K, y = _inputs_for(97, dev)
    K, y = K[:3].clone(), y[:3].contiguous()
    K[1, 40, 40] = -1.0
    a, b = _both(K, y)
    assert a[2][0] == 0 and a[2][2] == 0
    assert a[2][1] == 41, a[2].tolist()  # 1-based failing column
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


def test_gp_nmll_bitwise_across_schedules(dev, tmp_path):
    """Fused NMLL (per-row y, B = 18) under DMOSOPT_CHOL_LOOKAHEAD=0 and =1,
    each in a fresh child process: the switch is latched per process."""
    outs = {}
    for flag in ("0", "1"):
        path = tmp_path / f"nmll_{flag}.pt"
        env = dict(os.environ)
        env["DMOSOPT_CHOL_LOOKAHEAD"] = flag
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        subprocess.run([sys.executable, "-c", _NMLL_CHILD, str(path)],
                       check=True, env=env, cwd=ROOT, timeout=300)
        outs[flag] = torch.load(path)
    for N in (97, 300):
        assert torch.isfinite(outs["0"][N]).all()
        assert torch.equal(outs["0"][N], outs["1"][N]), N


def test_nmll_graph_static_binding(dev):
    """The NMLL graph skips the X / y input copies only while the bound
    source tensor is untouched: a new tensor or an in-place write rebinds."""
    from dmosopt_amd.models import gp_core

    if not gp_core._nmll_graph_enabled():
        pytest.skip("NMLL graph disabled by environment")
    g = torch.Generator().manual_seed(5)
    N, B = 97, 6
    X = torch.rand(N, 5, generator=g).float().to(dev)
    y = torch.randn(B, N, generator=g).float().to(dev)
    theta = torch.stack([torch.zeros(B), torch.rand(B, generator=g) - 0.5,
                         torch.full((B,), -3.0)], dim=1).float().to(dev)

    def eager(yy):
        from dmosopt_amd import ops

        out = ops.gp_nmll_fused(X, theta, yy, 2.5, False, 1e-6)
        return torch.where(torch.isfinite(out), out, torch.full_like(out, float("inf")))

    kw = dict(nu=2.5, anisotropic=False, jitter=1e-6)
    r1 = gp_core.batched_nmll(X, y, theta, **kw)
    r2 = gp_core.batched_nmll(X, y, theta, **kw)       # bound: copies skipped
    assert torch.equal(r1, eager(y)) and torch.equal(r2, r1)
    y.mul_(0.5)                                         # in-place write
    r3 = gp_core.batched_nmll(X, y, theta, **kw)
    assert torch.equal(r3, eager(y)) and not torch.equal(r3, r1)
    y2 = y * 3.0                                        # another tensor
    r4 = gp_core.batched_nmll(X, y2, theta, **kw)
    assert torch.equal(r4, eager(y2))
