"""One-launch Cholesky schedule: bitwise equality with the look-ahead schedule.

The one-launch kernel (one workgroup per matrix for the whole factorization)
must reproduce the look-ahead schedule bit for bit: SCE-UA accept decisions
downstream are bit-sensitive. The explicit-schedule binding runs both
schedules inside one process; the env-selected default is compared through
fresh child processes (DMOSOPT_CHOL_ONELAUNCH is latched).
"""

import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N -> why the kernel can go wrong there. Its constants that split work:
# 16x16 tiles, 15 worker waves, 4 tiles in flight per worker, 64-lane waves
# in the TRSM / writeback split, 64-row rhs groups.
SHAPES = {
    33: "a 1-column last panel, no tiles",
    64: "exactly two panels",
    65: "one row below the diagonal block; a 1-column strip",
    96: "the first trailing tiles; strip 0 is exactly one wave of TRSM rows",
    97: "a one-row tile; strip 0 is one wave of TRSM rows plus one row; "
        "12 tiles at step 1, fewer than the 15 workers",
    129: "the last strip is one column; 25 tiles at step 1, more than the "
         "workers, at most 2 per worker (under the batch of 4)",
    161: "42 tiles at step 1",
    257: "117 tiles at step 1: 7 or 8 per worker, two batches of 4",
    300: "the workload's own size",
}
BATCHES = (1, 3, 18)
BMAX = max(BATCHES)

# largest N whose LDS need fits the 160 KiB of a CU: the S block (33 x 33),
# the staged next diagonal block (32 x 33), two 32-float segments, 256 NMLL
# partials and two panel buffers of (N - 32) x 33 floats:
# 4 * (1089 + 1056 + 64 + 256 + 66 * (N - 32)) <= 163840
N_LDS_MAX = 615


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

    a = ops.chol_factor_multik(K, y, schedule="lookahead")
    b = ops.chol_factor_multik(K, y, schedule="onelaunch")
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
def test_onelaunch_bitwise_equals_lookahead(dev, N, B, with_rhs):
    K, y = _inputs_for(N, dev)
    K, y = K[:B].contiguous(), y[:B].contiguous()
    a, b = _both(K, y if with_rhs else None)
    assert (a[2] == 0).all(), f"look-ahead failed on an SPD input: {a[2].tolist()}"
    # the factor is a real factor, not merely equal garbage: fp32 backward
    # error ~ N * eps * max|K| = 300 * 6e-8 * 1.7 ~ 3e-5, bound 1e-3
    L = b[0].tril().double()
    err = (L @ L.transpose(1, 2) - K.double()).abs().max()
    assert err < 1e-3, float(err)
    _assert_same(a, b)


def test_onelaunch_same_failure_reporting(dev):
    """One matrix of the batch is not positive definite (negative pivot in
    the second panel): info is [0, 41, 0] in both schedules and the other
    matrices stay bitwise equal."""
    K, y = _inputs_for(97, dev)
    K, y = K[:3].clone(), y[:3].contiguous()
    K[1, 40, 40] = -1.0
    a, b = _both(K, y)
    assert a[2].tolist() == [0, 41, 0], a[2].tolist()  # 1-based failing column
    assert b[2].tolist() == [0, 41, 0], b[2].tolist()
    _assert_same(a, b, rows=[0, 2])


@pytest.mark.parametrize("N", [N_LDS_MAX, N_LDS_MAX + 1],
                         ids=["largest_admitted", "one_above"])
def test_onelaunch_route_bound(dev, N):
    """B = 1 at the largest N the LDS bound admits, and at one above it,
    where the request runs through the look-ahead schedule."""
    K, y = _spd_batch(N, 1, dev, seed=N)
    a, b = _both(K, y)
    assert (a[2] == 0).all()
    _assert_same(a, b)


_NMLL_CHILD = r"""
import math, sys, torch
from dmosopt_amd import _hipops, ops
assert ops.native_available()
dev = torch.device("cuda", 0)
out = {}
for N in (97, 300):
    g = torch.Generator().manual_seed(7000 + N)
    B = 18
    X = torch.rand(N, 30, generator=g).float().to(dev).contiguous()
    theta = torch.stack([torch.rand(B, generator=g) - 0.5,
                         torch.rand(B, generator=g) * 1.5 - 1.0,
                         torch.full((B,), math.log(1e-3))], dim=1).float().to(dev).contiguous()
    y = torch.randn(B, N, generator=g).float().to(dev).contiguous()
    out[N] = _hipops.gp_nmll(X, theta, y, 2.5, False, 1e-6).cpu()
    # the same value through the chain that ends in the NMLL epilogue
    f32 = dict(dtype=torch.float32, device=dev)
    K, Z = torch.empty(B, N, N, **f32), torch.empty(B, N, **f32)
    logdet, o = torch.empty(B, **f32), torch.empty(B, **f32)
    info = torch.empty(B, dtype=torch.int32, device=dev)
    ops.gp_nmll_into(X, theta, y, K, Z, logdet, info, o, 2.5, False, 1e-6)
    out[(N, "into")] = o.cpu()
torch.save(out, sys.argv[1])
"""


def _children(script, tmp_path, name):
    outs = {}
    for flag in ("0", "1"):
        path = tmp_path / f"{name}_{flag}.pt"
        env = dict(os.environ)
        env["DMOSOPT_CHOL_ONELAUNCH"] = flag
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        subprocess.run([sys.executable, "-c", script, str(path)],
                       check=True, env=env, cwd=ROOT, timeout=300)
        outs[flag] = torch.load(path, weights_only=False)
    return outs


def test_gp_nmll_bitwise_across_switch(dev, tmp_path):
    """Fused NMLL (per-row y, B = 18) under DMOSOPT_CHOL_ONELAUNCH=0 and =1,
    each in a fresh child process: the switch is latched per process."""
    outs = _children(_NMLL_CHILD, tmp_path, "nmll")
    for N in (97, 300):
        assert torch.isfinite(outs["0"][N]).all()
        assert torch.equal(outs["0"][N], outs["1"][N]), N
        for flag in ("0", "1"):
            assert torch.equal(outs[flag][N], outs[flag][(N, "into")]), (N, flag)


_FIT_CHILD = r"""
import sys
import numpy as np
import torch
from bench import make_archive
from dmosopt_amd.core import engine
from dmosopt_amd.models import gp
dev = torch.device("cuda", 0)
X, Y = make_archive(seed=7)
X, Y = X[:120], Y[:120]
got = []
real = gp.sceua_batched
def spy(*a, **k):
    r = real(*a, **k)
    got.append(r)
    return r
gp.sceua_batched = spy
out = {}
for seed in (0, 1, 2):
    del got[:]
    m = engine.train(
        X.shape[1], Y.shape[1], np.zeros(X.shape[1]), np.ones(X.shape[1]), X, Y,
        None, surrogate_method_name="gpr",
        surrogate_method_kwargs={"anisotropic": False, "optimizer": "sceua",
                                 "seed": seed},
        logger=None, device=dev)
    assert len(got) >= 1
    host = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    out[seed] = dict(theta=host(m.theta),
                     bestf=[host(g[1]) for g in got],
                     icall=[host(g[2]) for g in got])
torch.save(out, sys.argv[1])
"""


def test_fit_end_to_end_across_switch(dev, tmp_path):
    """engine.train on a 120-row cut of the bench archive, seeds 0..2, under
    both switch values: theta, the SCE-UA call count and the best f are
    identical."""
    import numpy as np

    outs = _children(_FIT_CHILD, tmp_path, "fit")
    for seed in (0, 1, 2):
        a, b = outs["0"][seed], outs["1"][seed]
        assert np.array_equal(a["theta"], b["theta"]), seed
        assert len(a["icall"]) == len(b["icall"])
        for u, v in zip(a["icall"] + a["bestf"], b["icall"] + b["bestf"]):
            assert np.array_equal(u, v), seed
        assert all(np.isfinite(f).all() for f in a["bestf"])
        assert all((np.asarray(c) > 0).all() for c in a["icall"])


def test_nmll_graph_replay_is_deterministic(dev):
    """50 replays of the captured NMLL pipeline on fixed inputs give identical
    bytes each time (a captured node that races on replay shows here)."""
    from dmosopt_amd.models import gp_core

    g = torch.Generator().manual_seed(11)
    N, B = 300, 18
    X = torch.rand(N, 30, generator=g).float().to(dev)
    y = torch.randn(B, N, generator=g).float().to(dev)
    theta = torch.stack([torch.rand(B, generator=g) - 0.5,
                         torch.rand(B, generator=g) * 1.5 - 1.0,
                         torch.full((B,), math.log(1e-3))], dim=1).float().to(dev)
    graph = gp_core._NmllGraph(X, y, theta, 2.5, False, 1e-6)
    first = graph.run(X, y, theta)
    assert torch.isfinite(first).all()
    for _ in range(50):
        assert torch.equal(graph.run(X, y, theta), first)
