"""optimizer="grad" against optimizer="sceua": fit wall time and fit quality
at bench.py's headline archive (N=300, d=30, 2 objectives), isotropic and
ARD, and the per-call cost of gp_nmll_grad against gp_nmll at B=16.

Same box, one process, warmed up (the first fit of each kind also captures
the NMLL graph / loads the kernels), the kinds alternate inside every round;
the spread is printed with the median. NMLL of each fitted theta is
re-evaluated in float64 on the CPU.

optimizer="adam" is NOT timed here: at N=300 its torch.linalg.cholesky_ex
call is the rocSOLVER batched f32 path that README.md records as raising
hipErrorLaunchFailure at this size.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=200)
args = ap.parse_args()

torch.set_num_threads(min(8, os.cpu_count() or 8))
sys.path.insert(0, args.tree)
import bench  # noqa: E402  (archive generator and headline sizes)
from dmosopt_amd import _hipops  # noqa: E402
from dmosopt_amd.models.gp import GPRMatern  # noqa: E402
from dmosopt_amd.models.gp_core import batched_nmll  # noqa: E402

assert torch.cuda.is_available(), "this benchmark measures the GPU"
dev = torch.device("cuda", 0)
D, M = bench.D_IN, bench.N_OBJ
lb, ub = np.zeros(D), np.ones(D)
X, Y = bench.make_archive(7)


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fit(optimizer, aniso, seed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = GPRMatern(X, Y, D, M, lb, ub, optimizer=optimizer, anisotropic=aniso,
                  seed=seed, device=dev)
    torch.cuda.synchronize()
    return m, 1e3 * (time.perf_counter() - t0)


def nmll64(m):
    Xn = ((np.asarray(X, dtype=np.float64) - lb) / (ub - lb)).astype(np.float32)
    X64 = torch.as_tensor(Xn).double()
    Y64 = torch.as_tensor(np.asarray(Y, dtype=np.float64)).float().double()
    Yn = (Y64 - Y64.mean(0)) / Y64.std(0, unbiased=False)
    return batched_nmll(X64, Yn.T.contiguous(), m.theta.double().cpu(),
                        nu=m.nu, anisotropic=m.anisotropic).tolist()


for aniso in (False, True):
    kinds = ("grad", "sceua")
    for k in kinds:
        fit(k, aniso, 1)  # warmup
    times = {k: [] for k in kinds}
    last = {}
    for r in range(args.rounds):
        for k in kinds:
            last[k], t = fit(k, aniso, 3 + r)
            times[k].append(t)
    for k in kinds:
        med, lo, hi = stats(times[k])
        print(f"fit {'ARD' if aniso else 'iso'} {k:5s}: median {med:8.1f} ms "
              f"(min {lo:.1f}, max {hi:.1f}, {args.rounds} fits); float64 NMLL "
              f"of the last fit {['%.2f' % v for v in nmll64(last[k])]}")

# ---- per call: what the K^-1 solves and the gradient kernels add
N, B = X.shape[0], 16
g = torch.Generator().manual_seed(0)
Xd = torch.as_tensor(np.asarray(X, dtype=np.float32), device=dev)
Yd = torch.as_tensor(np.asarray(Y, dtype=np.float32), device=dev)
Yn = ((Yd - Yd.mean(0)) / Yd.std(0, unbiased=False)).T.contiguous().repeat(B // M, 1)
for aniso in (False, True):
    n_ell = D if aniso else 1
    theta = torch.cat([
        torch.zeros(B, 1), torch.log(0.5 * (0.7 + 0.7 * torch.rand(B, n_ell, generator=g))),
        torch.full((B, 1), float(np.log(1e-3))),
    ], dim=1).float().to(dev)
    paths = {
        "gp_nmll": lambda: _hipops.gp_nmll(Xd, theta, Yn, 2.5, aniso, 1e-6),
        "gp_nmll_grad": lambda: _hipops.gp_nmll_grad(Xd, theta, Yn, 2.5, aniso, 1e-6),
    }
    for fn in paths.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(5):
        for k, fn in paths.items():
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            times[k].append(1e6 * (time.perf_counter() - t0) / args.calls)
    for k, ts in times.items():
        med, lo, hi = stats(ts)
        print(f"per call {'ARD' if aniso else 'iso'} B={B} N={N} {k:12s}: median "
              f"{med:8.1f} us (min {lo:.1f}, max {hi:.1f}, 5 windows x {args.calls})")
