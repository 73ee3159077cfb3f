"""Mean-variance mode: one generation's surrogate evaluate, and the whole
inner loop, at bench.py's headline archive (N=300, d=30, 2 objectives) and
population (200).

(a) LEGACY: the branch engine._surrogate_eval had before the fused
    variance kernel — queries to the host, float64 numpy normalisation,
    H2D, torch cross kernel + bmm + the K^-1 variance chain, D2H,
    np.round. Replicated here from the torch pieces the package still has
    (FittedGP._finish_var), so both sides run in one process on one box.
(b) DEVICE: engine._surrogate_eval as it is now (one fused extension call,
    device tensor in, device tensor out).

Same box, warmup, alternating timed windows; the spread is printed with the
median. `--tree DIR` imports the package from another checkout (an older
commit measures only what it has: there (b) is absent and the loop runs
that commit's own branch). `--trace-only` runs just the (b) loop, for a
kernel trace taken in a run of its own.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--inner", type=int, default=100)
ap.add_argument("--gens", type=int, default=200)
ap.add_argument("--loops", type=int, default=5)
ap.add_argument("--trace-only", action="store_true")
args = ap.parse_args()

torch.set_num_threads(min(8, os.cpu_count() or 8))
sys.path.insert(0, args.tree)
import bench  # noqa: E402  (archive generator and headline sizes)
from dmosopt_amd.core import engine  # noqa: E402
from dmosopt_amd.models.gp_core import build_kernel  # noqa: E402
from dmosopt_amd.models.model import Model  # noqa: E402
from dmosopt_amd.moea.nsga2 import NSGA2Optimizer  # noqa: E402

assert torch.cuda.is_available(), "this benchmark measures the GPU"
dev = torch.device("cuda", 0)
D, M, POP = bench.D_IN, bench.N_OBJ, bench.POP_PER_GPU
lb, ub = np.zeros(D), np.ones(D)


def legacy_eval(mdl, x, optimize_mean_variance=True):
    gp = mdl.objective
    xin = np.asarray(engine._to_np(x), dtype=np.float64)
    xn = (xin - gp.xlb[None, :]) / gp.xrg[None, :]
    Xq = torch.as_tensor(xn, dtype=gp.dtype, device=gp.device)
    f = gp._fitted
    Ks = build_kernel(Xq, f.X, f.theta, nu=f.nu, anisotropic=f.anisotropic)
    mean_n = torch.bmm(Ks, f.alpha)[:, :, 0]
    mean, var = f._finish_var(Xq, Ks, mean_n)
    y_mean = mean.cpu().numpy().astype(np.float64)
    y_var = var.cpu().numpy().astype(np.float64)
    return np.column_stack((y_mean, np.round(y_var, 6)))


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def fit(seed):
    return engine.train(
        D, M, lb, ub, *bench.make_archive(seed), None,
        surrogate_method_name="gpr",
        surrogate_method_kwargs={"anisotropic": False, "optimizer": "sceua", "seed": seed},
        surrogate_return_mean_variance=True, logger=None, device=dev,
    )


X, Y = bench.make_archive(7)
gp = fit(7)
mdl = Model(return_mean_variance=True, objective=gp)
has_device = bool(getattr(gp, "supports_device_mean_variance", False))
x = torch.rand(POP, D, device=dev)


def loop(eval_fn, seed=11):
    """One inner loop in mean-variance mode, as engine.epoch sets it up."""
    opt = NSGA2Optimizer(
        popsize=POP, nInput=D, nOutput=M, model=mdl, optimize_mean_variance=True,
        distance_metric="crowding", sampling_method="slh", mutation_rate=None, nchildren=1,
    )
    opt.set_device(dev)
    saved = engine._surrogate_eval
    if eval_fn is not None:
        engine._surrogate_eval = eval_fn
    try:
        y0 = np.column_stack((Y, np.zeros_like(Y))).astype(np.float32)
        res = engine.optimize_loop(
            args.gens, opt, mdl, D, M, lb, ub, popsize=POP,
            initial=(X.astype(np.float32), y0),
            local_random=np.random.default_rng(seed), optimize_mean_variance=True,
        )
    finally:
        engine._surrogate_eval = saved
    torch.cuda.synchronize()
    return res


if args.trace_only:
    assert has_device, "--trace-only traces the device path"
    loop(None)
    sys.exit(0)

# ---- one generation's evaluate
paths = {"legacy": lambda: legacy_eval(mdl, x)}
if has_device:
    paths["device"] = lambda: engine._surrogate_eval(mdl, x, True)
for fn in paths.values():
    for _ in range(20):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in paths}
for _ in range(args.windows):
    for k, fn in paths.items():  # alternate the two inside every window
        t0 = time.perf_counter()
        for _ in range(args.inner):
            fn()
        torch.cuda.synchronize()
        times[k].append(1e6 * (time.perf_counter() - t0) / args.inner)
for k, ts in times.items():
    med, lo, hi = stats(ts)
    print(f"evaluate {k:7s}: median {med:8.1f} us/call  (min {lo:.1f}, max {hi:.1f}, "
          f"{args.windows} windows x {args.inner})")
if has_device:
    a, b = legacy_eval(mdl, x), engine._surrogate_eval(mdl, x, True).cpu().numpy()
    print(f"legacy vs device: max |mean diff| {np.abs(a[:, :M] - b[:, :M]).max():.3e}, "
          f"max |var diff| {np.abs(a[:, M:] - b[:, M:]).max():.3e}")

# ---- the whole inner loop
modes = {"legacy": legacy_eval} if has_device else {"own": None}
if has_device:
    modes["device"] = None
for fn in modes.values():
    loop(fn)  # warmup
ltimes = {k: [] for k in modes}
for _ in range(args.loops):
    for k, fn in modes.items():
        t0 = time.perf_counter()
        loop(fn)
        ltimes[k].append(1e3 * (time.perf_counter() - t0))
for k, ts in ltimes.items():
    med, lo, hi = stats(ts)
    print(f"optimize_loop {k:7s}: median {med:8.1f} ms / {args.gens} generations  "
          f"(min {lo:.1f}, max {hi:.1f}, {args.loops} runs)")

# ---- the fit (K^-1 is no longer built by it)
for s in (1, 2):
    fit(s)  # warmup, and the NMLL graph capture
fts = []
for s in (3, 4, 5, 3, 4, 5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit(s)
    torch.cuda.synchronize()
    fts.append(1e3 * (time.perf_counter() - t0))
print("GP fit (seeds 3,4,5 twice): " + " ".join(f"{t:.1f}" for t in fts) + " ms")
