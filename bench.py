"""Flagship benchmark: MO-ASMO epoch time (GP fit + 200-gen NSGA2), ZDT1 d=30.

Measures BASELINE.json's headline metric on its named config: one timed
"step" = one full MO-ASMO epoch — GP surrogate fit (Matern-5/2, SCE-UA
batched MLL search) on a fixed 300-point archive + 200 NSGA-II generations
against the surrogate + resample selection + real (synthetic, on-device)
ZDT1 evaluation of the resample batch. Weak scaling: per-GPU population is
fixed at 200, global population = 200 * n_gpus; every rank runs the
replicated NSGA2 control flow (identical seeds) while surrogate prediction
is rank-sharded and all-gathered over RCCL/xGMI each generation.

Run: python bench.py [--gpus N] [--steps K] [--warmup W]
Distributed: torchrun --nnodes=1 --nproc-per-node N bench.py --gpus N ...

A plain run only sets up, warms up, times the K steps and prints the JSON
result line. --dump-outputs DIR additionally writes what the last timed
step returned (x_res, y_res, hv) as DIR/<name>.npy; the inputs are seeded,
so two builds can be compared output for output. Everything else the
benchmark measures (the bf16-vs-fp32 accuracy block of --dtype bf16) runs
only with --full.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

# host-side control code thrashes with one thread per core on many-core
# GPU boxes (small CPU tensor ops); the compute path is the GPU anyway.
# Divide by the local world size: N co-located ranks each spinning 8 OMP
# threads oversubscribe small hosts 16x (measured on an 8-core box).
_local_world = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
torch.set_num_threads(max(1, min(8, (os.cpu_count() or 8) // max(1, _local_world))))

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dmosopt_amd.benchmarks.problems import zdt1
from dmosopt_amd.core import engine
from dmosopt_amd.hv.exact import hv_2d
from dmosopt_amd.models.model import Model
from dmosopt_amd.parallel import comm

D_IN = 30
N_OBJ = 2
POP_PER_GPU = 200
N_GEN = 200
ARCHIVE_N = 300


def make_archive(seed: int) -> tuple:
    rng = np.random.default_rng(seed)
    X = rng.random((ARCHIVE_N, D_IN))
    Y = zdt1(X).numpy()
    return X, Y


def one_epoch(X, Y, pop, rank, world, device, seed, n_gen=N_GEN, compute="fp32"):
    """One MO-ASMO epoch; returns (resample_x, predicted_y, hv).

    Multi-rank path = the PACKAGE path: rank 0 fits the GP and broadcasts
    theta (engine.train), predictions are rank-sharded and all-gathered
    each generation (parallel.sharded.ShardedObjective). compute="bf16"
    runs the posterior path (cross kernel + Cholesky trailing updates) on
    the bf16 matrix units; the SCE-UA hyperparameter search stays fp32, so
    theta is identical between the two modes."""
    gp = engine.train(
        D_IN, N_OBJ, np.zeros(D_IN), np.ones(D_IN), X, Y, None,
        surrogate_method_name="gpr",
        surrogate_method_kwargs={
            "anisotropic": False, "optimizer": "sceua", "seed": seed,
            "compute": compute,
        },
        logger=None, device=device,
    )
    if world > 1:
        from dmosopt_amd.parallel.context import get_context
        from dmosopt_amd.parallel.sharded import ShardedObjective

        mdl = Model(objective=ShardedObjective(gp, get_context()))
    else:
        mdl = Model(objective=gp)

    from dmosopt_amd.moea.nsga2 import NSGA2Optimizer

    optimizer = NSGA2Optimizer(
        popsize=pop, nInput=D_IN, nOutput=N_OBJ, model=mdl,
        distance_metric="crowding", sampling_method="slh", mutation_rate=None, nchildren=1,
    )
    if device.type == "cuda":
        optimizer.set_device(device)
    local_random = np.random.default_rng(seed + 1)
    res = engine.optimize_loop(
        n_gen, optimizer, mdl, D_IN, N_OBJ, np.zeros(D_IN), np.ones(D_IN),
        popsize=pop, initial=(X.astype(np.float32), Y.astype(np.float32)),
        local_random=local_random,
    )
    # resample selection (25% of pop) + real evaluation of the batch
    from dmosopt_amd import ops

    best_x = torch.as_tensor(res.best_x, dtype=torch.float32, device=device)
    best_y = torch.as_tensor(res.best_y, dtype=torch.float32, device=device)
    Dc = ops.crowding_distance(best_y)
    n_res = max(1, int(0.25 * pop))
    idx = torch.argsort(Dc, descending=True)[:n_res]
    x_res = best_x[idx]
    y_res = zdt1(x_res.double())  # on-device synthetic objective evaluation
    # final hypervolume of the REAL-evaluated resample batch (the quality
    # half of the headline metric); device-resident fronts stay on device
    if y_res.is_cuda:
        hv = hv_2d(y_res, np.array([11.0, 11.0]))
    else:
        hv = hv_2d(y_res.cpu().numpy(), np.array([11.0, 11.0]))
    return x_res, y_res, hv


def dump_outputs(out_dir, x_res, y_res, hv):
    """Write one_epoch's return values as <out_dir>/<name>.npy (float32 /
    float64, a few KB): the resample batch, its real objective values and
    the batch's hypervolume."""
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "x_res.npy"),
            x_res.detach().cpu().numpy().astype(np.float32))
    np.save(os.path.join(out_dir, "y_res.npy"),
            y_res.detach().cpu().numpy().astype(np.float64))
    np.save(os.path.join(out_dir, "hv.npy"), np.asarray([float(hv)], dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gens", type=int, default=N_GEN)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--pop-per-gpu", type=int, default=POP_PER_GPU,
                    help="diagnostic override of the per-GPU population")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the untimed extras (bf16 accuracy delta "
                         "vs fp32 with --dtype bf16)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    compute = "bf16" if args.dtype == "bf16" else "fp32"

    rank, world = comm.init_from_env()
    if torch.cuda.is_available():
        device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)) % torch.cuda.device_count())
        torch.cuda.set_device(device)
    else:
        device = torch.device("cpu")

    pop = args.pop_per_gpu * world  # weak scaling: global population grows
    X, Y = make_archive(seed=1234)

    import torch.distributed as dist

    def barrier_sync():
        if world > 1:
            dist.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize()

    x_res = y_res = hv = None
    for w in range(args.warmup):
        one_epoch(X, Y, pop, rank, world, device, seed=100 + w, n_gen=args.gens,
                  compute=compute)

    barrier_sync()
    t0 = time.perf_counter()
    for s in range(args.steps):
        x_res, y_res, hv = one_epoch(X, Y, pop, rank, world, device, seed=200 + s,
                                     n_gen=args.gens, compute=compute)
    barrier_sync()
    t1 = time.perf_counter()

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, x_res, y_res, hv)

    accuracy = None
    if args.full and compute == "bf16" and rank == 0 and device.type == "cuda":
        # untimed accuracy delta vs fp32: same seed => identical theta (the
        # search is fp32 in both modes), so the delta isolates the bf16
        # posterior path (cross kernel + Cholesky trailing updates)
        gp32 = engine.train(
            D_IN, N_OBJ, np.zeros(D_IN), np.ones(D_IN), X, Y, None,
            surrogate_method_name="gpr",
            surrogate_method_kwargs={"anisotropic": False, "optimizer": "sceua",
                                     "seed": 200, "compute": "fp32"},
            logger=None, device=device)
        gp16 = engine.train(
            D_IN, N_OBJ, np.zeros(D_IN), np.ones(D_IN), X, Y, None,
            surrogate_method_name="gpr",
            surrogate_method_kwargs={"anisotropic": False, "optimizer": "sceua",
                                     "seed": 200, "compute": "bf16"},
            logger=None, device=device)
        probe = np.random.default_rng(0).random((2048, D_IN))
        m32, _ = gp32.predict(probe)
        m16, _ = gp16.predict(probe)
        scale = np.abs(m32).mean()
        _, _, hv32 = one_epoch(X, Y, pop, rank, world, device, seed=200,
                               n_gen=args.gens, compute="fp32")
        accuracy = {
            "posterior_mean_abs_err_max": float(np.abs(m16 - m32).max()),
            "posterior_mean_abs_err_mean": float(np.abs(m16 - m32).mean()),
            "posterior_mean_rel_err_mean": float(np.abs(m16 - m32).mean() / scale),
            "final_hv_fp32": float(hv32),
            "final_hv_bf16": float(hv),
            "hv_rel_delta": float(abs(hv - hv32) / max(abs(hv32), 1e-12)),
        }

    elapsed = t1 - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        if device.type == "cuda":
            t = t.to(device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    ms_per_step = 1000.0 * elapsed / args.steps
    if rank == 0:
        out = {
            "metric": "MO-ASMO epoch time (GP fit + 200-gen NSGA2), ZDT1 d=30",
            "value": ms_per_step,
            "unit": "ms_per_epoch",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": False,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic ZDT1 d=30, random-init archive of 300 evals",
            "config": {
                "model": "GPR-Matern52 surrogate + NSGA2",
                "global_batch": pop,
                "seq_len": None,
                "parallelism": f"replicated-moea+sharded-gp dp{world}",
                "population_size": pop,
                "num_generations": args.gens,
                "archive_size": ARCHIVE_N,
                "final_hypervolume_ref11": hv,
                "reference_measured_ms_per_epoch_cpu": 19200.0,
                "bf16_accuracy_vs_fp32": accuracy,
            },
        }
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
