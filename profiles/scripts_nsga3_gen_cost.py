"""ms per generation of the nsga3 survival next to nsga2 (DTLZ2, 3 objectives,
d = 7, pop 200) and next to age at the config-3 shape (ZDT3, d = 30, pop 1024),
surrogate-free: the optimizer API driven directly, the problem evaluated on
the device. (loop at G2 generations - loop at G1) / (G2 - G1), same seeds,
the optimizers alternating, one warm-up per shape, every loop ends in a
device synchronise. Results: profiles/README.md, "NSGA-III".

  python profiles/scripts_nsga3_gen_cost.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmosopt_amd.benchmarks import problems as bp  # noqa: E402
from dmosopt_amd.config import optimizer_registry, resolve  # noqa: E402

REPS = int(os.environ.get("NSGA3_REPS", 5))
SCALE = float(os.environ.get("NSGA3_GEN_SCALE", 1.0))  # < 1: a rehearsal
dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
if os.environ.get("NSGA3_REQUIRE_GPU", "1") == "1":
    assert dev.type == "cuda", "this measurement needs the GPU"

# name -> (optimizers, pop, d, m, problem, G1, G2)
SHAPES = {
    "dtlz2_m3_pop200": (("nsga2", "nsga3"), 200, 7, 3, lambda x: bp.dtlz2(x, 3), 50, 450),
    "zdt3_pop1024": (("age", "nsga2", "nsga3"), 1024, 30, 2, bp.zdt3, 10, 60),
}


def loop(name, pop, d, m, fn, gens, seed):
    opt = resolve(optimizer_registry, name)(popsize=pop, nInput=d, nOutput=m)
    opt.set_device(dev)
    bounds = np.column_stack([np.zeros(d), np.ones(d)])
    rng = np.random.default_rng(seed)
    x = opt.generate_initial(bounds, rng)
    y = fn(torch.as_tensor(x, dtype=torch.float32, device=dev))
    opt.initialize_strategy(x, y.cpu().numpy(), bounds, rng)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(gens):
        xg, gs = opt.generate()
        opt.update(xg, fn(xg), gs)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


out = {"reps": REPS, "device": str(dev)}
for shape, (names, pop, d, m, fn, g1, g2) in SHAPES.items():
    g1, g2 = max(1, int(g1 * SCALE)), max(2, int(g2 * SCALE))
    for name in names:
        loop(name, pop, d, m, fn, g1, 100)
    per_gen = {name: [] for name in names}
    for r in range(REPS):
        for name in names:
            a = loop(name, pop, d, m, fn, g1, 200 + r)
            b = loop(name, pop, d, m, fn, g2, 200 + r)
            per_gen[name].append((b - a) / (g2 - g1))
    out[shape] = {"pop": pop, "d": d, "m": m, "g1": g1, "g2": g2}
    for name, v in per_gen.items():
        s = sorted(v)
        out[shape][name] = {"ms_per_gen_median": s[len(s) // 2], "min": s[0], "max": s[-1],
                            "all": v}
        print(shape, name, f"{s[len(s) // 2]:.3f} ms/gen ({s[0]:.3f} .. {s[-1]:.3f})", flush=True)
if len(sys.argv) > 1:  # optional: keep every figure as JSON
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
