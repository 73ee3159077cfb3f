"""ms per generation of TNK + CMA-ES pop 4096 (config-5 shape) with the
logreg and the gp feasibility model: (epoch at G2 gens - epoch at G1 gens) /
(G2 - G1), same seeds, alternating the two models, one warm-up per shape.
Results: profiles/README.md, "GP feasibility".

  python profiles/scripts_feas_gen_cost.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dmosopt_amd.benchmarks import problems as bp  # noqa: E402
from dmosopt_amd.core import engine  # noqa: E402

POP = int(os.environ.get("FEAS_POP", 4096))
G1, G2 = 10, 40
REPS = int(os.environ.get("FEAS_REPS", 5))
dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
if os.environ.get("FEAS_REQUIRE_GPU", "1") == "1":
    assert dev.type == "cuda", "this measurement needs the GPU"

rng = np.random.default_rng(1234)
X = rng.random((512, 2))
Y, C = (t.numpy() for t in bp.tnk(X))


def epoch(feas, gens, seed):
    t0 = time.perf_counter()
    res = engine.run_epoch(
        gens, ["x0", "x1"], ["f0", "f1"], np.zeros(2), np.ones(2), 0.25, X, Y, C,
        pop=POP, optimizer_name="cmaes", surrogate_method_name="gpr",
        surrogate_method_kwargs={"anisotropic": False, "optimizer": "sceua", "seed": seed},
        feasibility_method_name=feas, local_random=np.random.default_rng(seed + 1),
        device=dev,
    )
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert type(res["optimizer"].model.feasibility).__name__ != "NoneType"
    return 1e3 * (time.perf_counter() - t0)


for feas in ("logreg", "gp"):
    for g in (G1, G2):
        epoch(feas, g, 100)
out = {"pop": POP, "g1": G1, "g2": G2, "reps": REPS, "device": str(dev)}
per_gen = {"logreg": [], "gp": []}
epochs = {"logreg": [], "gp": []}
for r in range(REPS):
    for feas in ("logreg", "gp"):
        a = epoch(feas, G1, 200 + r)
        b = epoch(feas, G2, 200 + r)
        per_gen[feas].append((b - a) / (G2 - G1))
        epochs[feas].append((a, b))
for feas in per_gen:
    v = sorted(per_gen[feas])
    out[feas] = {"ms_per_gen_median": v[len(v) // 2], "min": v[0], "max": v[-1],
                 "all": per_gen[feas], "epochs_ms_g1_g2": epochs[feas]}
    print(feas, f"{v[len(v) // 2]:.3f} ms/gen ({v[0]:.3f} .. {v[-1]:.3f})")
if len(sys.argv) > 1:  # optional: keep every figure as JSON
    with open(sys.argv[1], "w") as fh:
        json.dump(out, fh, indent=1)
