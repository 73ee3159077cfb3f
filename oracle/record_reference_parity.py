"""Record the reference implementation's outputs for tests/test_reference_parity.py.

    python oracle/record_reference_parity.py --reference /path/to/reference

Imports the reference `dmosopt` package from the given checkout, builds the
seeded inputs of every parity case, runs the reference on them and stores
inputs + reference outputs in tests/golden/reference_parity.npz (plain
arrays only, no pickles). The tests then compare this project's results
against the recorded values and need no reference checkout at run time.
Re-run only when a parity case is added or its inputs change.
"""

import argparse
import json
import logging
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "reference_parity.npz")


def zdt1(x):
    f1 = x[:, 0]
    g = 1 + 9 * x[:, 1:].mean(axis=1)
    return np.column_stack([f1, g * (1 - np.sqrt(f1 / g))])


class _Problem:
    def __init__(self, d=4, m=2):
        self.n_objectives = m
        self.lb = np.zeros(d)
        self.ub = np.ones(d)
        self.logger = logging.getLogger("parity_record")


def _decisions(term, X_seq, F_seq):
    from dmosopt.datatypes import OptHistory

    out = []
    for g, (X, F) in enumerate(zip(X_seq, F_seq), start=1):
        out.append(bool(term.has_terminated(OptHistory(g, g * 10, X, F, None))))
        if out[-1]:
            break
    return out


def record():
    G = {}

    # ---- MOASMO.epoch on a ZDT1 archive
    from dmosopt.MOASMO import epoch as ref_epoch

    rng = np.random.default_rng(42)
    D = 30
    X = rng.random((120, D))
    Y = zdt1(X)
    gen = ref_epoch(
        100, [f"x{i}" for i in range(D)], ["f1", "f2"],
        np.zeros(D), np.ones(D), 0.25, X, Y, None, pop=100,
        optimizer_name="nsga2", surrogate_method_name="gpr",
        surrogate_method_kwargs={"anisotropic": False, "optimizer": "sceua"},
        local_random=np.random.default_rng(4),
    )
    try:
        next(gen)
        while True:
            gen.send(None)
    except StopIteration as si:
        ref_out = si.args[0] if si.args else None
    G["epoch/X"] = X
    G["epoch/Y"] = Y
    G["epoch/x_resample"] = np.asarray(ref_out["x_resample"])

    # ---- crowding distance / pareto ranking / sortMO
    import dmosopt.dda as ref_dda
    import dmosopt.indicators as ref_ind
    from dmosopt.MOEA import sortMO

    rng = np.random.default_rng(7)
    for n, m in ((16, 2), (100, 3), (257, 5)):
        Y = rng.random((n, m))
        G[f"crowding/Y_{n}_{m}"] = Y
        G[f"crowding/ref_{n}_{m}"] = np.asarray(ref_ind.crowding_distance_metric(Y))

    rng = np.random.default_rng(8)
    for n, m in ((60, 2), (200, 3), (500, 4)):
        Y = rng.random((n, m))
        Y[:5] = Y[10:15]
        G[f"pareto_rank/Y_{n}_{m}"] = Y
        G[f"pareto_rank/ref_{n}_{m}"] = np.asarray(ref_dda.dda_ens(Y))

    rng = np.random.default_rng(9)
    x = rng.random((120, 6))
    y = rng.random((120, 3))
    xs, ys, ranks, dists = sortMO(x, y, y_distance_metrics=["crowding"])
    G["sortmo/x"] = x
    G["sortmo/y"] = y
    G["sortmo/xs"] = np.asarray(xs)
    G["sortmo/ranks"] = np.asarray(ranks)

    # ---- Lacour box decomposition HV and EHVI selection
    from dmosopt.hv_box_decomposition import HyperVolumeBoxDecomposition as RefHV

    rng = np.random.default_rng(11)
    for d, n in ((4, 40), (5, 30)):
        pts = rng.random((n, d))
        G[f"lacour/pts_{d}"] = pts
        G[f"lacour/ref_{d}"] = np.float64(
            RefHV(np.full(d, 1.2)).compute_hypervolume(pts))

    rng = np.random.default_rng(12)
    front = rng.random((25, 2))
    means = rng.random((200, 2)) * 1.5
    vars_ = rng.random((200, 2)) * 0.1 + 0.01
    sel_r, sc_r = RefHV(np.full(2, 2.0)).select_candidates(
        front, means, vars_, n_select=10)
    G["ehvi/front"] = front
    G["ehvi/means"] = means
    G["ehvi/vars"] = vars_
    G["ehvi/sel"] = np.asarray(sel_r)
    G["ehvi/scores"] = np.asarray(sc_r)

    # ---- termination criteria decision sequences
    import dmosopt.termination as rt

    rng = np.random.default_rng(13)
    d, m, T = 4, 2, 60
    X_seq, F_seq = [], []
    F = rng.random((30, m)) + 1.0
    X = rng.random((30, d))
    for t in range(T):
        F = 1.0 + (F - 1.0) * 0.7 + rng.normal(0, 1e-6, F.shape)
        X = 0.5 + (X - 0.5) * 0.7
        F_seq.append(F.copy())
        X_seq.append(X.copy())
    Xb_seq = [rng.random((30, d)) for _ in range(T)]
    Fb_seq = [rng.random((30, m)) for _ in range(T)]
    G["termination/X_conv"] = np.stack(X_seq)
    G["termination/F_conv"] = np.stack(F_seq)
    G["termination/X_noisy"] = np.stack(Xb_seq)
    G["termination/F_noisy"] = np.stack(Fb_seq)
    for cname, mk in (
        ("objtol", lambda: rt.MultiObjectiveToleranceTermination(
            _Problem(), tol=0.005, n_last=5)),
        ("paramtol", lambda: rt.ParameterToleranceTermination(
            _Problem(), tol=1e-3, n_last=5)),
        ("maxgen", lambda: rt.MaximumGenerationTermination(_Problem(), 25)),
    ):
        for hname, Xs, Fs in (("conv", X_seq, F_seq), ("noisy", Xb_seq, Fb_seq)):
            G[f"termination/ref_{cname}_{hname}"] = np.asarray(
                _decisions(mk(), Xs, Fs), dtype=bool)

    # ---- AGE-MOEA environmental selection
    from dmosopt.AGEMOEA import environmental_selection as ref_sel

    rng = np.random.default_rng(14)
    n, d, m, pop = 180, 5, 3, 90
    X = rng.random((n, d))
    Y = rng.random((n, m))
    rx, ry, rrank, rcrowd = ref_sel(np.random.default_rng(0), X, Y, pop, d, m)
    G["agemoea/X"] = X
    G["agemoea/Y"] = Y
    G["agemoea/y_sel"] = np.asarray(ry)
    G["agemoea/rank"] = np.asarray(rrank)

    # ---- GP surrogate posterior
    from dmosopt.model import GPR_Matern as RefGP

    rng = np.random.default_rng(5)
    X = rng.random((100, 10))
    Y = zdt1(np.column_stack([X[:, :1], X[:, 1:]]))
    Xq = rng.random((50, 10))
    ref = RefGP(X, Y, 10, 2, np.zeros(10), np.ones(10), optimizer="sceua")
    mr, _ = ref.predict(Xq)
    G["gp/X"] = X
    G["gp/Y"] = Y
    G["gp/Xq"] = Xq
    G["gp/mean"] = np.asarray(mr)

    # ---- discrepancy metrics, GLP designs, Sobol designs
    from dmosopt import discrepancy as rd
    from dmosopt import sampling as rs

    x = np.random.default_rng(0).random((30, 4))
    G["discrepancy/x"] = x
    G["discrepancy/ref"] = np.array([rd.CD2(x), rd.MD2(x), rd.WD2(x)])

    for n, s in ((50, 4), (100, 6)):
        a = rs.glp(n, s, local_random=np.random.default_rng(3))
        G[f"glp/cd2_ref_{n}_{s}"] = np.float64(rd.CD2(a))

    G["sobol/ref"] = np.asarray(
        rs.sobol(64, 4, local_random=np.random.default_rng(5)))

    # ---- benchmark problem values
    from dmosopt.benchmarks import moo_benchmarks as rb

    rng = np.random.default_rng(0)
    x = rng.random((13, 12))
    G["problems/x"] = x
    cases = [(n, 3) for n in ("dtlz1", "dtlz2", "dtlz3", "dtlz4", "dtlz5",
                              "dtlz7", "wfg1", "wfg4")]
    cases += [(n, 5) for n in ("maf1", "maf2", "maf4")]
    for name, m in cases:
        G[f"problems/ref_{name}"] = np.vstack([
            np.atleast_2d(getattr(rb, name)(x[i], m)) for i in range(len(x))
        ])

    # ---- epsilon-box archive
    from dmosopt.MOEA import EpsilonSort as RefES

    rng = np.random.default_rng(1)
    Y = rng.random((60, 3))
    r = RefES([0.05, 0.05, 0.05])
    for i in range(60):
        r.sortinto(Y[i], tagalong=i)
    G["epsilon/Y"] = Y
    G["epsilon/tagalongs"] = np.asarray(sorted(r.tagalongs), dtype=np.int64)

    # ---- nested parameter space
    from dmosopt.datatypes import ParameterSpace as RefPS

    spec = {"a": [0.0, 1.0], "grp": {"b": [1.0, 2.0], "c": [0, 5, True]}}
    rp = RefPS.from_dict(spec)
    G["pspace/names"] = np.asarray(list(rp.parameter_names), dtype=str)
    G["pspace/bound1"] = np.asarray(rp.bound1)
    G["pspace/bound2"] = np.asarray(rp.bound2)
    G["pspace/is_integer"] = np.asarray(rp.is_integer)
    G["pspace/unflatten_json"] = np.asarray(
        json.dumps(rp.unflatten(np.array([0.5, 1.5, 3.0])),
                   default=lambda o: o.item()))

    # ---- indicators
    from dmosopt.indicators import IGD as RefIGD
    from dmosopt.indicators import PopulationDiversity as RefPD
    from dmosopt.indicators import euclidean_distance_metric as ref_eu

    rng = np.random.default_rng(2)
    F = rng.random((40, 3))
    P = rng.random((25, 3))
    ranks = np.zeros(40, dtype=int)
    ranks[20:] = 1
    G["indicators/F"] = F
    G["indicators/P"] = P
    G["indicators/igd"] = np.float64(RefIGD(P).do(F))
    G["indicators/euclidean"] = np.asarray(ref_eu(F))
    G["indicators/diversity"] = np.asarray(RefPD().do(ranks, F))

    # ---- get_best
    from dmosopt.MOASMO import get_best as ref_get_best

    rng = np.random.default_rng(3)
    x = rng.random((80, 5))
    y = rng.random((80, 3))
    f = rng.random(80)
    c = rng.random((80, 2)) - 0.3
    ep = rng.integers(0, 4, 80)
    best = ref_get_best(x, y, f, c, 5, 3, epochs=ep, feasible=True)
    for k, v in (("x", x), ("y", y), ("f", f), ("c", c), ("ep", ep)):
        G[f"get_best/{k}"] = v
    G["get_best/best_x_shape"] = np.asarray(best[0].shape, dtype=np.int64)
    G["get_best/best_y"] = np.asarray(best[1])

    # ---- SCE-UA on Rosenbrock
    from dmosopt.model import sceua as ref_sceua

    def rosen_np(x):
        return (float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2
                             + (1 - x[:-1]) ** 2)),)

    out = ref_sceua(rosen_np, np.full(4, -2.0), np.full(4, 2.0),
                    4, 4, 3000, 10, 0.1, 0.001, seed=1)
    G["sceua/best"] = np.float64(np.atleast_1d(out[1])[0])
    G["sceua/icall"] = np.int64(np.atleast_1d(out[2])[0])

    # ---- adaptive hypervolume router
    from dmosopt.hv import AdaptiveHyperVolume as RefAHV

    rng = np.random.default_rng(2)
    for d in (5, 7):
        pts = rng.random((60, d))
        G[f"adaptive_hv/pts_{d}"] = pts
        G[f"adaptive_hv/ref_{d}"] = np.float64(
            RefAHV(np.full(d, 1.2)).compute_hypervolume(pts))
    pts = rng.random((40, 12))
    G["adaptive_hv/pts_12"] = pts
    G["adaptive_hv/ref_12"] = np.float64(
        RefAHV(np.full(12, 1.2)).compute_hypervolume(pts))

    return G


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True,
                    help="checkout of the reference implementation "
                         "(the directory that holds the dmosopt package)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        G = record()
    for k, v in G.items():
        assert np.asarray(v).dtype != object, k
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez_compressed(args.out, **G)
    print(f"{len(G)} arrays -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
