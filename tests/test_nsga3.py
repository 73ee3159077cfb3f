"""ops/hip/nsga3.hip against the float64 oracle of tests/test_nsga3_cpu.py,
stage by stage: the float32 (d, h) argmin may legitimately differ from the
float64 one at near-ties, so normalisation and association are checked against
float64 within a tolerance, and the niching exactly, on the kernel's own rank,
niche and dist.

Tolerance of the first two stages: the float32 torch_ref route on the CPU over
the same cases (emulate_fp32 below) deviates from the oracle by at most
EMULATED_SCALE (relative, scale) and EMULATED_DIST (absolute, distances of
O(1)); the kernels get 8x that, the project's margin for fp32 re-association.
Worst seen on the MI355X: MEASURED below."""

import numpy as np
import pytest
import torch

from test_nsga3_cpu import make_case, oracle_distances, oracle_normalize

# worst deviation of the float32 CPU route over CASES x KINDS (emulate_fp32)
EMULATED_SCALE = 2.55e-8
EMULATED_DIST = 4.67e-7
# worst deviation of the kernels on the MI355X over the same cases (a record,
# not a bound: test_select_staged prints each case's figures)
MEASURED = {"scale": 2.55e-8, "dist": 4.70e-7}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dmosopt_amd import ops

    assert ops.native_available(), "native extension must be built on a GPU box"
    return torch.device("cuda", 0)


def _largest_n(H=2048, m=16):
    """Largest merged N the gate admits, by bisection."""
    from dmosopt_amd import _hipops

    fits = lambda n: _hipops.nsga3_select_fits(n, H, m)  # noqa: E731
    lo, hi = 1, 1 << 20
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:  # the footprint grows with N
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


# (ng, np, keep, m, H); None: the gate's largest N, filled in by _shape
CASES = [(1, 1, 1, 2, 2), (3, 2, 2, 2, 3), (33, 31, 32, 3, 15), (65, 64, 64, 3, 91),
         (201, 200, 200, 5, 126), (66, 64, 64, 8, 156), None]
KINDS = ["continuous", "grid"]


def _shape(case, kind):
    if case is not None:
        return case
    n = _largest_n()
    # the edge of the gate in N and H (the niche kernel's LDS block above the
    # default 64 KB); m = 16 on the grid, 3 on continuous data (several
    # fronts, P not empty)
    return (n // 2, n - n // 2, n // 2, 16 if kind == "grid" else 3, 2048)


def _inputs(case, kind):
    ng, np_, keep, m, H = _shape(case, kind)
    N = ng + np_
    Y, Z, dp, rp = make_case(N, m, H, 1000 + N + H, kind)
    X = np.random.default_rng(N).random((N, 3))
    return dict(ng=ng, np=np_, keep=keep, m=m, H=H, Y=Y, Z=Z, dp=dp, rp=rp, X=X)


def _deviation(c, rank, ideal, scale, niche, dist):
    """(scale deviation, relative; worst of |dist - oracle distance to the
    row's own niche| and of dist above the oracle's minimum) of float32
    outputs against the float64 oracle on the same rank."""
    rank = np.asarray(rank)
    z, s, l, _ = oracle_normalize(c["Y"], rank, c["keep"])
    assert np.array_equal(np.asarray(ideal, dtype=np.float64), z)  # bitwise the column min
    dev_scale = np.abs(np.asarray(scale, dtype=np.float64) / s - 1.0).max()
    D = oracle_distances(c["Y"], z, s, c["Z"])
    S = rank <= l
    niche, dist = np.asarray(niche), np.asarray(dist, dtype=np.float64)
    assert (niche[~S] == -1).all() and np.isinf(dist[~S]).all()
    assert ((niche[S] >= 0) & (niche[S] < c["H"])).all()
    rows = np.flatnonzero(S)
    own = np.abs(dist[rows] - D[rows, niche[rows]]).max()
    above = (dist[rows] - D[rows].min(axis=1)).max()
    return dev_scale, max(own, above)


def emulate_fp32():
    """The EMULATED_* figures: torch_ref in float32 on the CPU."""
    from dmosopt_amd.ops import torch_ref

    worst = [0.0, 0.0]
    for case in CASES:
        for kind in KINDS:
            c = _inputs(case, kind)
            Y = torch.as_tensor(c["Y"], dtype=torch.float32)
            rank = torch_ref.pareto_rank(Y)
            ideal, scale, l = torch_ref.nsga3_normalize(Y, rank, c["keep"])
            niche, dist = torch_ref.nsga3_associate(
                Y, ideal, scale, torch.as_tensor(c["Z"], dtype=torch.float32), rank <= l)
            d = _deviation(c, rank.numpy(), ideal.numpy(), scale.numpy(), niche.numpy(),
                           dist.numpy())
            worst = [max(a, b) for a, b in zip(worst, d)]
    return worst


def _call(c, dev, extra=0):
    """The binding on case c; ``extra`` dominated rows appended to the parents."""
    from dmosopt_amd import _hipops

    f = lambda a: torch.as_tensor(a, dtype=torch.float32).to(dev)  # noqa: E731
    ng = c["ng"]
    pp, po = c["X"][ng:], c["Y"][ng:]
    rp = c["rp"]
    if extra:
        g = np.random.default_rng(extra)
        pp = np.vstack([pp, g.random((extra, pp.shape[1]))])
        po = np.vstack([po, c["Y"].max() + 1.0 + g.random((extra, c["m"]))])
        rp = np.concatenate([rp, len(rp) + g.permutation(extra)])
    return _hipops.nsga3_select(
        f(c["X"][:ng]), f(c["Y"][:ng]), f(pp), f(po), c["keep"], f(c["Z"]),
        torch.as_tensor(c["dp"]).to(dev), torch.as_tensor(rp).to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "edge" if c is None else "-".join(map(str, c)))
def test_select_staged(dev, case, kind):
    from dmosopt_amd import ops
    from dmosopt_amd.ops import torch_ref

    c = _inputs(case, kind)
    N, K = c["ng"] + c["np"], min(c["keep"], c["ng"] + c["np"])
    out = _call(c, dev)
    parm, obj, rank_o, perm, ideal, scale, niche, dist = out
    assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.long, torch.long,
                                      torch.float32, torch.float32, torch.long, torch.float32]
    assert parm.shape == (K, 3) and obj.shape == (K, c["m"]) and perm.shape == (K,)
    assert niche.shape == (N,) and dist.shape == (N,)
    Y32 = torch.as_tensor(c["Y"], dtype=torch.float32).to(dev)
    X32 = torch.as_tensor(c["X"], dtype=torch.float32).to(dev)
    rank = ops.pareto_rank(Y32)
    # 1 + 2: normalisation and association against float64
    ds, dd = _deviation(c, rank.cpu().numpy(), ideal.cpu().numpy(), scale.cpu().numpy(),
                        niche.cpu().numpy(), dist.cpu().numpy())
    print(f"{_shape(case, kind)} {kind}: scale deviation {ds:.3e}, dist deviation {dd:.3e}")
    assert ds <= 8 * EMULATED_SCALE and dd <= 8 * EMULATED_DIST
    # 3: niching, exact, on the kernel's own rank / niche / dist
    want = torch_ref.nsga3_niche_sequential(
        rank.cpu(), niche.cpu(), dist.cpu(), c["keep"], c["H"], torch.as_tensor(c["dp"]),
        torch.as_tensor(c["rp"]))
    assert torch.equal(perm.cpu(), want)
    assert torch.equal(rank_o, rank[perm])
    assert torch.equal(parm, X32[perm]) and torch.equal(obj, Y32[perm])
    # 4: repeatable bit for bit; a row's niche / dist do not see unrelated rows
    for a, b in zip(out, _call(c, dev)):
        assert torch.equal(a, b)
    more = _call(c, dev, extra=37) if N + 37 <= _largest_n() else None
    if more is not None:
        assert torch.equal(more[3], perm)
        assert torch.equal(more[4], ideal) and torch.equal(more[5], scale)
        assert torch.equal(more[6][:N], niche) and torch.equal(more[7][:N], dist)
        assert (more[6][N:] == -1).all() and torch.isinf(more[7][N:]).all()


@pytest.mark.gpu
def test_ops_route_and_torch_route_agree(dev):
    """ops.nsga3_select runs the kernels inside the gate and torch_ref on
    device tensors outside it (here: float64); same survivors on a case
    without near-ties."""
    from dmosopt_amd import ops

    c = _inputs((65, 64, 64, 3, 91), "continuous")
    ng = c["ng"]
    for dt in (torch.float32, torch.float64):
        f = lambda a: torch.as_tensor(a, dtype=dt).to(dev)  # noqa: E731
        out = ops.nsga3_select(
            f(c["X"][:ng]), f(c["Y"][:ng]), f(c["X"][ng:]), f(c["Y"][ng:]), c["keep"],
            f(c["Z"]), torch.as_tensor(c["dp"]).to(dev), torch.as_tensor(c["rp"]).to(dev))
        assert out[0].dtype == dt and out[0].is_cuda
        if dt == torch.float32:
            first = out
    assert torch.equal(first[3], out[3])
    assert torch.equal(first[6], out[6])


def _optimizer_run(dev, seed):
    from dmosopt_amd.benchmarks.problems import dtlz2
    from dmosopt_amd.moea.nsga3 import NSGA3Optimizer

    d, m, pop = 7, 3, 92
    opt = NSGA3Optimizer(popsize=pop, nInput=d, nOutput=m, ref_partitions=12)
    opt.set_device(dev)
    bounds = np.column_stack([np.zeros(d), np.ones(d)])
    rng = np.random.default_rng(seed)
    x = opt.generate_initial(bounds, rng)
    y = dtlz2(torch.as_tensor(x, dtype=torch.float32, device=dev), m)
    opt.initialize_strategy(x, y.cpu().numpy(), bounds, rng)
    for _ in range(5):
        xg, gs = opt.generate()
        opt.update(xg, dtlz2(xg, m), gs)
    return opt


@pytest.mark.gpu
def test_optimizer_on_the_gpu(dev):
    a, b = _optimizer_run(dev, 3), _optimizer_run(dev, 3)
    px, py = a.population_objectives
    assert px.shape == (92, 7) and py.shape == (92, 3)
    assert px.dtype == torch.float32 and py.dtype == torch.float32 and px.is_cuda
    assert a.state.rank.dtype == torch.long and a.state.niche.shape == (92,)
    assert torch.isfinite(py).all()
    assert int(a.state.niche.min()) >= 0 and int(a.state.niche.max()) < 91
    for u, v in zip(a.population_objectives, b.population_objectives):
        assert torch.equal(u, v)
    assert a.native_generations_eligible(None) is False
    assert int(a.state.successful_crossovers) + int(a.state.successful_mutations) > 0


def _dtlz2_obj(pp):
    x = np.array([pp[k] for k in sorted(pp.keys())])
    g = ((x[2:] - 0.5) ** 2).sum()
    c, s = np.cos(0.5 * np.pi * x[:2]), np.sin(0.5 * np.pi * x[:2])
    return (1.0 + g) * np.array([c[0] * c[1], c[0] * s[1], s[0]])


def _run_dtlz2(tag):
    import dmosopt_amd

    params = {
        "opt_id": tag,
        "obj_fun": _dtlz2_obj,
        "problem_parameters": {},
        "space": {f"x{i:02d}": [0.0, 1.0] for i in range(7)},
        "objective_names": ["f1", "f2", "f3"],
        "population_size": 40,
        "num_generations": 8,
        "n_initial": 3,
        "initial_maxiter": 2,
        "n_epochs": 2,
        "surrogate_method_name": "gpr",
        "surrogate_method_kwargs": {"anisotropic": False, "optimizer": "sceua"},
        "optimizer": "nsga3",
        "random_seed": 31,
    }
    assert dmosopt_amd.run(params, verbose=False) is not None
    x, y = dmosopt_amd.sopt_dict[tag].optimizer_dict[0].get_evals()
    return x.copy(), y.copy()


@pytest.mark.gpu
def test_run_end_to_end_on_the_gpu(dev):
    xa, ya = _run_dtlz2("t_nsga3_gpu_a")
    xb, yb = _run_dtlz2("t_nsga3_gpu_b")
    assert np.isfinite(xa).all() and np.isfinite(ya).all()
    assert xa.shape[0] > 21 and ya.shape[1] == 3  # the initial design and a resample batch
    assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
