"""The fused generation-loop kernels and the native chunk driver against the
chains of launches they replace: every comparison is torch.equal, both routes
in one process (the bindings' ``fused`` argument, NSGA2Optimizer.gen_fused /
.native_chunks), whatever DMOSOPT_GEN_FUSED says."""

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dmosopt_amd import ops

    assert ops.native_available(), "native extension must be built on a GPU box"
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ select
def _largest_fused_n(m):
    """Largest N = ng + np (ng = N // 2) the fused selection takes at m."""
    from dmosopt_amd import _hipops

    fits = lambda n: _hipops.nsga2_generations_fit(n - n // 2, n // 2, m)  # noqa: E731
    lo, hi = 2, 2048
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:  # the footprint grows with N
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


def _select_both(x_gen, y_gen, pp, po, keep, dev, seed):
    from dmosopt_amd import _hipops

    ng = x_gen.shape[0]
    g = torch.Generator().manual_seed(seed)
    n_cross = 2 * (torch.randint(0, ng // 2 + 1, (1,), generator=g).item())
    c_idx = torch.randperm(ng, generator=g)[:n_cross].to(dev)
    outs = []
    for fused in (0, 1):
        sc = torch.full((), 7, dtype=torch.long, device=dev)
        sm = torch.full((), 3, dtype=torch.long, device=dev)
        r = _hipops.nsga2_select_acc(x_gen, y_gen, pp, po, keep, c_idx, sc, sm,
                                     fused=fused)
        outs.append(list(r) + [sc, sm])
        r2 = _hipops.nsga2_select(x_gen, y_gen, pp, po, keep, fused=fused)
        for a, b in zip(r, r2):  # the plain binding is the same selection
            assert torch.equal(a, b)
    for name, a, b in zip(("parm", "obj", "rank", "perm", "succ_cross", "succ_mut"),
                          *outs):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a, b), name
    return outs[1]


def _rand_case(ng, np_, d, m, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x_gen = torch.rand(ng, d, generator=g).to(dev)
    pp = torch.rand(np_, d, generator=g).to(dev)
    # a coarse grid: many tied objective values and duplicated rows
    y_gen = (torch.randint(0, 12, (ng, m), generator=g).float() / 4).to(dev)
    po = (torch.randint(0, 12, (np_, m), generator=g).float() / 4).to(dev)
    return x_gen, y_gen, pp, po


SHAPES = [(1, 1), (3, 2), (31, 33), (32, 33), (199, 200), (201, 200)]


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("d", [1, 30])
def test_select_fused_matches_chain(dev, m, d):
    for k, (ng, np_) in enumerate(SHAPES):
        for keep in {np_, max(1, np_ // 2)}:
            _select_both(*_rand_case(ng, np_, d, m, dev, 100 * m + k), keep, dev, k)
    # continuous objectives: no ties, long fronts
    g = torch.Generator().manual_seed(m)
    x_gen, pp = torch.rand(201, d, generator=g).to(dev), torch.rand(200, d, generator=g).to(dev)
    y_gen, po = torch.rand(201, m, generator=g).to(dev), torch.rand(200, m, generator=g).to(dev)
    _select_both(x_gen, y_gen, pp, po, 200, dev, 9)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 3, 4])
def test_select_gate_edge(dev, m):
    """The largest N of the gate runs the fused kernel, N + 1 the chain."""
    from dmosopt_amd import _hipops

    n = _largest_fused_n(m)
    assert n >= 401  # the flagship's N
    for N in (n, n + 1):
        ng, np_ = N // 2, N - N // 2
        assert _hipops.nsga2_generations_fit(np_, ng, m) == (N == n)
        _select_both(*_rand_case(ng, np_, 3, m, dev, N), np_, dev, N)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 3])
def test_select_ties(dev, m):
    g = torch.Generator().manual_seed(5)
    d, ng, np_ = 4, 37, 40
    x_gen, pp = torch.rand(ng, d, generator=g).to(dev), torch.rand(np_, d, generator=g).to(dev)
    base = torch.rand(np_, m, generator=g)
    cases = {}
    # duplicated objective rows
    cases["dup_rows"] = (base[torch.randint(0, 5, (ng,), generator=g)], base.clone())
    # children equal to parents (objectives and parameters)
    cases["child_eq_parent"] = (base[:ng].clone(), base.clone())
    # one constant objective column (span 0)
    yc, pc = torch.rand(ng, m, generator=g), base.clone()
    yc[:, 1], pc[:, 1] = 0.25, 0.25
    cases["const_col"] = (yc, pc)
    # all rows identical
    cases["all_same"] = (torch.full((ng, m), 0.5), torch.full((np_, m), 0.5))
    # a front larger than keep: everything on one anti-diagonal
    t = torch.rand(ng + np_, generator=g)
    front = torch.stack([t, 1 - t] + [torch.zeros_like(t)] * (m - 2), 1)
    cases["big_front"] = (front[:ng], front[ng:])
    for name, (y_gen, po) in cases.items():
        xg = pp[:ng].clone() if name == "child_eq_parent" else x_gen
        for keep in (np_, 7):
            _select_both(xg, y_gen.to(dev).contiguous(), pp, po.to(dev).contiguous(),
                         keep, dev, 3)


# ------------------------------------------------------------------- spawn
def _spawn_both(dev, pop, d, C, M, seed):
    from dmosopt_amd import _hipops

    g = torch.Generator().manual_seed(seed)
    poolsize = max(2, pop // 2)
    population = torch.rand(pop, d, generator=g).to(dev)
    rank = torch.sort(torch.randint(0, 5, (pop,), generator=g)).values.to(dev)
    perm = torch.randperm(2 * C + M, generator=g).to(dev)
    ci, mi = perm[: 2 * C].contiguous(), perm[2 * C:].contiguous()
    i1 = torch.randint(0, poolsize, (C,), generator=g)
    i2 = ((i1 + 1 + torch.randint(0, poolsize - 1, (C,), generator=g)) % poolsize).to(dev)
    i1, im = i1.to(dev), torch.randint(0, poolsize, (M,), generator=g).to(dev)
    di_c = (1 + 3 * torch.rand(d, generator=g)).to(dev)
    di_m = (5 + 20 * torch.rand(d, generator=g)).to(dev)
    lo, hi = torch.zeros(d, device=dev), torch.ones(d, device=dev)
    args = (population, rank, poolsize, 0.5, 4242 + seed, ci, mi, i1, i2, im,
            di_c, di_m, lo, hi, 1.0 / d, 99 + seed, 1234 + seed)
    split = _hipops.generation_spawn(*args, rank_sorted=True, fused=0)
    fused = _hipops.generation_spawn(*args, rank_sorted=True, fused=1)
    assert split.shape == (2 * C + M, d)
    assert torch.equal(fused, split)


@pytest.mark.gpu
@pytest.mark.parametrize("pop,d,C,M", [
    (4, 1, 1, 1), (200, 30, 90, 20), (201, 30, 91, 19),
    (200, 30, 0, 199),  # a chunk item with C = 0
    (200, 30, 100, 0),  # a chunk item with M = 0
])
def test_spawn_fused_matches_split(dev, pop, d, C, M):
    for seed in range(3):
        _spawn_both(dev, pop, d, C, M, seed)


# ------------------------------------------------------------------ driver
@pytest.fixture(scope="module")
def tiny_gp(dev):
    from dmosopt_amd.core import engine

    rng = np.random.default_rng(0)
    X = rng.random((5, 3))
    Y = np.column_stack([X.sum(1), ((1 - X) ** 2).sum(1)])
    gp = engine.train(
        3, 2, np.zeros(3), np.ones(3), X, Y, None, surrogate_method_name="gpr",
        surrogate_method_kwargs={"anisotropic": False, "optimizer": "sceua", "seed": 1},
        logger=None, device=dev)
    return gp, X, Y


def _run_loop(dev, tiny_gp, n_gen, gen_fused, native_chunks, **loop_kwargs):
    from dmosopt_amd.core import engine
    from dmosopt_amd.models.model import Model
    from dmosopt_amd.moea.nsga2 import NSGA2Optimizer

    gp, X, Y = tiny_gp
    mdl = Model(objective=gp)
    opt = NSGA2Optimizer(popsize=8, nInput=3, nOutput=2, model=mdl,
                         distance_metric="crowding")
    opt.set_device(dev)
    opt.gen_fused, opt.native_chunks = gen_fused, native_chunks
    rng = np.random.default_rng(77)
    seen = []
    if native_chunks:
        run = opt.run_generations_native
        opt.run_generations_native = lambda *a: (seen.append(1), run(*a))[1]
    res = engine.optimize_loop(
        n_gen, opt, mdl, 3, 2, np.zeros(3), np.ones(3), popsize=8,
        initial=(X.astype(np.float32), Y.astype(np.float32)), local_random=rng,
        **loop_kwargs)
    st = opt.state
    out = dict(
        x=res.x, y=res.y, gen_index=res.gen_index, best_x=res.best_x,
        best_y=res.best_y, rank=st.rank.cpu().numpy(),
        counts=(st.total_crossovers, st.total_mutations,
                int(st.successful_crossovers), int(st.successful_mutations)),
        rng=rng.bit_generator.state, chunks=len(seen))
    return out


def _same(a, b):
    for k in ("x", "y", "gen_index", "best_x", "best_y", "rank"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k]), k
    assert a["counts"] == b["counts"]
    assert a["rng"] == b["rng"]


@pytest.mark.gpu
@pytest.mark.parametrize("n_gen", [3, 16, 17, 33])
def test_driver_matches_per_generation(dev, tiny_gp, n_gen):
    """A partial chunk, one exact chunk and a crossing of each chunk boundary:
    the driver against the per-generation path on the chains, and against the
    per-generation path on the fused kernels."""
    chain = _run_loop(dev, tiny_gp, n_gen, 0, False)
    fused_per_gen = _run_loop(dev, tiny_gp, n_gen, 1, False)
    driver = _run_loop(dev, tiny_gp, n_gen, 1, True)
    assert chain["chunks"] == 0 and fused_per_gen["chunks"] == 0
    assert driver["chunks"] == -(-n_gen // 16)
    assert chain["gen_index"][-1] == n_gen
    _same(fused_per_gen, chain)
    _same(driver, chain)


@pytest.mark.gpu
def test_ineligible_runs_per_generation(dev, tiny_gp):
    """A termination object keeps the loop on the per-generation path, with
    the results of the chains."""
    from dmosopt_amd.termination import MaximumGenerationTermination

    class P:  # the problem fields the criterion reads
        n_objectives, logger = 2, None

    mk = lambda: MaximumGenerationTermination(P(), n_max_gen=5)  # noqa: E731
    chain = _run_loop(dev, tiny_gp, 50, 0, False, termination=mk())
    fused = _run_loop(dev, tiny_gp, 50, 1, True, termination=mk())
    assert fused["chunks"] == 0
    _same(fused, chain)


def test_not_eligible_on_cpu():
    from dmosopt_amd.models.model import Model
    from dmosopt_amd.moea.nsga2 import NSGA2Optimizer

    class Obj:
        def native_mean_args(self, device):
            raise AssertionError("not reached on CPU")

    mdl = Model(objective=Obj())
    opt = NSGA2Optimizer(popsize=8, nInput=3, nOutput=2, model=mdl,
                         distance_metric="crowding")
    assert not opt.native_generations_eligible(mdl)  # before initialize_strategy
    rng = np.random.default_rng(0)
    x, y = rng.random((12, 3)), rng.random((12, 2))
    opt.initialize_strategy(x, y, np.column_stack([np.zeros(3), np.ones(3)]), rng)
    assert opt.state.population_parm.device.type == "cpu"
    assert not opt.native_generations_eligible(mdl)
