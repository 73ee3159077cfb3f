"""GPU numerics tests: gfx950 kernels vs the plain-PyTorch fp32/fp64
reference implementations (the framework's kernel-vs-oracle contract,
SURVEY.md section 4)."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# fused GPU predict against the torch / host path of the same model
PREDICT_TOL = dict(rtol=1e-3, atol=1e-3)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dmosopt_amd import ops

    assert ops.native_available(), "native extension must be built on a GPU box"
    return torch.device("cuda", 0)


def test_matern_train_matches_torch(dev):
    from dmosopt_amd import _hipops
    from dmosopt_amd.models.gp_core import build_kernel_torch

    g = torch.Generator().manual_seed(0)
    X = torch.rand(257, 30, generator=g).float().to(dev)
    theta = torch.tensor(
        [[0.3, math.log(0.5), math.log(1e-4)], [-0.2, math.log(2.0), math.log(1e-6)]]
    ).float().to(dev)
    K_native = _hipops.matern_train(X, theta, 2.5, False, 1e-6)
    K_ref = build_kernel_torch(X.double(), None, theta.double(), nu=2.5, jitter=1e-6)
    assert torch.allclose(K_native.double(), K_ref, atol=5e-5)


def test_matern_cross_aniso_matches_torch(dev):
    from dmosopt_amd import _hipops
    from dmosopt_amd.models.gp_core import build_kernel_torch

    g = torch.Generator().manual_seed(1)
    Xq = torch.rand(100, 10, generator=g).float().to(dev)
    X = torch.rand(211, 10, generator=g).float().to(dev)
    theta = torch.cat(
        [torch.zeros(3, 1), torch.randn(3, 10, generator=g) * 0.3, torch.full((3, 1), -9.0)],
        dim=1,
    ).float().to(dev)
    K_native = _hipops.matern_cross(Xq, X, theta, 2.5, True)
    K_ref = build_kernel_torch(Xq.double(), X.double(), theta.double(), nu=2.5, anisotropic=True)
    assert torch.allclose(K_native.double(), K_ref, atol=5e-5)


def _check_cholesky_batched(dev, B, N):
    from dmosopt_amd import _hipops

    g = torch.Generator().manual_seed(2)
    A = torch.randn(B, N, 8, generator=g)
    K = (A @ A.transpose(1, 2) + 0.5 * torch.eye(N)).float().to(dev).contiguous()
    L_ref = torch.linalg.cholesky(K.double().cpu())
    logdet_ref = torch.log(torch.diagonal(L_ref, dim1=1, dim2=2)).sum(dim=1)
    Kc = K.clone()
    logdet, info = _hipops.cholesky_batched_(Kc)
    assert (info == 0).all()
    L = Kc.double().cpu().tril()
    ld = logdet.double().cpu()
    print(f"B={B} N={N}: max |L - L_ref| = {(L - L_ref).abs().max():.3e}, "
          f"max rel logdet err = {((ld - logdet_ref) / logdet_ref).abs().max():.3e}")
    assert torch.allclose(L, L_ref, atol=2e-3, rtol=1e-3)
    assert torch.allclose(ld, logdet_ref, rtol=1e-4)


def test_cholesky_batched_matches_torch(dev):
    _check_cholesky_batched(dev, B=4, N=300)


@pytest.mark.parametrize("N", [33, 97, 449])
def test_cholesky_single_block_matches_torch(dev, N):
    """B = 49 is the first batch size routed to the one-block-per-matrix
    kernel (B = 4 above takes the multi-launch path). N = 33: one full
    32-column block plus a 1-column block, no second SYRK; N = 97: three full
    blocks plus one column; N = 449: the first step has 417 trailing rows,
    more than one 384-row LDS chunk, so the off-diagonal chunk pair runs."""
    _check_cholesky_batched(dev, B=49, N=N)


def test_solves_match_torch(dev):
    from dmosopt_amd import _hipops

    g = torch.Generator().manual_seed(3)
    B, N, R = 3, 200, 5
    A = torch.randn(B, N, 6, generator=g)
    K = (A @ A.transpose(1, 2) + 0.3 * torch.eye(N)).double()
    L = torch.linalg.cholesky(K).float().to(dev).contiguous()
    Y = torch.randn(B, N, R, generator=g).float().to(dev).contiguous()
    Z = Y.clone()
    _hipops.forward_solve_(L, Z)
    Z_ref = torch.linalg.solve_triangular(L.double().cpu(), Y.double().cpu(), upper=False)
    assert torch.allclose(Z.double().cpu(), Z_ref, atol=1e-3, rtol=1e-3)
    X2 = Z.clone()
    _hipops.backward_solve_(L, X2)
    X_ref = torch.cholesky_solve(Y.double().cpu(), L.double().cpu())
    assert torch.allclose(X2.double().cpu(), X_ref, atol=5e-3, rtol=1e-2)


def test_pareto_rank_matches_reference(dev):
    from dmosopt_amd import _hipops, ops
    from dmosopt_amd.ops import torch_ref

    g = torch.Generator().manual_seed(4)
    for n, m in [(100, 2), (500, 3), (1000, 5)]:
        Y = torch.rand(n, m, generator=g)
        Y[: n // 10] = Y[n // 2 : n // 2 + n // 10]  # inject duplicates
        r_ref = torch_ref.pareto_rank(Y.double())
        # native binding (bit-matrix peel at these N)
        r_native = _hipops.pareto_rank(Y.float().to(dev)).cpu()
        assert torch.equal(r_native, r_ref)
        # the dispatching op
        r_gpu = ops.pareto_rank(Y.float().to(dev)).cpu()
        assert torch.equal(r_gpu, r_ref)
    # many-front stress (d=2 spread points, the TNK-like regime)
    Y2 = torch.rand(4096, 2, generator=g)
    assert torch.equal(
        ops.pareto_rank(Y2.float().to(dev)).cpu(), torch_ref.pareto_rank(Y2.double())
    )


def test_crowding_matches_reference(dev):
    from dmosopt_amd import _hipops
    from dmosopt_amd.ops import torch_ref

    g = torch.Generator().manual_seed(5)
    for n, m in [(64, 2), (513, 3), (2000, 4)]:
        Y = torch.rand(n, m, generator=g)
        d_gpu = _hipops.crowding_distance(Y.float().to(dev)).cpu().double()
        d_ref = torch_ref.crowding_distance(Y.double())
        assert torch.allclose(d_gpu, d_ref, atol=1e-5)


def test_variation_bounds_and_stats(dev):
    from dmosopt_amd import _hipops

    g = torch.Generator().manual_seed(6)
    K, d, C, M = 50, 12, 40, 30
    pool = torch.rand(K, d, generator=g).float().to(dev)
    p1 = torch.randint(0, K, (C,), generator=g).int().to(dev)
    p2 = torch.randint(0, K, (C,), generator=g).int().to(dev)
    di = torch.full((d,), 1.0).float().to(dev)
    lo = torch.zeros(d).float().to(dev)
    hi = torch.ones(d).float().to(dev)
    c1, c2 = _hipops.sbx_batch(pool, p1, p2, di, lo, hi, 12345)
    assert (c1 >= 0).all() and (c1 <= 1).all()
    # midpoint preservation (before clipping dominates): mean over genes
    mid_p = (pool[p1.long()] + pool[p2.long()]).mean()
    mid_c = (c1 + c2).mean()
    assert abs(float(mid_p - mid_c)) < 0.05
    mp = torch.randint(0, K, (M,), generator=g).int().to(dev)
    dm = torch.full((d,), 20.0).float().to(dev)
    child = _hipops.mutation_batch(pool, mp, dm, lo, hi, 0.5, 999)
    assert (child >= 0).all() and (child <= 1).all()
    assert float((child - pool[mp.long()]).abs().mean()) < 0.15
    # determinism: same seed -> same output
    c1b, _ = _hipops.sbx_batch(pool, p1, p2, di, lo, hi, 12345)
    assert torch.equal(c1, c1b)


def test_hv_mc_kernels_match_exact(dev):
    from dmosopt_amd import _hipops
    from dmosopt_amd.hv.exact import hv_3d

    g = torch.Generator().manual_seed(7)
    P = torch.rand(20, 3, generator=g).double()
    ref = torch.full((3,), 1.1).double()
    exact = hv_3d(P.numpy(), ref.numpy())
    Pf = P.float().to(dev).contiguous()
    reff = ref.float().to(dev)
    ideal = Pf.min(dim=0).values.contiguous()
    n = 2_000_000
    hits = _hipops.hv_mc_uniform_hits(Pf, ideal, reff, n, 11)
    box_vol = float(torch.prod(reff - ideal))
    est = box_vol * hits / n
    assert est == pytest.approx(exact, rel=0.02)
    vols = torch.prod(reff[None, :] - Pf, dim=1)
    cdf = (vols.cumsum(0) / vols.sum()).contiguous()
    hits2 = _hipops.hv_fpras_hits(Pf, reff, cdf, n, 13)
    est2 = float(vols.sum()) * hits2 / n
    assert est2 == pytest.approx(exact, rel=0.02)


def test_gp_end_to_end_gpu_vs_cpu(dev):
    """Full GP fit+predict on GPU (native path) tracks the CPU fp64 fit."""
    from dmosopt_amd.models.gp import GPRMatern
    from dmosopt_amd.benchmarks.problems import zdt1

    rng = np.random.default_rng(8)
    X = rng.random((150, 30))
    Y = zdt1(X).numpy()
    gp_gpu = GPRMatern(X, Y, 30, 2, np.zeros(30), np.ones(30), optimizer="sceua",
                       seed=1, device=dev)
    gp_cpu = GPRMatern(X, Y, 30, 2, np.zeros(30), np.ones(30), optimizer="sceua",
                       seed=1, device="cpu")
    Xq = rng.random((64, 30))
    mg, vg = gp_gpu.predict(Xq)
    mc, vc = gp_cpu.predict(Xq)
    Ytrue = zdt1(Xq).numpy()
    rmse_gpu = np.sqrt(((mg - Ytrue) ** 2).mean())
    rmse_cpu = np.sqrt(((mc - Ytrue) ** 2).mean())
    assert rmse_gpu < max(2.5 * rmse_cpu, 0.05)


def test_bench_one_epoch_runs(dev):
    from bench import make_archive, one_epoch

    X, Y = make_archive(seed=3)
    x_res, y_res, hv = one_epoch(X[:100], Y[:100], pop=64, rank=0, world=1,
                                 device=dev, seed=2, n_gen=5)
    assert np.isfinite(hv)


def test_cmaes_update_matches_torch(dev):
    from dmosopt_amd import _hipops
    from dmosopt_amd.moea import cmaes as cm

    g = torch.Generator().manual_seed(9)
    K, d = 64, 30
    A0 = torch.eye(d)[None].repeat(K, 1, 1) + 0.01 * torch.randn(K, d, d, generator=g).tril()
    Ainv0 = torch.linalg.inv(A0)
    pc0 = 0.1 * torch.randn(K, d, generator=g)
    z = torch.randn(K, d, generator=g)
    ps = torch.rand(K, generator=g)
    cc, ccov, pthresh = 2.0 / (d + 2.0), 2.0 / (d**2 + 6.0), 0.44

    # fp64 torch oracle
    A_ref, Ainv_ref, pc_ref = cm.batched_cholesky_update(
        A0.double(), Ainv0.double(), pc0.double(), z.double(), ps.double(),
        cc, ccov, pthresh,
    )
    A_g = A0.float().to(dev).contiguous()
    Ai_g = Ainv0.float().to(dev).contiguous()
    pc_g = pc0.float().to(dev).contiguous()
    _hipops.cmaes_update_(A_g, Ai_g, pc_g, z.float().to(dev), ps.float().to(dev),
                          cc, ccov, pthresh)
    assert torch.allclose(A_g.cpu().double(), A_ref, atol=1e-5)
    assert torch.allclose(Ai_g.cpu().double(), Ainv_ref, atol=1e-4)
    assert torch.allclose(pc_g.cpu().double(), pc_ref, atol=1e-6)


def test_cmaes_optimizer_gpu_e2e(dev):
    """MO-CMA-ES on GPU with the fused update kernel on the hot path."""
    import numpy as np
    from dmosopt_amd.moea.cmaes import CMAESOptimizer
    from dmosopt_amd.benchmarks.problems import zdt1

    rng = np.random.default_rng(3)
    d, pop = 10, 32
    opt = CMAESOptimizer(popsize=pop, nInput=d, nOutput=2, model=None)
    opt.set_device(dev)
    bounds = np.stack([np.zeros(d), np.ones(d)], axis=1)
    x0 = opt.generate_initial(bounds, rng)
    y0 = zdt1(x0).numpy()
    opt.initialize_strategy(x0, y0, bounds, rng)
    for _ in range(5):
        x_gen, st = opt.generate()
        y_gen = zdt1(x_gen.double().cpu()).to(dev).float()
        opt.update(x_gen, y_gen, st)
    px, py = opt.population_objectives
    assert torch.isfinite(py).all()


@pytest.mark.gpu
def test_full_run_on_gpu(tmp_path):
    """Complete dmosopt_amd.run() stack on the GPU: GP surrogate fit with
    the native Cholesky/SCE-UA path, device-resident NSGA2, H5 output."""
    import dmosopt_amd
    from dmosopt_amd.benchmarks.problems import zdt1

    def objfun(pp):
        names = sorted(pp.keys())
        x = np.array([pp[k] for k in names])
        return zdt1(x[None, :]).numpy()[0]

    fp = str(tmp_path / "gpu_run.h5")
    params = {
        "opt_id": "gpu_e2e",
        "obj_fun": objfun,
        "problem_parameters": {},
        "space": {f"x{i:02d}": [0.0, 1.0] for i in range(6)},
        "objective_names": ["f1", "f2"],
        "population_size": 48,
        "num_generations": 8,
        "initial_maxiter": 2,
        "n_initial": 3,
        "n_epochs": 2,
        "surrogate_method_name": "gpr",
        "surrogate_method_kwargs": {"anisotropic": False, "optimizer": "sceua"},
        "optimizer": "nsga2",
        "random_seed": 21,
        "file_path": fp,
        "save": True,
    }
    best = dmosopt_amd.run(params, verbose=False)
    assert best is not None
    bx, by = best
    y = np.column_stack([v for _, v in by])
    assert y.shape[1] == 2 and y.shape[0] > 0
    import os

    assert os.path.exists(fp)
    # drop the module-global driver reference NOW: device tensors held in a
    # module global are otherwise destroyed during interpreter shutdown,
    # after the HIP runtime has torn down (exit-time SIGSEGV)
    import gc

    dmosopt_amd.sopt_dict.clear()
    gc.collect()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_fused_moea_kernels(dev):
    from dmosopt_amd import _hipops

    torch.manual_seed(3)
    # survivor_count against the reference boolean accounting
    n_children, n_pop = 201, 200
    perm = torch.randperm(401, device=dev)[:n_pop]
    c_idx = torch.arange(0, 120, device=dev)
    sc = torch.zeros((), dtype=torch.long, device=dev)
    sm = torch.zeros((), dtype=torch.long, device=dev)
    assert _hipops.survivor_count(perm.contiguous(), c_idx.contiguous(), n_children, sc, sm)
    is_cross = torch.zeros(n_children, dtype=torch.bool, device=dev)
    is_cross[c_idx] = True
    child = perm < n_children
    slot = torch.where(child, perm, torch.zeros_like(perm))
    want_c = (is_cross[slot] & child).sum() // 2
    want_m = ((~is_cross[slot]) & child).sum()
    assert int(sc) == int(want_c) and int(sm) == int(want_m)

    # tournament_pool: valid indices, geometric bias toward best ranks
    N, d, poolsize = 400, 12, 200
    population = torch.randn(N, d, device=dev)
    rank = torch.randint(0, 6, (N,), device=dev, dtype=torch.long)
    picks_best = 0
    for seed in range(20):
        pool, pool_idx = _hipops.tournament_pool(
            population.contiguous(), rank.contiguous(), poolsize, 0.5, seed
        )
        assert pool.shape == (poolsize, d)
        assert int(pool_idx.min()) >= 0 and int(pool_idx.max()) < N
        assert len(set(pool_idx.tolist())) == poolsize  # without replacement
        assert torch.allclose(pool, population[pool_idx])
        picks_best += int((rank[pool_idx] == 0).sum())
    # best-rank candidates must be strongly overrepresented vs uniform
    frac_best_pop = float((rank == 0).sum()) / N
    frac_best_pool = picks_best / (20 * poolsize)
    assert frac_best_pool > 1.2 * frac_best_pop


@pytest.mark.gpu
def test_variation_events_matches_split_path(dev):
    from dmosopt_amd import _hipops
    from dmosopt_amd import ops as dops

    torch.manual_seed(5)
    K, d, C, M = 100, 30, 45, 22
    pool = torch.rand(K, d, device=dev)
    i1 = torch.randint(0, K, (C,), device=dev)
    i2 = (i1 + 1 + torch.randint(0, K - 1, (C,), device=dev)) % K
    im = torch.randint(0, K, (M,), device=dev)
    di_c = torch.full((d,), 1.0, device=dev)
    di_m = torch.full((d,), 20.0, device=dev)
    lo = torch.zeros(d, device=dev)
    hi = torch.ones(d, device=dev)
    total = 2 * C + M
    src_rows = torch.randperm(total, device=dev)

    s1, s2 = 1234, 9876
    c1, c2 = dops.sbx_from_pool(pool, i1, i2, di_c, lo, hi, seed=s1)
    mm = dops.mutation_from_pool(pool, im, di_m, lo, hi, 0.1, seed=s2)
    want = torch.cat([c1, c2, mm], dim=0)[src_rows]

    # event-decoded variant (the event_stream_variation route): slot lists
    # partition [0, total); children must land bit-identically
    c_idx = torch.empty(2 * C, dtype=torch.long, device=dev)
    inv = torch.argsort(src_rows)  # slot of virtual row r
    c_idx[0::2] = inv[:C]
    c_idx[1::2] = inv[C : 2 * C]
    m_idx = inv[2 * C :].contiguous()
    got2 = _hipops.variation_events(
        pool.contiguous(), c_idx.contiguous(), m_idx, i1.contiguous(),
        i2.contiguous(), im.contiguous(), di_c, di_m, lo, hi, 0.1, s1, s2,
    )
    assert torch.equal(got2, want)


@pytest.mark.gpu
def test_all_optimizers_one_epoch_gpu(dev):
    """Every MOEA family steps on the GPU with the fused kernel paths."""
    import numpy as np
    from dmosopt_amd.benchmarks.problems import zdt1
    from dmosopt_amd.core import engine
    from dmosopt_amd.models.model import Model

    d, m, pop = 8, 2, 64
    rng = np.random.default_rng(0)
    X = rng.random((40, d)).astype(np.float32)
    Y = zdt1(X).numpy().astype(np.float32)

    class TorchObj:
        def evaluate_tensor(self, x):
            return zdt1(x.double()).to(x.dtype)

        def evaluate(self, x):
            return zdt1(np.asarray(x)).numpy()

    mdl = Model(objective=TorchObj())
    from dmosopt_amd.config import optimizer_registry, resolve

    for name in ["nsga2", "age", "smpso", "cmaes", "trs"]:
        cls = resolve(optimizer_registry, name)
        opt = cls(popsize=pop, nInput=d, nOutput=m, model=mdl)
        opt.set_device(dev)
        res = engine.optimize_loop(
            4, opt, mdl, d, m, np.zeros(d), np.ones(d), popsize=pop,
            initial=(X, Y), local_random=np.random.default_rng(7),
        )
        assert res.best_x.shape[1] == d and res.best_y.shape[1] == m
        assert np.isfinite(res.best_y).all(), name


@pytest.mark.gpu
def test_gp_nmll_fused_matches_torch_oracle(dev):
    from dmosopt_amd import _hipops
    from dmosopt_amd.models.gp_core import batched_nmll

    torch.manual_seed(2)
    N, d, B = 120, 8, 10
    X = torch.rand(N, d, device=dev)
    y = torch.randn(N, device=dev)
    theta = torch.stack(
        [
            torch.zeros(B, device=dev),                      # log sf2
            torch.rand(B, device=dev) * 1.5 - 1.0,           # log ell
            torch.full((B,), -3.0, device=dev),              # log noise
        ],
        dim=1,
    )
    got = _hipops.gp_nmll(X.contiguous(), theta.contiguous(), y.contiguous(),
                          2.5, False, 1e-6)
    want = batched_nmll(X.double(), y.double(), theta.double(), nu=2.5,
                        anisotropic=False, jitter=1e-6, differentiable=True)
    assert torch.allclose(got.double().cpu(), want.cpu(), rtol=2e-3, atol=2e-3)


@pytest.mark.gpu
def test_gp_predict_mean_fused_matches_oracle(dev):
    import numpy as np
    from dmosopt_amd.models.gp import GPRMatern
    from dmosopt_amd.benchmarks.problems import zdt1

    rng = np.random.default_rng(3)
    X = rng.random((90, 6))
    Y = zdt1(X).numpy()
    gp = GPRMatern(X, Y, 6, 2, np.zeros(6), np.ones(6), optimizer="sceua",
                   seed=11, device=dev)
    xq = torch.as_tensor(rng.random((33, 6)), device=dev)
    got = gp.evaluate_tensor(xq).cpu().numpy()          # fused affine path
    want, _ = gp.predict(xq.cpu().numpy())               # host oracle path
    assert np.allclose(got, want, **PREDICT_TOL)


# N = 33 is one element past a 32-wide tile: the smallest shape with a tile edge
_CHECK_N, _CHECK_D, _CHECK_B, _CHECK_P = 33, 2, 2, 5


def _gp_call_args(dev, aniso):
    """Valid float32 GPU arguments of gp_nmll and gp_predict_mean."""
    N, D, B, P = _CHECK_N, _CHECK_D, _CHECK_B, _CHECK_P
    g = torch.Generator().manual_seed(33)
    p = D + 2 if aniso else 3
    theta = torch.cat([torch.zeros(B, 1), torch.rand(B, p - 2, generator=g) - 1.0,
                       torch.full((B, 1), -3.0)], dim=1)
    a = dict(
        X=torch.rand(N, D, generator=g), Xq=torch.rand(P, D, generator=g),
        theta=theta, y=torch.randn(N, generator=g),
        alpha=torch.randn(B, N, 1, generator=g), y_mean=torch.randn(B, generator=g),
        y_std=torch.rand(B, generator=g) + 0.5, q_lb=torch.zeros(D),
        q_invrg=torch.ones(D),
    )
    return {k: v.float().contiguous().to(dev) for k, v in a.items()}


def _call_nmll(a, aniso=False, **over):
    from dmosopt_amd import _hipops

    a = {**a, **over}
    return _hipops.gp_nmll(a["X"], a["theta"], a["y"], 2.5, aniso, 1e-6)


def _call_predict_mean(a, aniso=False, **over):
    from dmosopt_amd import _hipops

    a = {**a, **over}
    return _hipops.gp_predict_mean(
        a["Xq"], a["X"], a["theta"], a["alpha"], a["y_mean"], a["y_std"], 2.5,
        aniso, a["q_lb"], a["q_invrg"])


@pytest.mark.gpu
@pytest.mark.parametrize("call,name", [(_call_nmll, "gp_nmll"),
                                       (_call_predict_mean, "gp_predict_mean")])
def test_gp_entry_points_reject_bad_arguments(dev, call, name):
    """gp_nmll and gp_predict_mean reject what gp_nmll_grad and
    gp_predict_mean_var reject, and name themselves in the message."""
    iso, ard = _gp_call_args(dev, False), _gp_call_args(dev, True)
    for a, aniso in ((iso, False), (ard, True)):
        out = call(a, aniso)                      # the valid call goes through
        assert torch.isfinite(out).all()
    with pytest.raises(RuntimeError, match=name + ": X must be a GPU tensor"):
        call(iso, X=iso["X"].cpu())
    with pytest.raises(RuntimeError, match=name + ": theta must be float32"):
        call(iso, theta=iso["theta"].double())
    with pytest.raises(RuntimeError, match=name + ": theta width"):
        call(iso, True)                           # aniso wants D + 2 = 4 columns
    with pytest.raises(RuntimeError, match=name + ": theta width"):
        call(ard, False)                          # isotropic wants 3 columns
    if call is _call_nmll:
        with pytest.raises(RuntimeError, match="gp_nmll: y must be"):
            call(iso, y=iso["y"][:5].contiguous())
        with pytest.raises(RuntimeError, match="gp_nmll: y must be float32"):
            call(iso, y=iso["y"].double())
    else:
        with pytest.raises(RuntimeError, match="gp_predict_mean: q_lb and q_invrg"):
            call(iso, q_invrg=None)
        with pytest.raises(RuntimeError, match="gp_predict_mean: alpha must be a GPU"):
            call(iso, alpha=iso["alpha"].cpu())
        with pytest.raises(RuntimeError, match="gp_predict_mean: y_std must be float32"):
            call(iso, y_std=iso["y_std"].double())
        with pytest.raises(RuntimeError, match="gp_predict_mean: q_lb/q_invrg must be"):
            call(iso, q_lb=torch.zeros(3, device=dev), q_invrg=torch.ones(3, device=dev))
        with pytest.raises(RuntimeError, match="gp_predict_mean: alpha/y_mean/y_std"):
            call(iso, y_mean=iso["y_mean"][:1].contiguous())


_FORCE_TORCH_CHILD = r"""
import sys, numpy as np, torch
from dmosopt_amd import ops
from dmosopt_amd.models.gp import GPRMatern
N, D, B, P = (int(v) for v in sys.argv[2:6])
assert ops._FORCE_TORCH
rng = np.random.default_rng(33)
X = rng.random((N, D))
Y = np.column_stack([np.sin(3.0 * X[:, 0]) + X[:, 1], X[:, 0] ** 2 - X[:, 1]])
lb, ub = np.full(D, -0.5), np.full(D, 1.5)
theta = np.array([[0.1, -0.7, -7.0], [-0.2, -0.4, -7.0]])
gp = GPRMatern(X, Y, D, B, lb, ub, theta_override=theta, device="cuda")
assert gp.dtype == torch.float32 and gp._fitted.X.is_cuda
xq = rng.random((P, D))
got = gp.evaluate_tensor(torch.as_tensor(xq, device="cuda"))
assert got.is_cuda and got.dtype == torch.float32
# forced torch: nothing on the way loaded the native extension
assert ops._native is None, "evaluate_tensor took the native path"
assert not gp.supports_device_mean_variance
np.savez(sys.argv[1], got=got.cpu().numpy(), want=gp.evaluate(xq))
"""


@pytest.mark.gpu
def test_force_torch_covers_evaluate_tensor(dev, tmp_path):
    """DMOSOPT_AMD_FORCE_TORCH=1 (read at import: fresh child process) keeps
    evaluate_tensor of a float32 GPU model on the torch path, where it agrees
    with the model's host evaluate()."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = tmp_path / "force_torch.npz"
    env = dict(os.environ)
    env["DMOSOPT_AMD_FORCE_TORCH"] = "1"
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    subprocess.run(
        [sys.executable, "-c", _FORCE_TORCH_CHILD, str(path), str(_CHECK_N),
         str(_CHECK_D), str(_CHECK_B), str(_CHECK_P)],
        check=True, env=env, cwd=root, timeout=120)
    r = np.load(path)
    assert r["got"].shape == (_CHECK_P, _CHECK_B)
    assert np.isfinite(r["want"]).all()
    assert np.allclose(r["got"], r["want"], **PREDICT_TOL)


@pytest.mark.gpu
def test_gpu_epoch_bit_determinism(dev):
    """Two same-seed epochs on the GPU must agree bitwise — the multi-GPU
    weak-scaling bench replicates the MOEA control flow across ranks, so
    every kernel feeding control flow must be run-to-run deterministic
    (no float atomics, fixed-order reductions, counter-based RNG)."""
    from bench import make_archive, one_epoch

    X, Y = make_archive(seed=9)
    r1 = one_epoch(X, Y, pop=64, rank=0, world=1, device=dev, seed=5, n_gen=12)
    r2 = one_epoch(X, Y, pop=64, rank=0, world=1, device=dev, seed=5, n_gen=12)
    assert torch.equal(r1[0].cpu(), r2[0].cpu()), "resample params diverged"
    assert torch.equal(r1[1].cpu(), r2[1].cpu()), "resample objectives diverged"


# ------------------------------------------------------------ exact HV kernels
def _np_hv2d(points, ref):
    from dmosopt_amd.hv import exact

    pts = np.asarray(points, dtype=np.float64)
    pts = pts[np.all(pts < ref, axis=1)]
    if len(pts) == 0:
        return 0.0
    order = np.lexsort((pts[:, 1], pts[:, 0]))
    pts = pts[order]
    y = pts[:, 1]
    pm = np.empty(len(y))
    pm[0] = np.inf
    if len(y) > 1:
        pm[1:] = np.minimum.accumulate(y)[:-1]
    pts = pts[y < pm]
    if len(pts) == 0:
        return 0.0
    x_next = np.empty(len(pts))
    x_next[:-1] = pts[1:, 0]
    x_next[-1] = ref[0]
    return float(np.dot(x_next - pts[:, 0], ref[1] - pts[:, 1]))


def test_hv2d_kernel_matches_oracle(dev):
    from dmosopt_amd.hv.exact import hv_2d_device

    rng = np.random.default_rng(0)
    ref = np.array([1.2, 1.3])
    for n in (1, 2, 7, 63, 64, 200, 1024, 4096):
        pts = rng.random((n, 2)) * 1.5  # some rows beyond the ref point
        pts[rng.random(n) < 0.1] = pts[0]  # duplicates
        got = hv2d_val = hv_2d_device(pts, ref)
        want = _np_hv2d(pts, ref)
        assert got == pytest.approx(want, rel=1e-10, abs=1e-12), n


def test_hv3d_kernel_matches_oracle(dev):
    from dmosopt_amd.hv import exact

    rng = np.random.default_rng(1)
    ref = np.array([1.1, 1.1, 1.1])
    for n in (1, 5, 64, 333, 1024):
        pts = rng.random((n, 3)) * 1.3
        got = exact.hv_3d_device(pts, ref)
        # host oracle (pure numpy path, force below device threshold)
        pts_f = pts[np.all(pts < ref, axis=1)]
        want = 0.0
        if len(pts_f):
            pts_s = pts_f[np.argsort(pts_f[:, 2], kind="stable")]
            for i in range(len(pts_s)):
                z_hi = pts_s[i + 1, 2] if i + 1 < len(pts_s) else ref[2]
                dzv = z_hi - pts_s[i, 2]
                if dzv > 0:
                    want += dzv * _np_hv2d(pts_s[: i + 1, :2], ref[:2])
        assert got == pytest.approx(want, rel=1e-10, abs=1e-12), n


def test_ehvi_kernel_matches_oracle(dev):
    from dmosopt_amd.hv.exact import HyperVolumeBoxDecomposition

    rng = np.random.default_rng(2)
    for d in (2, 3, 5):
        ref = np.full(d, 2.0)
        box = HyperVolumeBoxDecomposition(ref)
        front = rng.random((40, d))
        L, U = box._decompose_dominated_space(front)
        mu = rng.random((300, d)) * 1.5
        var = rng.random((300, d)) * 0.2 + 0.01
        # explicit fp64 scipy oracle (the _batch_ehvi numpy small-path math)
        from scipy.stats import norm

        std = np.sqrt(var)[:, None, :]
        mub = mu[:, None, :]
        Lb, Ub = L[None, :, :], U[None, :, :]
        with np.errstate(invalid="ignore"):
            zl, zu = (Lb - mub) / std, (Ub - mub) / std
        Phi_l = np.where(np.isinf(Lb), 0.0, norm.cdf(zl))
        Phi_u = np.where(np.isinf(Ub), 1.0, norm.cdf(zu))
        phi_l = np.where(np.isinf(Lb), 0.0, norm.pdf(zl))
        phi_u = np.where(np.isinf(Ub), 0.0, norm.pdf(zu))
        want = (std * (phi_l - phi_u) + mub * (Phi_u - Phi_l)).prod(axis=2).sum(axis=1)
        got = box._batch_ehvi_device(L, U, mu, var)
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)


def test_lacour_device_matches_numpy(dev):
    from dmosopt_amd.hv.exact import _FlatUBSet, lacour_hv_device

    rng = np.random.default_rng(3)
    for d, n in ((4, 20), (4, 80), (5, 60), (6, 40)):
        ref = np.full(d, 1.0 + 0.1 * d)
        pts = rng.random((n, d))
        # same preprocessing as compute_hypervolume: filter + z-sort
        from dmosopt_amd.hv.exact import _filter_dominated

        p = _filter_dominated(pts)
        p = p[np.all(p < ref, axis=1)]
        p = p[np.argsort(p[:, -1], kind="stable")]
        ub = _FlatUBSet(ref, p)
        for i in range(len(p)):
            ub.insert(i)
        want = float(ub.volumes().sum())
        got = lacour_hv_device(p, ref)
        assert got == pytest.approx(want, rel=1e-9), (d, n)


def test_compute_hypervolume_device_route(dev):
    """Large fronts route to the device kernels inside the public entry."""
    from dmosopt_amd.hv.exact import HyperVolumeBoxDecomposition, hv_2d

    rng = np.random.default_rng(4)
    ref4 = np.full(4, 1.5)
    pts = rng.random((96, 4))
    hv_dev = HyperVolumeBoxDecomposition(ref4).compute_hypervolume(pts)
    assert hv_dev > 0
    # 2D public entry with a device-resident tensor input
    front = torch.rand(512, 2, generator=torch.Generator().manual_seed(5))
    ref2 = np.array([1.1, 1.1])
    got = hv_2d(front.to(dev), ref2)
    want = _np_hv2d(front.numpy(), ref2)
    assert got == pytest.approx(want, rel=1e-10)


# ----------------------------------------------------------------- bf16 path
def test_mfma_bf16_probe_layout(dev):
    """Verify the assumed A/B/C fragment mapping of mfma_f32_16x16x32_bf16
    against a torch matmul oracle (asymmetric B per the guide's advice)."""
    from dmosopt_amd import _hipops

    g = torch.Generator().manual_seed(11)
    A = torch.randn(16, 32, generator=g).float().to(dev)
    B = (torch.arange(32 * 16, dtype=torch.float32).reshape(32, 16) * 0.01
         + torch.randn(32, 16, generator=g)).to(dev)
    D = _hipops.mfma_bf16_probe(A.contiguous(), B.contiguous())
    want = (A.to(torch.bfloat16).float() @ B.to(torch.bfloat16).float())
    torch.testing.assert_close(D, want, rtol=1e-5, atol=1e-5)


def test_matern_cross_bf16_matches_rounded_oracle(dev):
    from dmosopt_amd import ops

    g = torch.Generator().manual_seed(12)
    for P, N, Dd, aniso in ((200, 300, 30, False), (97, 131, 30, True), (64, 64, 100, False)):
        Xq = torch.rand(P, Dd, generator=g).float().to(dev)
        X = torch.rand(N, Dd, generator=g).float().to(dev)
        p = Dd if aniso else 1
        theta = torch.zeros(2, 2 + p)
        theta[:, 0] = torch.tensor([0.0, 0.3])      # log sf2
        theta[:, 1:-1] = torch.randn(2, p, generator=g) * 0.3  # log ell
        theta[:, -1] = -10.0
        theta = theta.float().to(dev)
        K = ops.matern_cross_bf16_kernel(Xq, X, theta, 2.5, aniso)
        # oracle: same math from the SAME bf16-rounded scaled inputs, fp32
        for b in range(2):
            ell = torch.exp(theta[b, 1:-1]) if aniso else torch.exp(theta[b, 1:2])
            qs = (Xq / ell).to(torch.bfloat16).float()
            xs = (X / ell).to(torch.bfloat16).float()
            d2 = ((qs * qs).sum(1)[:, None] + (xs * xs).sum(1)[None, :]
                  - 2.0 * qs @ xs.T).clamp_min(0)
            r = torch.sqrt(d2)
            s = math.sqrt(5.0) * r
            want = torch.exp(theta[b, 0]) * (1 + s + (5.0 / 3.0) * d2) * torch.exp(-s)
            torch.testing.assert_close(K[b], want, rtol=1e-3, atol=2e-4)
        # and the bf16 rounding effect vs the exact fp32 kernel is bounded
        K32 = ops.matern_cross_kernel(Xq, X, theta, 2.5, aniso)
        assert float((K - K32).abs().max()) < 0.05 * float(torch.exp(theta[:, 0]).max())


def test_cholesky_bf16_syrk_factorizes(dev):
    from dmosopt_amd import ops

    g = torch.Generator().manual_seed(13)
    B, N = 4, 300
    A = torch.randn(B, N, 40, generator=g).float()
    K = (A @ A.transpose(1, 2) / 40 + 0.5 * torch.eye(N)).to(dev).contiguous()
    Kc = K.clone()
    L, logdet, info = ops.chol_factor_batched_bf16(Kc)
    assert int(info.abs().sum()) == 0
    Lt = torch.tril(L)
    rec = Lt @ Lt.transpose(1, 2)
    # trailing updates carry bf16 rounding: reconstruction error is
    # bf16-scale relative to the matrix norm, far below the 0.5 diagonal
    err = (rec - K).abs().max()
    assert float(err) < 0.05, float(err)
    # fp32 reference factor for comparison
    K2 = K.clone()
    L32, _, info32 = ops.chol_factor_batched(K2)
    assert float((torch.tril(L32) - Lt).abs().max()) < 0.05


def test_gp_bf16_end_to_end(dev):
    from dmosopt_amd.models.gp import GPRMatern

    rng = np.random.default_rng(14)
    X = rng.random((300, 30))
    Y = np.column_stack([np.sum(X**2, axis=1), np.sum((X - 1) ** 2, axis=1)])
    kw = dict(optimizer="sceua", seed=5, device=dev)
    gp32 = GPRMatern(X, Y, 30, 2, np.zeros(30), np.ones(30), compute="fp32", **kw)
    gp16 = GPRMatern(X, Y, 30, 2, np.zeros(30), np.ones(30), compute="bf16", **kw)
    # same seed + fp32 search in both modes -> identical theta
    torch.testing.assert_close(gp16.theta, gp32.theta)
    q = rng.random((512, 30))
    m32, v32 = gp32.predict(q)
    m16, v16 = gp16.predict(q)
    scale = np.abs(m32).mean()
    # bf16 rounding through kernel + solve: ~1-3% mean posterior error
    # (measured 1.1% on the bench archive; HV delta 1e-4)
    assert np.abs(m16 - m32).mean() / scale < 0.05, np.abs(m16 - m32).mean() / scale
    assert np.isfinite(v16).all()
    # tensor route stays finite and close
    qt = torch.as_tensor(q, dtype=torch.float32, device=dev)
    mt = gp16.evaluate_tensor(qt)
    assert float((mt.cpu().double() - torch.as_tensor(m16)).abs().mean()) / scale < 0.05


def test_agemoea_survival_kernel_matches_host_loop(dev):
    """The single-workgroup greedy 2-NN kernel reproduces the host loop's
    selections and scores exactly on the SAME fp32 distance matrix."""
    from dmosopt_amd import _hipops

    rng = np.random.default_rng(21)
    for m, n_ext, p in ((150, 2, 2.0), (600, 3, 1.3), (1024, 2, 0.7)):
        Y = rng.random((m, 3)).astype(np.float32)
        At = torch.as_tensor(Y, device=dev)
        Dt = _hipops.minkowski_norm_matrix(At.contiguous(), float(p))
        # the fused matrix kernel must match the torch route closely
        nn_t = torch.linalg.vector_norm(At.abs(), ord=float(p), dim=1)
        Dt_ref = torch.cdist(At.double(), At.double(), p=float(p)) / nn_t.double()[:, None]
        torch.testing.assert_close(Dt.double(), Dt_ref, rtol=2e-4, atol=2e-5)
        extreme = np.arange(n_ext)
        pre = torch.zeros(m, dtype=torch.uint8, device=dev)
        pre[:n_ext] = 1
        got = _hipops.agemoea_survival(Dt, pre).cpu().numpy()

        # host oracle: the incremental numpy loop on the identical matrix
        # in FLOAT32 (the kernel's arithmetic): the d1+d2 score sums round
        # differently in fp64 and near-ties then flip the greedy order
        distances = Dt.cpu().numpy()  # float32
        crowd = np.zeros(m, dtype=np.float32)
        crowd[extreme] = np.inf
        selected = np.zeros(m, dtype=bool)
        selected[extreme] = True
        remaining = np.flatnonzero(~selected)
        sel_idx = np.flatnonzero(selected)
        D_sel = distances[np.ix_(remaining, sel_idx)]
        if D_sel.shape[1] >= 2:
            part = np.partition(D_sel, 1, axis=1)
            d1, d2 = part[:, 0].copy(), part[:, 1].copy()
        else:
            d1 = D_sel[:, 0].copy()
            d2 = np.full(len(remaining), np.inf, dtype=np.float32)
        alive = np.ones(len(remaining), dtype=bool)
        for _ in range(len(remaining)):
            score = np.where(alive, np.where(np.isinf(d2), d1, d1 + d2),
                             np.float32(-np.inf))
            pos = int(np.argmax(score))
            best = remaining[pos]
            crowd[best] = d1[pos] if np.isinf(d2[pos]) else d1[pos] + d2[pos]
            alive[pos] = False
            dn = distances[remaining, best]
            repl2 = alive & (dn < d2)
            d2[repl2] = dn[repl2]
            swap = alive & (d2 < d1)
            d1[swap], d2[swap] = d2[swap], d1[swap]

        assert np.isinf(got[:n_ext]).all()
        np.testing.assert_array_equal(got[n_ext:], crowd[n_ext:])


def test_agemoea_gpu_selection_e2e(dev):
    """environmental_selection on a big GPU population routes the survival
    scores through the device kernel and returns a coherent survivor set."""
    from dmosopt_amd.moea.agemoea import environmental_selection

    rng = np.random.default_rng(22)
    n, d, m = 1500, 10, 3
    X = torch.rand(n, d, device=dev)
    Y = torch.rand(n, m, device=dev)
    xs, ys, rank, cd = environmental_selection(
        np.random.default_rng(0), X, Y, 700, d, m
    )
    assert xs.shape == (700, d) and ys.shape == (700, m)
    assert np.isfinite(ys).all()


def test_nmll_graph_matches_eager(dev, monkeypatch):
    """The hipGraph-captured NMLL pipeline must be BITWISE identical to the
    eager launch sequence (same kernels, same order), across replays with
    changing theta."""
    from dmosopt_amd.models import gp_core

    g = torch.Generator().manual_seed(31)
    N, D, B = 200, 30, 18
    X = torch.rand(N, D, generator=g).float().to(dev)
    y = torch.randn(B, N, generator=g).float().to(dev)
    gp_core._nmll_graphs.clear()

    thetas = [
        torch.cat([
            torch.randn(B, 1, generator=g) * 0.3,
            torch.randn(B, 1, generator=g) * 0.5,
            torch.full((B, 1), -8.0) + torch.rand(B, 1, generator=g),
        ], dim=1).float().to(dev)
        for _ in range(4)
    ]
    # eager reference
    monkeypatch.setenv("DMOSOPT_NMLL_GRAPH", "0")
    eager = [gp_core.batched_nmll(X, y, t, nu=2.5, anisotropic=False) for t in thetas]
    # graph path (fresh capture + replays)
    monkeypatch.setenv("DMOSOPT_NMLL_GRAPH", "1")
    graphed = [gp_core.batched_nmll(X, y, t, nu=2.5, anisotropic=False) for t in thetas]
    gp_core._nmll_graphs.clear()
    for e, gr in zip(eager, graphed):
        assert torch.equal(e, gr), float((e - gr).abs().max())


def test_pareto_rank_large_n_sync_free(dev):
    """N beyond the old 2048 gate (the 8-GPU headline regime: cat pop is
    1600+1600=3200 rows) must stay on the sync-free cooperative peel and
    match the reference ranking."""
    from dmosopt_amd import ops
    from dmosopt_amd.ops import torch_ref

    g = torch.Generator().manual_seed(41)
    for n, m in ((3200, 2), (4096, 2), (5000, 5)):
        Y = torch.rand(n, m, generator=g)
        Y[: n // 20] = Y[n // 2 : n // 2 + n // 20]  # duplicates
        r_gpu = ops.pareto_rank(Y.float().to(dev)).cpu()
        r_ref = torch_ref.pareto_rank(Y.double())
        assert torch.equal(r_gpu, r_ref), (n, m)


def test_pareto_rank_early_stop_truncation_exact(dev):
    """Early-stop peel (pareto_rank stop=k, the nsga2_select route): every
    point that can enter the kept top-k carries its TRUE rank, the sentinel
    exceeds every kept rank, and the kept set (rank-sorted top-k) is
    identical to the full ranking's."""
    from dmosopt_amd.ops import _load_native
    from dmosopt_amd.ops import torch_ref

    native = _load_native()
    g = torch.Generator().manual_seed(43)
    for n, m, k in ((3200, 2, 1600), (4096, 3, 1024), (2500, 2, 2499)):
        Y = torch.rand(n, m, generator=g)
        Y[: n // 30] = Y[n // 3 : n // 3 + n // 30]  # duplicates
        Yd = Y.float().to(dev)
        r_full = torch_ref.pareto_rank(Y.double())
        r_stop = native.pareto_rank(Yd, k).cpu()
        # truncation selection keeps the k lowest ranks (stable by index)
        keep_full = torch.argsort(r_full, stable=True)[:k]
        keep_stop = torch.argsort(r_stop, stable=True)[:k]
        assert torch.equal(keep_full, keep_stop), (n, m, k)
        # every kept point carries its true rank; sentinel dominates the rest
        assert torch.equal(r_stop[keep_stop], r_full[keep_full]), (n, m, k)
        assert int(r_stop.max()) <= int(r_full.max()) + 1


@pytest.mark.parametrize("n", [1024, 1025])
@pytest.mark.parametrize("m", [2, 3])
def test_pareto_rank_route_boundary(dev, n, m):
    """N = 1024 is the last bit-matrix shape (and its largest LDS block),
    N = 1025 the first cooperative one: both match the float64 reference,
    and the early-stop peel at 1025 keeps the exact top-k."""
    from dmosopt_amd import _hipops
    from dmosopt_amd.ops import torch_ref

    g = torch.Generator().manual_seed(47 + m)
    Y = torch.rand(n, m, generator=g)
    Y[: n // 10] = Y[n // 2 : n // 2 + n // 10]  # inject duplicates
    Yd = Y.float().to(dev)
    r_full = torch_ref.pareto_rank(Y.double())
    assert torch.equal(_hipops.pareto_rank(Yd).cpu(), r_full)
    if n == 1025:
        k = 512
        r_stop = _hipops.pareto_rank(Yd, k).cpu()
        keep_full = torch.argsort(r_full, stable=True)[:k]
        keep_stop = torch.argsort(r_stop, stable=True)[:k]
        assert torch.equal(keep_full, keep_stop)
        assert torch.equal(r_stop[keep_stop], r_full[keep_full])
        assert int(r_stop.max()) <= int(r_full.max()) + 1


@pytest.mark.parametrize("n,m", [(33, 2), (65, 3)])
def test_dominance_degree_matrix_matches_reference(dev, n, m):
    """More than one 32-row tile each way, duplicated rows (mutual degree m)
    and one constant column (every pair counts it)."""
    from dmosopt_amd import _hipops
    from dmosopt_amd.ops import torch_ref

    g = torch.Generator().manual_seed(53)
    Y = torch.rand(n, m, generator=g)
    Y[: n // 10] = Y[n // 2 : n // 2 + n // 10]
    Y[:, m - 1] = 0.25
    D = _hipops.dominance_degree_matrix(Y.to(dev)).cpu()
    assert torch.equal(D, torch_ref.dominance_degree_matrix(Y))


def test_nsga2_select_acc_rejects_more_children_than_it_counts(dev):
    """The survivor count takes at most 2048 children; beyond, the call
    raises before any launch and leaves the counters alone."""
    from dmosopt_amd import _hipops

    ng, npop, d, m = 2049, 8, 3, 2
    x_gen, y_gen = torch.rand(ng, d, device=dev), torch.rand(ng, m, device=dev)
    parm, obj = torch.rand(npop, d, device=dev), torch.rand(npop, m, device=dev)
    c_idx = torch.arange(0, 100, device=dev)
    sc = torch.full((), 7, dtype=torch.long, device=dev)
    sm = torch.full((), 11, dtype=torch.long, device=dev)
    for fused in (0, 1):
        with pytest.raises(RuntimeError, match="2048"):
            _hipops.nsga2_select_acc(x_gen, y_gen, parm, obj, npop, c_idx, sc, sm, fused=fused)
    assert int(sc) == 7 and int(sm) == 11


def test_tournament_pool_raises_beyond_gate(dev):
    from dmosopt_amd import _hipops

    N = 2049
    population = torch.rand(N, 4, device=dev)
    rank = torch.zeros(N, dtype=torch.long, device=dev)
    with pytest.raises(RuntimeError, match="2048"):
        _hipops.tournament_pool(population, rank, 100, 0.5, 1)


def test_transformer_joint_on_gpu(dev):
    """The FT-Transformer surrogate family (plain PyTorch) fits and
    predicts on the GPU: the joint() custom-training hook end-to-end."""
    from dmosopt_amd.models.transformer import joint

    rng = np.random.default_rng(61)
    X = rng.random((80, 4))
    Y = np.column_stack([X.sum(axis=1), (X**2).sum(axis=1)])
    C = np.column_stack([X[:, 0] - 0.3])

    class FakeOpt:
        pass

    opt_cls, obj_model, feas_model, sens_model = joint(
        FakeOpt, X, Y, C, np.zeros(4), np.ones(4), None, {},
        constraints=True, epochs=40,
    )
    mean = obj_model.evaluate(X[:10])
    assert mean.shape == (10, 2) and np.isfinite(mean).all()
    ranks = feas_model.rank(X[:10])
    assert (ranks >= 0).all() and (ranks <= 1).all()
    di = sens_model.di_dict()
    assert (di["di_mutation"] >= 1).all()


def test_variational_gp_on_gpu(dev):
    """Variational GP family on the GPU (svgp registry entry)."""
    from dmosopt_amd import config as cfg

    rng = np.random.default_rng(62)
    X = rng.random((120, 5))
    Y = np.column_stack([X.sum(axis=1), np.sin(X[:, 0] * 3)])
    cls = cfg.resolve(cfg.surrogate_registry, "svgp")
    sm = cls(X, Y, 5, 2, np.zeros(5), np.ones(5), device="cuda", n_iter=60)
    mean, var = sm.predict(rng.random((16, 5)))
    assert mean.shape == (16, 2) and np.isfinite(mean).all()
    assert (np.asarray(var) >= 0).all()


def test_smpso_velocity_kernel_matches_torch(dev):
    from dmosopt_amd import _hipops

    g = torch.Generator().manual_seed(71)
    n, d = 200, 12
    pos = torch.rand(n, d, generator=g).float().to(dev)
    vel = (torch.rand(n, d, generator=g).float().to(dev) - 0.5) * 0.2
    L1 = torch.rand(d, generator=g).float().to(dev)
    L2 = torch.rand(d, generator=g).float().to(dev)
    xlb = torch.zeros(d).float().to(dev)
    xub = torch.ones(d).float().to(dev)
    w, a1, a2, chi = 0.3, 1.9 * 0.7, 2.1 * 0.2, 0.73
    got = _hipops.smpso_velocity(pos, vel, L1, L2, xlb, xub, w, a1, a2, chi)
    delta = (xub - xlb) / 2.0
    want = (
        (w * vel + a1 * (L1[None, :] - pos) + a2 * (L2[None, :] - pos)) * chi
    ).clamp(-delta, delta)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6)


def test_smpso_gpu_e2e_uses_kernel(dev):
    from dmosopt_amd.moea.smpso import SMPSOOptimizer
    from dmosopt_amd.models.model import Model

    rng = np.random.default_rng(72)

    class Obj:
        def evaluate(self, x):
            x = np.asarray(x)
            return np.column_stack([x.sum(1), (1 - x).sum(1)])

    opt = SMPSOOptimizer(popsize=20, nInput=6, nOutput=2, model=Model(objective=Obj()))
    opt.set_device(dev)
    bounds = np.stack([np.zeros(6), np.ones(6)], axis=1)
    x0 = opt.generate_initial(bounds, rng)
    y0 = Obj().evaluate(x0)
    opt.initialize_strategy(x0, y0, bounds, rng)
    for _ in range(3):
        xg, st = opt.generate()
        yg = Obj().evaluate(xg.cpu().numpy() if isinstance(xg, torch.Tensor) else xg)
        opt.update(xg, torch.as_tensor(yg, dtype=torch.float32, device=dev), st)
    px, py = opt.population_objectives
    assert torch.isfinite(torch.as_tensor(np.asarray(py) if not isinstance(py, torch.Tensor) else py.cpu().numpy())).all()


def test_generation_spawn_matches_split_composition(dev):
    """generation_spawn (one binding call) must equal tournament_pool +
    variation_events composed manually with the same seeds — locks the
    fused production route against the pieces it fuses."""
    from dmosopt_amd import _hipops

    torch.manual_seed(11)
    N, d, poolsize, C, M = 300, 12, 150, 80, 20
    population = torch.rand(N, d, device=dev)
    rank = torch.sort(torch.randint(0, 9, (N,), device=dev)).values.long()
    total = 2 * C + M
    perm = torch.randperm(total, device=dev)
    ci = perm[: 2 * C].contiguous()
    mi = perm[2 * C :].contiguous()
    g = torch.Generator().manual_seed(5)
    i1 = torch.randint(0, poolsize, (C,), generator=g).to(dev)
    i2 = (i1 + 1 + torch.randint(0, poolsize - 1, (C,), generator=g).to(dev)) % poolsize
    im = torch.randint(0, poolsize, (M,), generator=g).to(dev)
    di_c = torch.full((d,), 1.0, device=dev)
    di_m = torch.full((d,), 20.0, device=dev)
    lo = torch.zeros(d, device=dev)
    hi = torch.ones(d, device=dev)
    st, s1, s2 = 777, 1234, 9876

    pool, _ = _hipops.tournament_pool(population.contiguous(), rank.contiguous(),
                                      poolsize, 0.5, st)
    want = _hipops.variation_events(pool.contiguous(), ci, mi, i1, i2, im,
                                    di_c, di_m, lo, hi, 0.1, s1, s2)
    got = _hipops.generation_spawn(population.contiguous(), rank.contiguous(),
                                   poolsize, 0.5, st, ci, mi, i1, i2, im,
                                   di_c, di_m, lo, hi, 0.1, s1, s2,
                                   rank_sorted=True)
    assert torch.equal(got, want)


def test_large_pop_epoch_bitwise_deterministic(dev):
    """pop=1600 epoch (the 8-GPU weak-scaling regime) twice with the same
    seed: final front must be BIT-identical — locks the large-N kernels
    (cooperative peel atomics, wide-block bitonics, event-decoded
    variation) to run-to-run determinism, the replicated-control-flow
    invariant."""
    import bench as B

    X, Y = B.make_archive(seed=9)
    outs = []
    for _ in range(2):
        x_res, y_res, hv = B.one_epoch(X, Y, 1600, 0, 1, dev, seed=77, n_gen=30)
        outs.append((x_res.cpu().clone(), y_res.cpu().clone(), float(hv)))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert outs[0][2] == outs[1][2]
