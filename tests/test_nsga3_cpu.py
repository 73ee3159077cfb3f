"""NSGA-III on the CPU: reference directions, the closed-form niching against
the textbook loop, normalisation, the whole selection against a float64 numpy
transcription of the specification, the optimizer protocol and a quality gate
against NSGA-II. The oracle and the case builders are shared with
tests/test_nsga3.py."""

import numpy as np
import pytest
import torch

from dmosopt_amd.ops import torch_ref


# ------------------------------------------------------------------- oracle
def oracle_normalize(Y, rank, K):
    """(ideal, scale, l, used_solve) in float64 numpy, loops as in the text."""
    Y = np.asarray(Y, dtype=np.float64)
    rank = np.asarray(rank)
    N, m = Y.shape
    K = min(K, N)
    l = 0
    while (rank <= l).sum() < K:
        l += 1
    S = rank <= l
    F0 = np.flatnonzero(rank == 0)
    z = Y[S].min(axis=0)
    T = Y - z
    ext = []
    for j in range(m):
        w = np.full(m, 1e-6)
        w[j] = 1.0
        best, bi = None, -1
        for i in F0:
            v = (T[i] / w).max()
            if best is None or v < best:
                best, bi = v, i
        ext.append(bi)
    s, used = None, False
    if len(set(ext)) == m:
        try:
            a = np.linalg.solve(T[ext], np.ones(m))
            if np.isfinite(a).all() and (a > 0).all():
                s, used = 1.0 / a, True
        except np.linalg.LinAlgError:
            pass
    if s is None:
        s = T[F0].max(axis=0)
    s = np.where(s < 1e-6, 1.0, s)
    return z, s, l, used


def oracle_distances(Y, z, s, Z):
    """(N, H) perpendicular distances of the normalised rows, float64."""
    yp = (np.asarray(Y, dtype=np.float64) - z) / s
    zh = np.asarray(Z, dtype=np.float64)
    zh = zh / np.sqrt((zh * zh).sum(axis=1, keepdims=True))
    D = np.empty((yp.shape[0], zh.shape[0]))
    step = max(1, (1 << 21) // zh.size)  # bounded (rows, H, m) blocks
    for i in range(0, yp.shape[0], step):
        y = yp[i:i + step]
        res = y[:, None, :] - (y @ zh.T)[:, :, None] * zh[None, :, :]
        D[i:i + step] = np.sqrt((res * res).sum(axis=2))
    return D


def oracle_select(Y, K, Z, dir_prio, row_prio):
    """The whole specification in float64 numpy with the textbook loop."""
    Yt = torch.as_tensor(np.asarray(Y, dtype=np.float64))
    rank = torch_ref.pareto_rank(Yt).numpy()
    z, s, l, used = oracle_normalize(Y, rank, K)
    D = oracle_distances(Y, z, s, Z)
    S = rank <= l
    niche = np.where(S, D.argmin(axis=1), -1)
    dist = np.where(S, D.min(axis=1), np.inf)
    perm = torch_ref.nsga3_niche_sequential(
        torch.as_tensor(rank), torch.as_tensor(niche), torch.as_tensor(dist), K,
        Z.shape[0], torch.as_tensor(dir_prio), torch.as_tensor(row_prio),
    ).numpy()
    return dict(rank=rank, ideal=z, scale=s, l=l, niche=niche, dist=dist, perm=perm,
                used_solve=used)


def make_case(N, m, H, seed, kind):
    """(Y (N, m), Z (H, m), dir_prio, row_prio), float64 arrays of float32
    values. ``continuous``: a few fronts of a noisy sphere octant, and rows
    0..m-1 the axis extremes, which make the intercept system diagonal (well
    conditioned in any precision). ``grid``: a coarse grid, duplicate-heavy
    with many exact ties, under a first front of two rows: a diagonal system
    at m = 2, coinciding extremes (the fallback) beyond."""
    g = np.random.default_rng(seed)
    if kind == "grid":
        Y = g.integers(0, 6, (N, m)).astype(np.float64) / 4.0
        Y[0] = 0.0
        Y[0, 0] = -0.5
        Y[N - 1] = -0.5
        Y[N - 1, 0] = 0.0
    else:
        U = np.abs(g.normal(size=(N, m))) + 0.05
        U /= np.sqrt((U * U).sum(axis=1, keepdims=True))
        Y = U * (1.0 + 0.5 * g.random((N, 1))) * (1.0 + np.arange(m))[None, :]
        for j in range(min(m, N)):
            Y[j] = 0.001 * (1.0 + np.arange(m))
            Y[j, j] = 0.9 * (1.0 + j)
    Z = g.random((H, m)) + 0.01
    Z[: min(m, H)] = np.eye(m)[: min(m, H)] + 1e-3
    f32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    return f32(Y), f32(Z), g.permutation(H), g.permutation(N)


# ------------------------------------------------------ reference directions
def test_reference_directions():
    from dmosopt_amd.moea.nsga3 import default_partitions, reference_directions

    Z = reference_directions(3, 2)
    assert np.array_equal(Z, np.array([
        [0.0, 0.0, 1.0], [0.0, 0.5, 0.5], [0.0, 1.0, 0.0],
        [0.5, 0.0, 0.5], [0.5, 0.5, 0.0], [1.0, 0.0, 0.0]]))
    for (m, p), H in {(2, 199): 200, (3, 12): 91, (5, 5): 126, (8, (3, 2)): 156}.items():
        Z = reference_directions(m, p)
        assert Z.shape == (H, m)
        assert np.allclose(Z.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert (Z >= 0).all()
    assert [default_partitions(m, 200) for m in (2, 3, 5)] == [199, 18, 5]


# ------------------------------------------------------------------ niching
def test_niche_closed_form_equals_the_loop():
    """3000 seeded cases: H 1..12, N 1..40, quantised distances (ties), zero
    and positive niche counts, directions that run out of candidates, R = 1
    and R = |F| forced on a share of the cases."""
    g = np.random.default_rng(2024)
    seen_R1 = seen_RF = seen_exhaust = seen_rho0 = seen_rhopos = 0
    for case in range(3000):
        H, N = int(g.integers(1, 13)), int(g.integers(1, 41))
        n_fronts = int(g.integers(1, 5))
        rank = np.sort(g.integers(0, n_fronts, N))
        rank = np.unique(rank, return_inverse=True)[1]  # fronts 0..max, none empty
        g.shuffle(rank)
        niche = g.integers(0, max(1, int(g.integers(1, H + 1))), N)
        dist = g.integers(0, 4, N).astype(np.float64) / 4.0
        counts = np.bincount(rank)
        cum = np.cumsum(counts)
        l = int(g.integers(0, len(counts)))
        before = int(cum[l] - counts[l])
        mode = case % 3
        if mode == 0:
            K = before + 1  # R = 1
        elif mode == 1:
            K = int(cum[l])  # R = |F|
        else:
            K = before + int(g.integers(1, counts[l] + 1))
        if case % 7 == 0:
            K = N + int(g.integers(0, 3))  # N <= K
        args = (torch.as_tensor(rank), torch.as_tensor(niche), torch.as_tensor(dist), K, H,
                torch.as_tensor(g.permutation(H)), torch.as_tensor(g.permutation(N)))
        want = torch_ref.nsga3_niche_sequential(*args)
        got = torch_ref.nsga3_niche(*args)
        assert torch.equal(got, want), (case, rank, niche, dist, K)
        le = int(np.searchsorted(cum, min(K, N)))  # the front the case ends in
        F = rank == le
        R = min(K, N) - int((rank < le).sum())
        seen_R1 += R == 1
        seen_RF += R == F.sum()
        rho = np.bincount(niche[rank < le], minlength=H)
        seen_rho0 += (rho[niche[F]] == 0).any()
        seen_rhopos += (rho[niche[F]] > 0).any()
        seen_exhaust += R > len(set(niche[F]))
    assert min(seen_R1, seen_RF, seen_exhaust, seen_rho0, seen_rhopos) > 100


# ------------------------------------------------------------ normalisation
def _rank(Y):
    return torch_ref.pareto_rank(Y)


def test_normalize_known_intercepts():
    """Rows on the plane x/2 + y/3 + z/4 = 1 through the axis points: the
    ideal is the origin and the scale the intercepts."""
    P = np.array([[2, 0, 0], [0, 3, 0], [0, 0, 4], [1, 1.5, 0], [0, 1.5, 2],
                  [1, 0, 2], [0.5, 0.75, 2], [1, 0.75, 1]], dtype=np.float64)
    back = P[3:] + 0.5  # a dominated second front
    Y = torch.as_tensor(np.vstack([back, P]))
    rank = _rank(Y)
    assert int((rank == 0).sum()) == 8
    for dt, tol in ((torch.float64, 1e-12), (torch.float32, 1e-5)):
        ideal, scale, l = torch_ref.nsga3_normalize(Y.to(dt), rank, 6)
        assert int(l) == 0
        assert torch.equal(ideal, torch.zeros(3, dtype=dt))
        assert torch.allclose(scale, torch.tensor([2.0, 3.0, 4.0], dtype=dt), rtol=tol, atol=0)


def test_normalize_fallbacks():
    # a first front of two rows under three objectives: two extremes coincide
    Y = torch.tensor([[0.0, 2.0, 1.0], [3.0, 0.0, 0.5], [4.0, 3.0, 2.0], [5.0, 2.5, 1.5],
                      [3.5, 2.5, 3.0]], dtype=torch.float64)
    rank = _rank(Y)
    assert int((rank == 0).sum()) == 2
    ideal, scale, l = torch_ref.nsga3_normalize(Y, rank, 4)
    assert int(l) == 1
    assert torch.equal(ideal, torch.tensor([0.0, 0.0, 0.5], dtype=torch.float64))
    # the first front's column maximum of Y - ideal
    assert torch.equal(scale, torch.tensor([3.0, 2.0, 0.5], dtype=torch.float64))
    z, s, lo, used = oracle_normalize(Y.numpy(), rank.numpy(), 4)
    assert not used and np.array_equal(s, scale.numpy()) and lo == 1
    # a constant column: singular solve, zero span, scale 1
    Y = torch.tensor([[0.0, 1.0, 7.0], [1.0, 0.0, 7.0], [0.5, 0.5, 7.0]], dtype=torch.float64)
    ideal, scale, l = torch_ref.nsga3_normalize(Y, _rank(Y), 2)
    assert float(scale[2]) == 1.0 and float(ideal[2]) == 7.0
    assert torch.isfinite(scale).all() and (scale > 0).all()


# ---------------------------------------------------------------- selection
def _check_select(Y, K, Z, dp, rp):
    want = oracle_select(Y, K, Z, dp, rp)
    Yt = torch.as_tensor(Y)
    X = torch.arange(Y.shape[0], dtype=torch.float64)[:, None] * torch.ones(1, 2, dtype=torch.float64)
    parm, obj, rank, perm, ideal, scale, niche, dist = torch_ref.nsga3_select(
        X, Yt, K, torch.as_tensor(Z), torch.as_tensor(dp), torch.as_tensor(rp))
    assert np.array_equal(ideal.numpy(), want["ideal"])
    assert np.allclose(scale.numpy(), want["scale"], rtol=1e-9, atol=0)
    assert np.array_equal(niche.numpy(), want["niche"])
    assert np.allclose(dist.numpy(), want["dist"], rtol=1e-9, atol=1e-12)
    assert np.array_equal(perm.numpy(), want["perm"])
    assert perm.shape[0] == min(K, Y.shape[0]) == len(set(perm.tolist()))
    assert torch.equal(parm, X[perm]) and torch.equal(obj, Yt[perm])
    assert np.array_equal(rank.numpy(), want["rank"][perm.numpy()])
    return want


@pytest.mark.parametrize("N,K,m,H", [(64, 32, 3, 15), (130, 64, 5, 126)])
def test_select_continuous(N, K, m, H):
    want = _check_select(*(lambda c: (c[0], K, c[1], c[2], c[3]))(make_case(N, m, H, N, "continuous")))
    assert want["used_solve"]


def test_select_duplicate_heavy():
    Y, Z, dp, rp = make_case(96, 3, 28, 5, "grid")
    Y[40:] = Y[:56]  # whole rows repeated
    _check_select(Y, 48, Z, dp, rp)


def test_select_all_nondominated():
    """One front: P is empty and every survivor is a niching pick."""
    g = np.random.default_rng(3)
    a = np.sort(g.random(50))
    Y = np.column_stack([a, 1.0 - a, 0.5 + 0.0 * a])
    from dmosopt_amd.moea.nsga3 import reference_directions

    Z = reference_directions(3, 5)
    want = _check_select(Y, 20, Z, g.permutation(Z.shape[0]), g.permutation(50))
    assert want["l"] == 0 and (want["rank"] == 0).all()


def test_select_exact_fit_and_small_population():
    Y, Z, dp, rp = make_case(64, 3, 15, 11, "continuous")
    rank = torch_ref.pareto_rank(torch.as_tensor(Y)).numpy()
    K = int((rank <= 1).sum())  # the first two fronts fill K exactly
    assert 0 < K < 64
    want = _check_select(Y, K, Z, dp, rp)
    assert set(want["perm"].tolist()) == set(np.flatnonzero(rank <= 1).tolist())
    for K in (64, 100):  # N <= K: every row survives
        want = _check_select(Y, K, Z, dp, rp)
        assert sorted(want["perm"].tolist()) == list(range(64))


# ------------------------------------------------------- optimizer protocol
def test_registered():
    from dmosopt_amd.config import optimizer_registry, resolve
    from dmosopt_amd.moea.nsga3 import NSGA3Optimizer

    assert resolve(optimizer_registry, "nsga3") is NSGA3Optimizer


@pytest.mark.parametrize("m", [3, 5])
def test_duplicate_heavy_two_generations(m):
    """The step of test_many_objectives_duplicate_heavy."""
    from dmosopt_amd.config import optimizer_registry, resolve

    rng = np.random.default_rng(0)
    cls = resolve(optimizer_registry, "nsga3")
    d, pop = 4, 12
    opt = cls(popsize=pop, nInput=d, nOutput=m)
    bounds = np.column_stack([np.zeros(d), np.ones(d)])
    x = rng.random((pop, d))
    x[: pop // 2] = x[0]
    y = np.column_stack([x.sum(1) + j * 0.1 for j in range(m)])
    opt.initialize_strategy(x, y, bounds, np.random.default_rng(1))
    for _ in range(2):
        xg, gs = opt.generate()
        xgn = xg.cpu().numpy()
        yg = np.column_stack([xgn.sum(1) + j * 0.1 for j in range(m)])
        opt.update(xgn, yg, gs)
    px, py = opt.population_objectives
    assert px.shape == (pop, d) and py.shape == (pop, m)
    assert np.isfinite(py.cpu().numpy()).all()
    assert opt.state.niche.shape == (pop,) and int(opt.state.niche.min()) >= 0
    assert opt.native_generations_eligible(None) is False


def test_ref_dirs_validation():
    from dmosopt_amd.moea.nsga3 import NSGA3Optimizer

    mk = lambda Z: NSGA3Optimizer(popsize=8, nInput=3, nOutput=3, ref_dirs=Z)  # noqa: E731
    for bad in (np.ones(3), np.array([[1.0, -0.1, 0.2]]), np.array([[1.0, np.nan, 0.2]]),
                np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            mk(bad)
    opt = mk(np.array([[1.0, 1.0], [1.0, 2.0]]))  # two columns, three objectives
    x = np.random.default_rng(0).random((8, 3))
    with pytest.raises(ValueError):
        opt.initialize_strategy(x, x.copy(), np.column_stack([np.zeros(3), np.ones(3)]),
                                np.random.default_rng(1))
    # the user's own directions steer the survivors
    Z = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 4.0]])
    opt = mk(Z)
    opt.initialize_strategy(x, x.copy(), np.column_stack([np.zeros(3), np.ones(3)]),
                            np.random.default_rng(1))
    assert opt.reference_dirs(opt.state.population_obj).shape == (2, 3)
    assert set(opt.state.niche.tolist()) <= {0, 1}


def _dtlz2(x, m=3):
    g = ((x[:, m - 1:] - 0.5) ** 2).sum(axis=1)
    f = np.tile((1.0 + g)[:, None], (1, m))
    for j in range(m):
        f[:, j] *= np.prod(np.cos(0.5 * np.pi * x[:, : m - 1 - j]), axis=1)
        if j > 0:
            f[:, j] *= np.sin(0.5 * np.pi * x[:, m - 1 - j])
    return f


def _run(name, seed, gens=60, pop=92, d=7, m=3, **kw):
    from dmosopt_amd.config import optimizer_registry, resolve

    opt = resolve(optimizer_registry, name)(popsize=pop, nInput=d, nOutput=m, **kw)
    bounds = np.column_stack([np.zeros(d), np.ones(d)])
    rng = np.random.default_rng(seed)
    x = opt.generate_initial(bounds, rng)
    opt.initialize_strategy(x, _dtlz2(x, m), bounds, rng)
    for _ in range(gens):
        xg, gs = opt.generate()
        xgn = xg.cpu().numpy()
        opt.update(xgn, _dtlz2(xgn, m), gs)
    px, py = opt.population_objectives
    return px.cpu().numpy(), py.cpu().numpy()


def test_same_seed_same_population():
    a = _run("nsga3", 4, gens=5, ref_partitions=12)
    b = _run("nsga3", 4, gens=5, ref_partitions=12)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_quality_gate_against_nsga2():
    """DTLZ2, 3 objectives, d = 7, pop 92, 91 directions, 60 generations,
    seeds 0..2: median IGD against the unit-sphere points of the directions.
    Measured: nsga3 0.0251, nsga2 0.0847 (ratio 0.30)."""
    from dmosopt_amd.moea.nsga3 import reference_directions

    Z = reference_directions(3, 12)
    target = Z / np.sqrt((Z * Z).sum(axis=1, keepdims=True))

    def igd(py):
        return np.sqrt(((target[:, None, :] - py[None, :, :]) ** 2).sum(axis=2)).min(axis=1).mean()

    med3 = np.median([igd(_run("nsga3", s, ref_partitions=12)[1]) for s in range(3)])
    med2 = np.median([igd(_run("nsga2", s)[1]) for s in range(3)])
    print(f"median IGD nsga3 {med3:.4f} nsga2 {med2:.4f} ratio {med3 / med2:.3f}")
    assert med3 <= 0.5 * med2
