"""Population-op tests against independent numpy oracles.

The oracles re-derive the reference semantics (dda.py, indicators.py,
MOEA.py) directly in this file, so the library implementation is tested
against an INDEPENDENT formulation, not against itself.
"""

import numpy as np
import pytest
import torch

from dmosopt_amd import ops
from dmosopt_amd.ops import torch_ref


def brute_force_fronts(Y: np.ndarray) -> np.ndarray:
    """O(n^2 m) straightforward non-dominated sorting oracle.

    dominates(i, j): all(Y[i] <= Y[j]) and any(Y[i] < Y[j]).
    Identical rows do not dominate each other.
    """
    n = Y.shape[0]
    dominated_by = [
        [
            j
            for j in range(n)
            if j != i
            and np.all(Y[j] <= Y[i])
            and np.any(Y[j] < Y[i])
        ]
        for i in range(n)
    ]
    rank = np.full(n, -1)
    k = 0
    remaining = set(range(n))
    while remaining:
        front = [
            i for i in remaining if not any(j in remaining for j in dominated_by[i])
        ]
        for i in front:
            rank[i] = k
        remaining -= set(front)
        k += 1
    return rank


@pytest.mark.parametrize("n,m", [(30, 2), (60, 3), (100, 5), (17, 2)])
def test_pareto_rank_matches_bruteforce(n, m, rng):
    Y = rng.random((n, m))
    r = ops.pareto_rank(torch.as_tensor(Y)).numpy()
    expected = brute_force_fronts(Y)
    assert np.array_equal(r, expected)


def test_pareto_rank_with_duplicates(rng):
    Y = rng.random((20, 3))
    Y = np.vstack([Y, Y[:5]])  # duplicate rows
    r = ops.pareto_rank(torch.as_tensor(Y)).numpy()
    expected = brute_force_fronts(Y)
    assert np.array_equal(r, expected)
    # duplicated rows land in the same front as their originals
    assert np.array_equal(r[:5], r[20:])


def crowding_oracle(Y):
    """Reference crowding semantics (indicators.py:12-51) re-derived."""
    n, d = Y.shape
    if n == 1:
        return np.array([1.0])
    lb, ub = Y.min(0), Y.max(0)
    span = np.where(ub - lb == 0, 1.0, ub - lb)
    U = (Y - lb) / span
    D = np.zeros(n)
    for j in range(d):
        idx = np.argsort(U[:, j])
        us = U[idx, j]
        ds = np.empty(n)
        ds[0] = ds[-1] = 1.0
        for i in range(1, n - 1):
            ds[i] = us[i + 1] - us[i - 1]
        for i in range(n):
            D[idx[i]] += ds[i]
    return D


@pytest.mark.parametrize("n,m", [(2, 2), (50, 2), (80, 4)])
def test_crowding_distance(n, m, rng):
    Y = rng.random((n, m))
    d = ops.crowding_distance(torch.as_tensor(Y)).numpy()
    assert np.allclose(d, crowding_oracle(Y), atol=1e-12)


def test_lexsort_matches_numpy(rng):
    a = rng.integers(0, 5, 100).astype(float)
    b = rng.random(100)
    c = rng.integers(0, 3, 100).astype(float)
    ours = ops.lexsort([torch.as_tensor(b), torch.as_tensor(-a), torch.as_tensor(c)]).numpy()
    theirs = np.lexsort((b, -a, c))
    assert np.array_equal(ours, theirs)


def test_order_mo_sorts_by_rank_then_crowding(rng):
    Y = rng.random((40, 2))
    X = rng.random((40, 5))
    perm, rank, dists = ops.order_mo(
        torch.as_tensor(X), torch.as_tensor(Y), y_distance_metrics=["crowding"]
    )
    assert np.all(np.diff(rank.numpy()) >= 0)  # ranks nondecreasing
    # within a front, crowding distance is nonincreasing
    r = rank.numpy()
    d = dists[0].numpy()
    for k in np.unique(r):
        dk = d[r == k]
        assert np.all(np.diff(dk) <= 1e-12)


def test_sbx_crossover_bounds_and_mean(rng):
    d = 10
    p1 = torch.rand(500, d, dtype=torch.float64)
    p2 = torch.rand(500, d, dtype=torch.float64)
    di = torch.full((d,), 1.0, dtype=torch.float64)
    lo = torch.zeros(d, dtype=torch.float64)
    hi = torch.ones(d, dtype=torch.float64)
    g = torch.Generator().manual_seed(0)
    c1, c2 = ops.sbx_crossover_batch(p1, p2, di, lo, hi, generator=g)
    assert (c1 >= 0).all() and (c1 <= 1).all()
    assert (c2 >= 0).all() and (c2 <= 1).all()
    # SBX preserves the parent midpoint before clipping: c1+c2 == p1+p2
    mid_parent = (p1 + p2).mean()
    mid_child = (c1 + c2).mean()
    assert abs(mid_parent - mid_child) < 0.02


def test_polynomial_mutation_bounds(rng):
    d = 8
    p = torch.rand(300, d, dtype=torch.float64)
    di = torch.full((d,), 20.0, dtype=torch.float64)
    lo = torch.zeros(d, dtype=torch.float64)
    hi = torch.ones(d, dtype=torch.float64)
    g = torch.Generator().manual_seed(3)
    child = ops.polynomial_mutation_batch(p, di, lo, hi, mutation_rate=0.5, generator=g)
    assert (child >= 0).all() and (child <= 1).all()
    # high di keeps children near parents
    assert (child - p).abs().mean() < 0.1


def test_get_duplicates_marks_earlier_row(rng):
    X = rng.random((10, 4))
    X[7] = X[2]  # pair (2, 7): later index marked (triu-mask semantics)
    dup = ops.get_duplicates(torch.as_tensor(X)).numpy()
    assert dup[7] and not dup[2]
    assert dup.sum() == 1


def test_remove_worst_keeps_best_front(rng):
    X = torch.rand(60, 4, dtype=torch.float64)
    Y = torch.rand(60, 2, dtype=torch.float64)
    x2, y2, rank, perm = ops.remove_worst(X, Y, 20, y_distance_metrics=["crowding"])
    assert x2.shape == (20, 4)
    full_rank = ops.pareto_rank(Y).numpy()
    kept_ranks = full_rank[perm.numpy()]
    dropped = np.setdiff1d(np.arange(60), perm.numpy())
    assert kept_ranks.max() <= full_rank[dropped].min() or len(dropped) == 0


def test_filter_samples_nan_remove():
    y = torch.tensor([[1.0, 2.0], [float("nan"), 1.0], [3.0, 4.0]])
    x = torch.arange(3).double()[:, None]
    y2, x2 = ops.filter_samples(y, x, nan="remove")
    assert y2.shape[0] == 2 and x2.shape[0] == 2


def test_tournament_selection_distribution(rng):
    # best-ranked individuals must be selected more often
    pop = 20
    metrics = [torch.arange(pop, dtype=torch.float64)]  # identity rank
    counts = np.zeros(pop)
    for _ in range(200):
        idx = ops.tournament_selection(pop, 5, metrics, rng).numpy()
        counts[idx] += 1
    assert counts[:5].sum() > counts[15:].sum()


def test_agemoea_survival_matches_reference_greedy(rng):
    """Incremental 2-NN greedy selection == reference O(m^3) formulation
    (AGEMOEA.py:389-442)."""
    from dmosopt_amd.moea.agemoea import (
        find_corner_solutions, get_geometry, minkowski_matrix, normalize_front,
        survival_score,
    )

    y = rng.random((40, 3)) + 0.1
    front = np.arange(40)
    ideal = y.min(axis=0)

    # reference-style oracle
    yf = y - ideal
    extreme = find_corner_solutions(yf)
    normalization = normalize_front(yf, extreme)
    yn = yf / normalization
    p = get_geometry(yn, extreme)
    m = 40
    crowd = np.zeros(m)
    crowd[extreme] = np.inf
    selected = np.zeros(m, dtype=bool)
    selected[extreme] = True
    nn_norm = np.power(np.power(np.abs(yn), p).sum(axis=1), 1.0 / p)
    distances = minkowski_matrix(yn, yn, p) / nn_norm[:, None]
    remaining = list(np.arange(m)[~selected])
    for _ in range(m - selected.sum()):
        D_mg = distances[np.ix_(remaining, np.flatnonzero(selected))]
        if D_mg.shape[1] > 1:
            part = np.argpartition(D_mg, 1, axis=1)[:, :2]
            tmp = np.take_along_axis(D_mg, part, axis=1).sum(axis=1)
            index = int(np.argmax(tmp))
            d = tmp[index]
        else:
            index = int(D_mg[:, 0].argmax())
            d = D_mg[index, 0]
        best = remaining.pop(index)
        selected[best] = True
        crowd[best] = d

    _, _, crowd_fast = survival_score(y, front, ideal)
    finite = np.isfinite(crowd)
    assert np.allclose(crowd_fast[finite], crowd[finite], atol=1e-10)
    assert np.array_equal(np.isinf(crowd_fast), np.isinf(crowd))


def test_pareto_rank_beats_naive_reference_walltime():
    """Performance-regression gate in the reference's style
    (test_dda_performance.py / test_hv_performance.py: fast path within a
    wall-clock ratio of a reference implementation). Our vectorized DDA
    ranking must beat a pure-Python per-pair peel outright at N=512 — a
    generous inversion bound that survives noisy CI boxes."""
    import time

    rng = np.random.default_rng(11)
    Y = torch.as_tensor(rng.random((512, 3)))

    t0 = time.perf_counter()
    fast = ops.pareto_rank(Y)
    t_fast = time.perf_counter() - t0

    def naive_rank(Yn):
        n = Yn.shape[0]
        rank = np.full(n, -1)
        alive = np.ones(n, bool)
        k = 0
        while alive.any():
            front = []
            for j in np.flatnonzero(alive):
                dominated = False
                for i in np.flatnonzero(alive):
                    if i == j:
                        continue
                    if np.all(Yn[i] <= Yn[j]) and np.any(Yn[i] < Yn[j]):
                        dominated = True
                        break
                if not dominated:
                    front.append(j)
            for j in front:
                rank[j] = k
                alive[j] = False
            k += 1
        return rank

    t0 = time.perf_counter()
    want = naive_rank(Y.numpy())
    t_naive = time.perf_counter() - t0

    assert np.array_equal(fast.numpy(), want)
    assert t_fast < t_naive, (t_fast, t_naive)


def test_packed_rank_crowding_key_orders_like_lexsort():
    """The GPU survivor-selection path sorts ONE packed int64 key
    (rank << 32 | ~float32_bits(crowding)) instead of two stable sorts;
    this guards the bit-trick's ordering equivalence (non-negative IEEE
    floats compare like their bit patterns; +inf boundary points first
    within a rank; ties resolved by index exactly like np.lexsort)."""
    torch.manual_seed(0)
    N = 600
    rank = torch.randint(0, 12, (N,))
    d = torch.rand(N).double() * 10
    d[torch.randint(0, N, (25,))] = float("inf")
    d[torch.randint(0, N, (10,))] = 0.0

    df = torch.nan_to_num(
        d.float().clamp_min(0.0), nan=0.0, posinf=float(torch.finfo(torch.float32).max)
    )
    bits = df.view(torch.int32).to(torch.int64)
    key = (rank.to(torch.int64) << 32) | ((0x7FFFFFFF - bits) & 0xFFFFFFFF)
    perm_fast = torch.argsort(key, stable=True)

    perm = torch.arange(N)
    for k in [(-df.double()), rank.double()]:  # np.lexsort order: last primary
        order = torch.argsort(k[perm], stable=True)
        perm = perm[order]
    assert torch.equal(perm_fast, perm)


def test_epsilon_sort_box_semantics():
    """Epsilon-box archive (reference MOEA.py:470-595 semantics): box
    dominance, same-box corner-distance replacement, eviction."""
    from dmosopt_amd.moea.epsilon import EpsilonSort

    s = EpsilonSort([1.0, 1.0])
    s.sortinto(np.array([2.3, 2.3]), tagalong="a")   # box (2,2)
    s.sortinto(np.array([2.6, 2.6]), tagalong="b")   # same box, farther corner
    assert s.tagalongs == ["a"]                      # a kept (closer to corner)
    s.sortinto(np.array([2.1, 2.1]), tagalong="c")   # same box, closer
    assert s.tagalongs == ["c"]
    s.sortinto(np.array([0.5, 3.5]), tagalong="d")   # box (0,3): nondominated
    assert set(s.tagalongs) == {"c", "d"}
    s.sortinto(np.array([0.5, 0.5]), tagalong="e")   # box (0,0): dominates both
    assert s.tagalongs == ["e"]
    s.sortinto(np.array([5.0, 5.0]), tagalong="f")   # dominated by e's box
    assert s.tagalongs == ["e"]


def test_epsilon_get_best_selects_archive():
    from dmosopt_amd.core.engine import epsilon_get_best

    rng = np.random.default_rng(4)
    x = rng.random((60, 3))
    f1 = rng.random(60)
    y = np.column_stack([f1, 1.0 - f1 + 0.02 * rng.standard_normal(60)])
    bx, by, _, _, eps = epsilon_get_best(x, y, None, None, epsilons=[0.1, 0.1])
    assert by.shape[0] > 1
    # archive members pairwise non-dominated at epsilon-box resolution
    boxes = np.floor(by / np.asarray(eps))
    for i in range(len(boxes)):
        for j in range(len(boxes)):
            if i == j:
                continue
            assert not (
                (boxes[i] <= boxes[j]).all() and (boxes[i] < boxes[j]).any()
            )


def test_ops_degenerate_shapes():
    """Empty and single-row populations must not crash any ranking op."""
    assert ops.pareto_rank(torch.zeros(0, 2)).shape == (0,)
    assert int(ops.pareto_rank(torch.zeros(1, 2))[0]) == 0
    assert ops.crowding_distance(torch.zeros(1, 2)).shape == (1,)
    assert ops.get_duplicates(torch.zeros(0, 3)).shape == (0,)
    assert ops.lexsort([torch.zeros(0)]).shape == (0,)
    # identical rows: same rank, neither dominates the other
    Y = torch.ones(4, 2)
    assert torch.equal(ops.pareto_rank(Y), torch.zeros(4, dtype=torch.long))
    # single objective column: total order by value
    y1 = torch.tensor([[3.0], [1.0], [2.0]])
    assert ops.pareto_rank(y1).tolist() == [2, 0, 1]


def test_nu_arg_maps_rbf_to_zero():
    assert ops._nu_arg(None) == 0.0
    assert ops._nu_arg(float("inf")) == 0.0
    for nu in (0.5, 1.5, 2.5):
        assert ops._nu_arg(nu) == nu
    assert isinstance(ops._nu_arg(2.5), float)
