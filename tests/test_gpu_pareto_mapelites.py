"""K7 (`domination_counts`, `pareto_ranks`) and K9 (`mapelites_assign`)
against references written from the definitions.

Every assertion is an equality of integer or boolean outputs
(`torch.equal` / `np.array_equal`); there is no tolerance in this module.

* `ref_counts`, `ref_rank`: numpy float64. `a` dominates `b` when `a >= b`
  in every objective and `a > b` in one. `ref_counts[j]` is the number of
  rows dominating `j`; `ref_rank[j]` is 0 when nothing dominates `j`, else
  `1 + max(ref_rank[i])` over the rows `i` dominating `j`, filled in order
  of increasing `ref_counts` (a dominator has strictly fewer dominators).
  That is the peel's front index without a peel.
* `ref_assign`: per cell, the lowest index among the rows inside the box
  (`lo <= x <= hi` in every feature, NaN never inside) that attain the
  largest utility, -inf included; `valid` says whether any row is inside.
* fp16, bf16 and fp32 inputs are judged on their exactly upcast float64
  values, fp64 inputs on the fp64 values themselves.

The unmarked tests run the references against `_compute_pareto_ranks_eager`
and against the eager branch of `MAPElites._assign_cells` on the same case
table at float64, so the references are proven on the CPU before they judge
the kernels, and the CPU path is pinned to the same answers.

The GPU tests then compare the kernels with the references: every data kind
and shape of the table, the four dtypes, strided views, repeated calls, the
early stop (`min_assigned`), `take_best` / `argsort` end to end, the
MAP-Elites edge cases through the kernel and through
`MAPElites._assign_cells`, and empty inputs (which must return before any
launch and leave no error behind).
"""

import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs ROCm GPU")


@pytest.fixture(scope="module")
def C():
    import evotorch_amd._C as _C

    return _C


# ---------------------------------------------------------------------------
# 1. references
# ---------------------------------------------------------------------------


def ref_dominates(a, b):
    """a dominates b: no worse anywhere, strictly better somewhere."""
    with np.errstate(invalid="ignore"):
        return bool(np.all(a >= b) and np.any(a > b))


def ref_domination(utils):
    """dom[i, j] = ref_dominates(utils[i], utils[j]) for all pairs at once."""
    u = np.asarray(utils, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ge = (u[:, None, :] >= u[None, :, :]).all(axis=-1)
        gt = (u[:, None, :] > u[None, :, :]).any(axis=-1)
    return ge & gt


def ref_counts(utils):
    return ref_domination(utils).sum(axis=0).astype(np.int64)


def ref_rank(utils):
    dom = ref_domination(utils)
    counts = dom.sum(axis=0)
    rank = np.full(dom.shape[0], -1, dtype=np.int64)
    for j in np.argsort(counts, kind="stable"):
        above = rank[dom[:, j]]
        assert (above >= 0).all()  # every dominator was ranked before j
        rank[j] = 0 if above.size == 0 else 1 + above.max()
    return rank


def ref_assign(grid, feats, utils):
    grid = np.asarray(grid, dtype=np.float64)
    feats = np.asarray(feats, dtype=np.float64)
    utils = np.asarray(utils, dtype=np.float64)
    cells = grid.shape[0]
    best = np.zeros(cells, dtype=np.int64)
    valid = np.zeros(cells, dtype=bool)
    for c in range(cells):
        with np.errstate(invalid="ignore"):
            inside = ((feats >= grid[c, :, 0]) & (feats <= grid[c, :, 1])).all(axis=1)
        rows = np.flatnonzero(inside)
        if rows.size:
            u = utils[rows]
            best[c] = rows[u == u.max()][0]
            valid[c] = True
    return best, valid


# ---------------------------------------------------------------------------
# 2. the Pareto case table
# ---------------------------------------------------------------------------

KINDS = ["randn", "grid4", "dup", "equal", "chain", "anti", "nanrows", "straddle"]
SIZES_N = [1, 2, 255, 256, 257, 513]  # around the 256-thread block
SIZES_M = [1, 2, 3, 16, 17, 20]  # 16 = kMaxObjCache: 17 and 20 take the uncached path
CHAIN_N = [15, 16, 17, 32, 33]  # around the peel batch of 16 fronts


def _shapes(kind):
    if kind == "anti":
        return [(n, 2) for n in SIZES_N]
    return [(n, 2) for n in SIZES_N] + [(257, m) for m in SIZES_M if m != 2]


TABLE = [(kind, n, m) for kind in KINDS[:7] for (n, m) in _shapes(kind)]
TABLE += [("chain", n, m) for n in CHAIN_N for m in (2, 17)]
STRADDLE = [("straddle", n, m) for (n, m) in [(2, 2), (256, 2), (257, 3), (257, 17)]]
DTYPE_TABLE = [(kind, n, m) for kind in ("randn", "grid4", "nanrows") for (n, m) in [(256, 2), (257, 3), (257, 17)]]


@functools.lru_cache(maxsize=None)
def _utils(kind, n, m, dtype=torch.float32):
    """(n, m) utilities of one case, computed once (callers must not modify
    them). Every kind but `randn`/`nanrows` holds small integers, exact in
    every dtype."""
    g = torch.Generator().manual_seed(100000 * KINDS.index(kind) + 100 * n + m)
    if kind == "randn":
        u = torch.randn(n, m, generator=g, dtype=torch.float64)
    elif kind == "grid4":
        u = torch.randint(0, 4, (n, m), generator=g).to(torch.float64)
    elif kind == "dup":
        distinct = torch.randint(0, 4, (8, m), generator=g).to(torch.float64)
        u = distinct[torch.randint(0, 8, (n,), generator=g)]
    elif kind == "equal":
        u = torch.full((n, m), 1.25, dtype=torch.float64)
    elif kind == "chain":
        u = torch.arange(n, dtype=torch.float64).unsqueeze(1).repeat(1, m)
    elif kind == "anti":
        assert m == 2
        k = torch.randperm(n, generator=g).to(torch.float64)
        u = torch.stack([k, -k], dim=1)
    elif kind == "nanrows":
        u = torch.randn(n, m, generator=g, dtype=torch.float64)
        for r in sorted({0, n // 3, n - 1}):
            u[r, r % m] = float("nan")
    elif kind == "straddle":
        # ties in fp32 that are none in fp64: integers 1..4 (so that the
        # offset is below fp32 resolution) plus k * 2**-40 on some entries
        assert dtype == torch.float64
        u = torch.randint(1, 5, (n, m), generator=g).to(torch.float64)
        k = torch.randint(1, 4, (n, m), generator=g).to(torch.float64)
        on = torch.rand(n, m, generator=g, dtype=torch.float64) < 0.4
        on[0, 0] = True
        u = u + torch.where(on, k, torch.zeros_like(k)) * 2.0**-40
        assert not torch.equal(u, u.float().double())
    else:
        raise ValueError(kind)
    return u.to(dtype)


@functools.lru_cache(maxsize=None)
def _reference(kind, n, m, dtype=torch.float32):
    """(ref_counts, ref_rank) on the exactly upcast values of the case."""
    u = _utils(kind, n, m, dtype).to(torch.float64).numpy()
    return ref_counts(u), ref_rank(u)


def _ids(cases):
    return ["-".join(str(x).replace("torch.", "") for x in c) for c in cases]


# ---------------------------------------------------------------------------
# 3. CPU: the references are right, and the eager path agrees with them
# ---------------------------------------------------------------------------


def test_ref_domination_is_the_definition():
    u = _utils("grid4", 40, 3).double().numpy()
    dom = ref_domination(u)
    for i in range(40):
        for j in range(40):
            assert dom[i, j] == ref_dominates(u[i], u[j])
    nan = _utils("nanrows", 12, 2).double().numpy()
    dom = ref_domination(nan)
    bad = np.isnan(nan).any(axis=1)
    assert bad.sum() >= 2
    assert not dom[bad].any() and not dom[:, bad].any()


def test_ref_rank_known_answers():
    for n in CHAIN_N:
        counts, rank = _reference("chain", n, 2)
        assert np.array_equal(rank, n - 1 - np.arange(n))
        assert np.array_equal(counts, n - 1 - np.arange(n))
    counts, rank = _reference("equal", 257, 3)
    assert not counts.any() and not rank.any()
    counts, rank = _reference("anti", 513, 2)
    assert not counts.any() and not rank.any()
    # fp64 separates what fp32 ties: [1, 0] and [1 + 1e-12, 0]
    u = np.array([[1.0, 0.0], [1.0 + 1e-12, 0.0]])
    assert np.array_equal(ref_rank(u), [1, 0])
    assert np.array_equal(ref_rank(u.astype(np.float32)), [0, 0])


@pytest.mark.parametrize("case", TABLE + STRADDLE, ids=_ids(TABLE + STRADDLE))
def test_eager_ranks_match_reference(case):
    from evotorch_amd.core import _compute_pareto_ranks_eager
    from evotorch_amd.ops import domination_counts

    kind, n, m = case
    dtype = torch.float64 if kind == "straddle" else torch.float32
    u = _utils(kind, n, m, dtype).to(torch.float64)
    counts, rank = _reference(kind, n, m, dtype)
    eranks, _ = _compute_pareto_ranks_eager(u, crowdsort=False)
    assert np.array_equal(eranks.numpy(), rank)
    assert np.array_equal(domination_counts(u).numpy(), counts)


# ---------------------------------------------------------------------------
# 4. GPU: counts and ranks
# ---------------------------------------------------------------------------


def _check_kernels(C, kind, n, m, dtype):
    u = _utils(kind, n, m, dtype).to("cuda")
    counts, rank = _reference(kind, n, m, dtype)
    got_counts = C.domination_counts(u)
    got_rank = C.pareto_ranks(u, 0)
    assert got_counts.dtype == torch.int32 and got_rank.dtype == torch.int64
    assert np.array_equal(got_counts.cpu().numpy(), counts)
    assert np.array_equal(got_rank.cpu().numpy(), rank)


@gpu
@requires_gpu
@pytest.mark.parametrize("case", TABLE, ids=_ids(TABLE))
def test_kernels_match_reference(C, case):
    _check_kernels(C, *case, torch.float32)


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.bfloat16], ids=["fp64", "fp16", "bf16"])
@pytest.mark.parametrize("case", DTYPE_TABLE, ids=_ids(DTYPE_TABLE))
def test_kernels_match_reference_dtypes(C, case, dtype):
    _check_kernels(C, *case, dtype)


@gpu
@requires_gpu
@pytest.mark.parametrize("case", STRADDLE, ids=_ids(STRADDLE))
def test_kernels_compare_fp64_in_fp64(C, case):
    """Rows that tie in fp32 and differ in fp64 are ranked by their fp64
    values, as the CPU path ranks them."""
    _check_kernels(C, *case, torch.float64)


@gpu
@requires_gpu
def test_fp64_rows_below_fp32_resolution(C):
    u = torch.tensor([[1.0, 0.0], [1.0 + 1e-12, 0.0]], dtype=torch.float64, device="cuda")
    assert C.pareto_ranks(u, 0).tolist() == [1, 0]
    assert C.domination_counts(u).tolist() == [1, 0]
    from evotorch_amd.core import _compute_pareto_ranks

    ranks, crowd = _compute_pareto_ranks(u, crowdsort=True)
    cranks, ccrowd = _compute_pareto_ranks(u.cpu(), crowdsort=True)
    assert torch.equal(ranks.cpu(), cranks)
    assert torch.equal(crowd.cpu(), ccrowd)


VIEWS = [("grid4", 257, 3), ("randn", 256, 17), ("nanrows", 257, 2)]


@gpu
@requires_gpu
@pytest.mark.parametrize("case", VIEWS, ids=_ids(VIEWS))
def test_column_view_matches_contiguous_copy(C, case):
    kind, n, m = case
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(n, m + 3, generator=g)
    wide[:, 1 : 1 + m] = _utils(kind, n, m)
    wide = wide.to("cuda")
    view = wide[:, 1 : 1 + m]
    assert not view.is_contiguous()
    counts, rank = _reference(kind, n, m)
    assert torch.equal(C.pareto_ranks(view, 0), C.pareto_ranks(view.contiguous(), 0))
    assert torch.equal(C.domination_counts(view), C.domination_counts(view.contiguous()))
    assert np.array_equal(C.pareto_ranks(view, 0).cpu().numpy(), rank)
    assert np.array_equal(C.domination_counts(view).cpu().numpy(), counts)


REPEATS = [("grid4", 513, 2), ("randn", 513, 2), ("dup", 257, 3)]


@gpu
@requires_gpu
@pytest.mark.parametrize("case", REPEATS, ids=_ids(REPEATS))
def test_repeated_calls_agree(C, case):
    """The front list is filled through an atomic counter, in any order;
    the ranks must not depend on it."""
    u = _utils(*case).to("cuda")
    first = C.pareto_ranks(u, 0)
    for _ in range(3):
        assert torch.equal(C.pareto_ranks(u, 0), first)
    assert torch.equal(C.domination_counts(u), C.domination_counts(u))


# ---------------------------------------------------------------------------
# 5. the early stop
# ---------------------------------------------------------------------------

EARLY = [("randn", 257, 2), ("randn", 300, 3), ("grid4", 257, 2), ("grid4", 300, 3), ("chain", 40, 2), ("chain", 257, 2)]


def _early_ks(n):
    return [None, 0, 1, n // 2, n - 1, n, n + 5]


def _check_early_stop(got, rank, k):
    """With F the first front index at which fronts 0..F hold k rows:
    (a) every row of fronts 0..F has its exact rank, (b) all rows whose rank
    is not exact share one value L, (c) L is above the rank returned for
    every row outside the lump {returned == L}, and no row of the lump
    belongs before L. The peel may go past F. The lump is numbered one past
    the last peeled front, so the rows of front L itself are in it with an
    exact rank: (c) is about the rows outside the lump."""
    n = rank.shape[0]
    need = n if (k is None or k <= 0 or k > n) else k
    sizes = np.bincount(rank)
    front = int(np.searchsorted(np.cumsum(sizes), need))
    assert front < sizes.shape[0]
    head = rank <= front
    assert np.array_equal(got[head], rank[head])  # (a)
    wrong = got != rank
    if wrong.any():
        lump = np.unique(got[wrong])
        assert lump.shape[0] == 1  # (b)
        in_lump = got == lump[0]
        assert (~in_lump).any() and lump[0] > got[~in_lump].max()  # (c)
        assert (rank[in_lump] >= lump[0]).all()
    if need == n:
        assert not wrong.any()


@pytest.mark.parametrize("case", EARLY, ids=_ids(EARLY))
def test_eager_early_stop(case):
    from evotorch_amd.core import _compute_pareto_ranks_eager

    u = _utils(*case).to(torch.float64)
    _, rank = _reference(*case)
    for k in _early_ks(case[1]):
        got, _ = _compute_pareto_ranks_eager(u, crowdsort=False, min_assigned=k)
        _check_early_stop(got.numpy(), rank, k)


@gpu
@requires_gpu
@pytest.mark.parametrize("case", EARLY, ids=_ids(EARLY))
def test_kernel_early_stop(case):
    from evotorch_amd import ops

    u = _utils(*case).to("cuda")
    _, rank = _reference(*case)
    for k in _early_ks(case[1]):
        got = ops.pareto_ranks(u, k)
        _check_early_stop(got.cpu().numpy(), rank, k)


# ---------------------------------------------------------------------------
# 6. take_best and argsort end to end
# ---------------------------------------------------------------------------

E2E = [(["min", "max"], 200, torch.float32), (["max", "min", "min"], 240, torch.float64)]


@functools.lru_cache(maxsize=None)
def _e2e_case(index):
    """Evals without ties (so that crowding does not depend on the order an
    unstable sort leaves equal values in), the reference ranks and float64
    CPU crowding distances, and the (rank, -crowding) order's pairs."""
    from evotorch_amd.core import _crowding_distances

    senses, n, dtype = E2E[index]
    g = torch.Generator().manual_seed(77 + index)
    evals = torch.randn(n, len(senses), generator=g, dtype=torch.float64).to(dtype)
    folded = evals.to(torch.float64).clone()
    for j, sense in enumerate(senses):
        if sense == "min":
            folded[:, j] = -folded[:, j]
    rank = ref_rank(folded.numpy())
    crowd = _crowding_distances(folded, torch.from_numpy(rank)).numpy()
    order = np.lexsort((-crowd, rank))
    pairs = np.stack([rank[order].astype(np.float64), crowd[order]], axis=1)
    return evals, rank, crowd, pairs


def _e2e_batch(index, device):
    from evotorch_amd import Problem

    senses, n, dtype = E2E[index]
    evals = _e2e_case(index)[0]
    problem = Problem(senses, lambda x: x, solution_length=1, initial_bounds=(-1, 1), eval_dtype=dtype, device=device)
    batch = problem.generate_batch(n)
    batch.access_values()[:, 0] = torch.arange(n, dtype=batch.dtype, device=device)  # a row's value is its index
    batch.set_evals(evals.to(device))
    return batch


def _check_take_best(index, device):
    _, rank, crowd, pairs = _e2e_case(index)
    n = rank.shape[0]
    sizes = np.bincount(rank)
    assert sizes.shape[0] > 3 and sizes[2] >= 2
    on_end = int(sizes[0] + sizes[1])  # k falls on the end of front 1
    in_front = on_end + int(sizes[2]) // 2  # k cuts front 2
    batch = _e2e_batch(index, device)
    for k in (1, on_end, in_front, n):
        chosen = batch.argsort(min_assigned=k)[:k].cpu().numpy()
        assert np.unique(chosen).shape[0] == k
        assert np.array_equal(np.stack([rank[chosen].astype(np.float64), crowd[chosen]], axis=1), pairs[:k])
        taken = batch.take_best(k).values[:, 0].cpu().numpy().astype(np.int64)
        assert np.unique(taken).shape[0] == k
        assert np.array_equal(np.stack([rank[taken].astype(np.float64), crowd[taken]], axis=1), pairs[:k])
    full = batch.argsort().cpu().numpy()
    assert np.array_equal(np.stack([rank[full].astype(np.float64), crowd[full]], axis=1), pairs)


@pytest.mark.parametrize("index", range(len(E2E)))
def test_take_best_cpu(index):
    _check_take_best(index, "cpu")


@gpu
@requires_gpu
@pytest.mark.parametrize("index", range(len(E2E)))
def test_take_best_gpu(index):
    _check_take_best(index, "cuda:0")


# ---------------------------------------------------------------------------
# 7. MAP-Elites cell assignment
# ---------------------------------------------------------------------------

NEG_INF = float("-inf")


def _random_boxes(cells, n, f, seed):
    """Integer boxes and integer features: many rows exactly on a box edge,
    overlapping boxes, utilities from {0, 1, 2} (ties), a few -inf
    utilities and a few rows with a NaN feature."""
    g = torch.Generator().manual_seed(seed)
    if f >= 16:  # wide boxes, or no row is inside all 16 intervals
        lo = torch.randint(0, 2, (cells, f), generator=g)
        hi = torch.randint(3, 5, (cells, f), generator=g)
    else:
        lo = torch.randint(0, 4, (cells, f), generator=g)
        hi = lo + torch.randint(0, 3, (cells, f), generator=g)
    grid = torch.stack([lo, hi], dim=-1).to(torch.float32)
    feats = torch.randint(0, 5, (n, f), generator=g).to(torch.float32)
    utils = torch.randint(0, 3, (n,), generator=g).to(torch.float32)
    utils[3::5] = NEG_INF
    if n > 1:
        for r in (n // 7, n - 1):
            feats[r, r % f] = float("nan")
    return grid, feats, utils


def _lattice(n, f, bins, seed, dtype=torch.float32):
    """A make_feature_grid grid over [0, bins]^f with integer edges, and
    features on the half-integer lattice from -2 to bins + 2: on interior
    edges (inside both neighbours), between them, and outside the nominal
    bounds (inside the outer cells, whose far edges are -inf and +inf)."""
    from evotorch_amd.algorithms import make_feature_grid

    g = torch.Generator().manual_seed(seed)
    grid = make_feature_grid([0.0] * f, [float(bins)] * f, bins, dtype=dtype)
    feats = (torch.randint(0, 2 * bins + 9, (n, f), generator=g).to(dtype) - 4.0) / 2.0
    utils = torch.randint(0, 3, (n,), generator=g).to(torch.float32)
    return grid, feats, utils


ME_SIZES = [(c, n, f) for c in (1, 255, 256, 257) for n in (1, 300) for f in (1, 3, 16)]
ME_CASES = [("boxes", c, n, f) for (c, n, f) in ME_SIZES] + [
    ("lattice", 16, 300, 2),
    ("lattice-sparse", 64, 5, 3),  # most cells stay empty
    ("all-neg-inf", 2, 3, 1),
    ("nan-rows", 3, 4, 1),
    ("straddle64", 4, 6, 1),
    ("lattice64", 16, 300, 2),
]


@functools.lru_cache(maxsize=None)
def _me_case(case):
    """(grid, feats, utils) on the CPU; utils are fp32 and hold no NaN."""
    kind, cells, n, f = case
    if kind == "boxes":
        return _random_boxes(cells, n, f, seed=1000 * cells + 10 * n + f)
    if kind == "lattice":
        return _lattice(n, f, 4, seed=1)
    if kind == "lattice-sparse":
        return _lattice(n, f, 4, seed=2)
    if kind == "lattice64":
        return _lattice(n, f, 4, seed=3, dtype=torch.float64)
    if kind == "all-neg-inf":
        # row 0 is the best of the batch and outside cell 1, whose inside
        # rows 1 and 2 both have utility -inf
        grid = torch.tensor([[[0.0, 1.0]], [[2.0, 3.0]]])
        feats = torch.tensor([[0.5], [2.5], [2.75]])
        utils = torch.tensor([1.0, NEG_INF, NEG_INF])
        return grid, feats, utils
    if kind == "nan-rows":
        grid = torch.tensor([[[NEG_INF, 1.0]], [[1.0, 2.0]], [[2.0, float("inf")]]])
        feats = torch.tensor([[float("nan")], [1.5], [float("nan")], [0.5]])
        utils = torch.tensor([2.0, 0.0, 2.0, 1.0])
        return grid, feats, utils
    if kind == "straddle64":
        from evotorch_amd.algorithms import make_feature_grid

        grid = make_feature_grid([0.0], [4.0], 4, dtype=torch.float64)
        e = 2.0**-40
        feats = torch.tensor([[1.0 + e], [2.0 - e], [2.0], [3.0 + e], [3.0 - e], [1.0]], dtype=torch.float64)
        utils = torch.tensor([0.0, 1.0, 2.0, 2.0, 1.0, 0.0])
        return grid, feats, utils
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _me_reference(case):
    grid, feats, utils = _me_case(case)
    return ref_assign(grid.double().numpy(), feats.double().numpy(), utils.double().numpy())


def test_ref_assign_known_answers():
    best, valid = _me_reference(("all-neg-inf", 2, 3, 1))
    assert best.tolist() == [0, 1] and valid.tolist() == [True, True]
    best, valid = _me_reference(("nan-rows", 3, 4, 1))
    assert best.tolist() == [3, 1, 0] and valid.tolist() == [True, True, False]
    # 1 + 2**-40 is in cell 1 only; 2.0 is on the edge of cells 1 and 2 and
    # wins both on utility; 3 + 2**-40 is in cell 3, 3 - 2**-40 in cell 2
    best, valid = _me_reference(("straddle64", 4, 6, 1))
    assert best.tolist() == [5, 2, 2, 3] and valid.all()
    grid, feats, utils = _me_case(("straddle64", 4, 6, 1))
    best32, _ = ref_assign(grid.float().numpy(), feats.float().numpy(), utils.numpy())
    assert best32.tolist() != best.tolist()
    # one feature row on an interior edge of one of two features: two cells
    from evotorch_amd.algorithms import make_feature_grid

    grid = make_feature_grid([0.0, 0.0], [4.0, 4.0], 4)
    _, valid = ref_assign(grid.numpy(), np.array([[1.0, 0.5]]), np.array([0.0]))
    assert np.flatnonzero(valid).tolist() == [0, 4]
    _, valid = ref_assign(grid.numpy(), np.array([[-7.0, 9.0]]), np.array([0.0]))
    assert np.flatnonzero(valid).tolist() == [3]
    _, valid = _me_reference(("lattice-sparse", 64, 5, 3))
    assert valid.any() and not valid.all()


def _assign_through_searcher(case, device, sense):
    """The case through MAPElites._assign_cells: a batch whose evals hold
    the fitness and the features; a -inf utility is a NaN fitness there."""
    from evotorch_amd import Problem
    from evotorch_amd.algorithms import MAPElites

    grid, feats, utils = _me_case(case)
    n, f = feats.shape
    dtype = grid.dtype
    fitness = (utils if sense == "max" else -utils).to(dtype)
    fitness = torch.where(torch.isinf(fitness), torch.full_like(fitness, float("nan")), fitness)
    problem = Problem(sense, lambda x: x, solution_length=1, initial_bounds=(-1, 1), eval_data_length=f,
                      eval_dtype=dtype, device=device)
    searcher = MAPElites(problem, operators=[], feature_grid=grid.to(device))
    batch = problem.generate_batch(n)
    batch.access_evals().copy_(torch.cat([fitness.unsqueeze(1), feats], dim=1))
    return searcher._assign_cells(batch)


@pytest.mark.parametrize("sense", ["max", "min"])
@pytest.mark.parametrize("case", ME_CASES, ids=_ids(ME_CASES))
def test_eager_assign_matches_reference(case, sense):
    best, valid = _me_reference(case)
    got_best, got_valid = _assign_through_searcher(case, "cpu", sense)
    assert np.array_equal(got_valid.numpy(), valid)
    assert np.array_equal(got_best.numpy(), best)


@gpu
@requires_gpu
@pytest.mark.parametrize("case", ME_CASES, ids=_ids(ME_CASES))
def test_assign_kernel_matches_reference(C, case):
    grid, feats, utils = (t.to("cuda") for t in _me_case(case))
    best, valid = _me_reference(case)
    got_best, got_valid = C.mapelites_assign(grid, feats, utils)
    assert got_best.dtype == torch.int64 and got_valid.dtype == torch.bool
    assert np.array_equal(got_valid.cpu().numpy(), valid)
    assert np.array_equal(got_best.cpu().numpy(), best)


ME_STRIDED = [("boxes", 257, 300, 3), ("boxes", 256, 300, 16), ("lattice64", 16, 300, 2)]


@gpu
@requires_gpu
@pytest.mark.parametrize("case", ME_STRIDED, ids=_ids(ME_STRIDED))
def test_assign_kernel_strided_operands(C, case):
    """feats and utils as two views of one (N, 1 + F) tensor."""
    grid, feats, utils = _me_case(case)
    evals = torch.cat([utils.to(grid.dtype).unsqueeze(1), feats], dim=1).to("cuda")
    feats_v, utils_v = evals[:, 1:], evals[:, 0]
    assert not feats_v.is_contiguous() and not utils_v.is_contiguous()
    best, valid = _me_reference(case)
    got_best, got_valid = C.mapelites_assign(grid.to("cuda"), feats_v, utils_v)
    assert np.array_equal(got_valid.cpu().numpy(), valid)
    assert np.array_equal(got_best.cpu().numpy(), best)


@gpu
@requires_gpu
@pytest.mark.parametrize("sense", ["max", "min"])
@pytest.mark.parametrize("case", ME_CASES, ids=_ids(ME_CASES))
def test_assign_cells_on_gpu_matches_reference(case, sense):
    best, valid = _me_reference(case)
    got_best, got_valid = _assign_through_searcher(case, "cuda:0", sense)
    assert np.array_equal(got_valid.cpu().numpy(), valid)
    assert np.array_equal(got_best.cpu().numpy(), best)


@gpu
@requires_gpu
def test_assign_kernel_rejects_17_features(C):
    grid = torch.zeros(4, 17, 2, device="cuda")
    feats = torch.zeros(5, 17, device="cuda")
    utils = torch.zeros(5, device="cuda")
    with pytest.raises(RuntimeError, match="at most 16 feature dimensions"):
        C.mapelites_assign(grid, feats, utils)


# ---------------------------------------------------------------------------
# 8. empty inputs return before any launch
# ---------------------------------------------------------------------------


def _ordinary_launch(C):
    """One ordinary launch and a synchronise: an error that an earlier call
    left in the runtime would surface here."""
    u = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0]], device="cuda")
    counts = C.domination_counts(u)
    torch.cuda.synchronize()
    assert counts.tolist() == [3, 0, 1, 1]


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_empty_population(C, dtype):
    u = torch.empty(0, 3, dtype=dtype, device="cuda")
    ranks = C.pareto_ranks(u, 0)
    assert ranks.shape == (0,) and ranks.dtype == torch.int64 and ranks.is_cuda
    _ordinary_launch(C)
    counts = C.domination_counts(u)
    assert counts.shape == (0,) and counts.dtype == torch.int32 and counts.is_cuda
    _ordinary_launch(C)
    from evotorch_amd import ops

    assert ops.pareto_ranks(u, 5).shape == (0,)
    assert ops.domination_counts(u).shape == (0,)
    _ordinary_launch(C)


@gpu
@requires_gpu
def test_empty_grid_and_empty_batch(C):
    feats = torch.zeros(5, 3, device="cuda")
    utils = torch.zeros(5, device="cuda")
    best, valid = C.mapelites_assign(torch.empty(0, 3, 2, device="cuda"), feats, utils)
    assert best.shape == (0,) and best.dtype == torch.int64
    assert valid.shape == (0,) and valid.dtype == torch.bool
    _ordinary_launch(C)
    grid = torch.zeros(7, 3, 2, device="cuda")
    best, valid = C.mapelites_assign(grid, torch.empty(0, 3, device="cuda"), torch.empty(0, device="cuda"))
    assert not valid.any() and valid.shape == (7,)
    assert not best.any() and best.shape == (7,)
    _ordinary_launch(C)
