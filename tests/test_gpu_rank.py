"""GPU tests of the fused score + rank-count kernels (K9, topk_kernels.hip)
against the float64 oracle ``reference.rank_counts_f64``.

Exact cases use integer factors in [-3, 3], as test_gpu_topk.py does: exact
in bf16, every dot exact in fp32 in any summation order, ties plentiful --
so both counts must equal the oracle's and the score must be bit-equal.
"""

import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.models.ranking import evaluate_ranking
from flink_ms_amd.ops import reference

import _topk_store_fixture as fx

pytestmark = pytest.mark.gpu


def _ints(shape, seed, lo=-3, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.bfloat16)


def _pairs(P, nq, nv, seed):
    """Shuffled, repeating queries; the last pair repeats the first."""
    g = torch.Generator().manual_seed(seed)
    q_idx = torch.randint(0, nq, (P,), generator=g)
    t_idx = torch.randint(0, nv, (P,), generator=g)
    q_idx[-1], t_idx[-1] = q_idx[0], t_idx[0]
    return q_idx, t_idx


def _to(gpu, t):
    if t is None:
        return None
    if isinstance(t, tuple):
        return tuple(x.to(gpu) for x in t)
    return t.to(gpu)


def _run(gpu, Q, V, q_idx, t_idx, cand=None, exclude=None, chunk_items=None):
    g, e, s = ops.rank_counts(Q.to(gpu), V.to(gpu), q_idx.to(gpu),
                              t_idx.to(gpu), cand=_to(gpu, cand),
                              exclude=_to(gpu, exclude),
                              chunk_items=chunk_items)
    torch.cuda.synchronize()
    P = q_idx.numel()
    assert g.shape == (P,) and g.dtype == torch.int64
    assert e.shape == (P,) and e.dtype == torch.int64
    assert s.shape == (P,) and s.dtype == torch.float32
    return g.cpu(), e.cpu(), s.cpu()


def _same_scores(a, b):
    """Bitwise-equal values (NaN == NaN, -0 != +0 is not asked)."""
    return torch.equal(torch.nan_to_num(a.double(), nan=12345.0),
                       torch.nan_to_num(b.double(), nan=12345.0))


def _check_exact(gpu, Q, V, q_idx, t_idx, cand=None, exclude=None,
                 chunk_items=None):
    got = _run(gpu, Q, V, q_idx, t_idx, cand, exclude, chunk_items)
    want = reference.rank_counts_f64(Q, V, q_idx, t_idx, cand, exclude)
    assert torch.equal(got[0], want[0]), (got[0], want[0])
    assert torch.equal(got[1], want[1]), (got[1], want[1])
    assert _same_scores(got[2], want[2])
    return got


def _csr(lists):
    ptr = torch.zeros(len(lists) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.tensor([len(x) for x in lists]), 0)
    flat = [r for rows in lists for r in sorted(rows)]
    return ptr, torch.tensor(flat, dtype=torch.int64)


# --------------------------------------------------------------- exact cross
# (P, nq, nc, k): k = 1 / 10 / 100 take the scalar load path, 40 the vector
# path with a zero-filled half step; (16, 1, ...) is one user filling a tile
CROSS = [
    (1, 1, 1, 1), (15, 3, 15, 10), (16, 16, 16, 16), (17, 5, 17, 32),
    (33, 7, 1000, 40), (16, 1, 1000, 100), (33, 33, 1000, 128),
    (17, 17, 1000, 64),
]


@pytest.mark.parametrize("P,nq,nc,k", CROSS)
def test_exact_cross(gpu, P, nq, nc, k):
    Q = _ints((nq, k), 100 + nq + k)
    V = _ints((nc, k), 200 + nc + k)
    q_idx, t_idx = _pairs(P, nq, nc, 300 + P)
    g, e, s = _check_exact(gpu, Q, V, q_idx, t_idx)
    assert (int(g[-1]), int(e[-1])) == (int(g[0]), int(e[0]))
    assert bool(((g + e) <= nc - 1).all())


def test_no_pairs(gpu):
    Q, V = _ints((3, 16), 1), _ints((20, 16), 2)
    none = torch.zeros(0, dtype=torch.int64)
    g, e, s = _run(gpu, Q, V, none, none)
    assert g.numel() == e.numel() == s.numel() == 0


# ------------------------------------------------------------------ chunking

@pytest.mark.parametrize("chunk", [16, 48, 64])
def test_explicit_chunks_do_not_change_the_result(gpu, chunk):
    nc = 3 * chunk + 5
    Q, V = _ints((7, 40), 1), _ints((nc, 40), 2)
    q_idx, t_idx = _pairs(33, 7, nc, 3)
    ptr, ex = _csr([list(range(q, nc, 5 + q)) for q in range(7)])
    for exclude in (None, (ptr, ex)):
        single = _check_exact(gpu, Q, V, q_idx, t_idx, exclude=exclude,
                              chunk_items=nc)
        split = _check_exact(gpu, Q, V, q_idx, t_idx, exclude=exclude,
                             chunk_items=chunk)
        for a, b in zip(single, split):
            assert torch.equal(a, b)


def test_default_chunk_edges(gpu):
    P, nq = 17, 5
    base = ops.rank_chunk_items(P, 1000)
    for nc in (base - 1, base, base + 1):
        # the default split of these sizes: one chunk up to base, then two
        assert ops.rank_chunk_items(P, nc) == base
        Q, V = _ints((nq, 32), 3), _ints((nc, 32), 4 + nc)
        q_idx, t_idx = _pairs(P, nq, nc, 5)
        a = _check_exact(gpu, Q, V, q_idx, t_idx)
        b = _check_exact(gpu, Q, V, q_idx, t_idx, chunk_items=nc)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ----------------------------------------------------------------- exclusion

def test_exclusion(gpu):
    nq, nv, k = 9, 300, 32
    Q, V = _ints((nq, k), 21), _ints((nv, k), 22)
    g = torch.Generator().manual_seed(23)
    # three pairs per query, so every slice is shared by several pairs
    q_idx = torch.arange(nq).repeat(3)
    t_idx = torch.randint(0, nv, (3 * nq,), generator=g)
    perm = [torch.randperm(nv, generator=g).tolist() for _ in range(nq)]
    lists = [
        [],                                   # empty
        t_idx[1::nq].tolist(),                # exactly query 1's targets
        list(range(nv)),                      # every candidate
        perm[3][:15], perm[4][:16], perm[5][:17], perm[6][:200],
        perm[7][:31] + [int(t_idx[7])],       # a tile edge plus a target
        perm[8][:1],
    ]
    lists = [sorted(set(x)) for x in lists]
    for chunk in (None, 48):
        g_, e_, _ = _check_exact(gpu, Q, V, q_idx, t_idx,
                                 exclude=_csr(lists), chunk_items=chunk)
        assert g_[2::nq].tolist() == [0, 0, 0]
        assert e_[2::nq].tolist() == [0, 0, 0]
    # with cand: excluded rows that are no candidates, targets that are none
    cand = torch.arange(0, nv, 2)
    assert bool((t_idx % 2 == 1).any()) and bool((t_idx % 2 == 0).any())
    for chunk in (None, 48):
        g_, e_, _ = _check_exact(gpu, Q, V, q_idx, t_idx, cand=cand,
                                 exclude=_csr(lists), chunk_items=chunk)
        assert g_[2::nq].tolist() == [0, 0, 0]
    # a permuted candidate list counts the same rows
    shuffled = cand[torch.randperm(cand.numel(), generator=g)]
    a = _check_exact(gpu, Q, V, q_idx, t_idx, cand=shuffled,
                     exclude=_csr(lists))
    assert torch.equal(a[0], g_) and torch.equal(a[1], e_)


# ------------------------------------------------------------ NaN, inf, -0

def test_nan_inf_order(gpu):
    Q = _ints((3, 16), 31, lo=1, hi=3)
    V = _ints((40, 16), 32)
    V[5] = float("nan")
    V[9, 3] = float("nan")
    V[7] = float("inf")
    V[8] = float("-inf")
    q_idx = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1])
    t_idx = torch.tensor([5, 9, 7, 8, 0, 5, 7, 20])   # NaN, inf, -inf targets
    g, e, s = _check_exact(gpu, Q, V, q_idx, t_idx)
    # a NaN target loses to the 38 numbers and ties with the other NaN row
    assert (int(g[0]), int(e[0])) == (38, 1) and bool(s[0].isnan())
    assert (int(g[2]), int(e[2])) == (0, 0) and float(s[2]) == float("inf")
    assert (int(g[3]), int(e[3])) == (37, 0) and float(s[3]) == -float("inf")
    ptr, ex = _csr([[9], [5, 7], []])
    _check_exact(gpu, Q, V, q_idx, t_idx, exclude=(ptr, ex))


def test_negative_zero_target_ties_with_zero(gpu):
    """A -0.0 target score is a tie with +0.0 candidates: the order word
    folds the two zeros."""
    V = _ints((40, 16), 33, lo=1, hi=3)
    V[4] = -V[4]
    Q = torch.zeros(2, 16, dtype=torch.bfloat16)
    Q[1] = -Q[1]                                       # a row of -0.0
    q_idx, t_idx = torch.tensor([0, 1, 0, 1]), torch.tensor([4, 4, 9, 9])
    g, e, s = _check_exact(gpu, Q, V, q_idx, t_idx)
    assert g.tolist() == [0] * 4 and e.tolist() == [39] * 4
    assert s.tolist() == [0.0] * 4


# ---------------------------------------------------------------- real data

def _real(k):
    g = torch.Generator().manual_seed(7 + k)
    Q = torch.randn(40, k, generator=g).to(torch.bfloat16)
    V = torch.randn(1000, k, generator=g).to(torch.bfloat16)
    q_idx = torch.randint(0, 40, (200,), generator=g)
    t_idx = torch.randint(0, 1000, (200,), generator=g)
    return Q, V, q_idx, t_idx


@pytest.mark.parametrize("k", [64, 100])
def test_same_bits_as_topk(gpu, k):
    """The score of a (query, row) is the same 32 bits in K8 and K9, so a
    target that K8 lists sits exactly where the counts say."""
    Q, V, q_idx, t_idx = _real(k)
    g0 = torch.Generator().manual_seed(k)
    exclude = _csr([torch.randperm(1000, generator=g0)[:50 + q].tolist()
                    for q in range(40)])
    topk = 128
    g, e, s = _run(gpu, Q, V, q_idx, t_idx, exclude=exclude)
    ls, lr = ops.topk_scores(Q.to(gpu), V.to(gpu), topk,
                             exclude=_to(gpu, exclude))
    ls, lr = ls.cpu(), lr.cpu()
    ls_bits, s_bits = ls.view(torch.int32), s.view(torch.int32)
    listed = 0
    for p in range(200):
        q, t = int(q_idx[p]), int(t_idx[p])
        at = (lr[q] == t).nonzero(as_tuple=True)[0]
        if int(g[p]) >= topk:
            assert at.numel() == 0
        if at.numel() == 0:
            continue
        listed += 1
        pos = int(at[0])
        assert int(ls_bits[q, pos]) == int(s_bits[p])
        assert int(g[p]) <= pos <= int(g[p]) + int(e[p])
        if int(e[p]) == 0:
            assert pos == int(g[p])
    assert listed >= 5                                 # not vacuous


@pytest.mark.parametrize("k", [64, 100])
def test_real_valued_bracket(gpu, k):
    """Normal factors against float64: with b(q, r) = 2 k 2^-24
    sum_c |Q[q][c] V[r][c]| bounding |fp32 - fp64| of one score (the bound
    of test_gpu_topk.test_real_valued), a row certainly above the target in
    float64 (by more than both bounds) must be counted greater, and a row
    certainly below must not be counted at all."""
    Q, V, q_idx, t_idx = _real(k)
    g, e, s = _run(gpu, Q, V, q_idx, t_idx)
    S64 = Q.double() @ V.double().T
    B = 2 * k * 2.0 ** -24 * (Q.double().abs() @ V.double().abs().T)
    tight = 0
    for p in range(200):
        q, t = int(q_idx[p]), int(t_idx[p])
        others = torch.ones(1000, dtype=torch.bool)
        others[t] = False
        lo = int(((S64[q] > S64[q, t] + B[q] + B[q, t]) & others).sum())
        hi = int(((S64[q] >= S64[q, t] - B[q] - B[q, t]) & others).sum())
        assert lo <= int(g[p]) <= hi, (p, lo, int(g[p]), hi)
        assert lo <= int(g[p]) + int(e[p]) <= hi, (p, lo, int(e[p]), hi)
        assert abs(float(s[p]) - float(S64[q, t])) <= float(B[q, t])
        tight += lo == hi
    # a property of the inputs, not of the kernel: 188 (k = 64) and 179
    # (k = 100) of the 200 brackets are a single value
    assert tight >= 170, tight


# ---------------------------------------------------------- model and store

def test_evaluate_ranking_gpu_equals_cpu(gpu):
    nu, ni, k = 50, 300, 24
    U, V = _ints((nu, k), 51), _ints((ni, k), 52)
    g = torch.Generator().manual_seed(53)
    tu = torch.randint(0, nu, (2000,), generator=g)
    ti = torch.randint(0, ni, (2000,), generator=g)
    hu = torch.randint(0, nu + 2, (400,), generator=g)     # two unknown users
    hi = torch.randint(0, ni, (400,), generator=g)
    want = evaluate_ranking(U, V, tu, ti, hu, hi, ns=(1, 10, 100))
    got = evaluate_ranking(U.to(gpu), V.to(gpu), tu, ti, hu, hi,
                           ns=(1, 10, 100))
    assert (got.n_scored, got.n_skipped, got.n_degenerate) == \
        (want.n_scored, want.n_skipped, want.n_degenerate)
    assert want.n_skipped > 0 and want.n_scored > 300
    flat = lambda r: ([r.mean_percentile_rank, r.auc, r.mrr]   # noqa: E731
                      + [r.hit_rate[n] for n in (1, 10, 100)]
                      + [r.ndcg[n] for n in (1, 10, 100)])
    for a, b in zip(flat(got), flat(want)):
        assert abs(a - b) <= 1e-12, (flat(got), flat(want))


def test_store_rank_gpu_equals_cpu(gpu):
    cpu_store = fx.build_store(torch.device("cpu"))
    gpu_store = fx.build_store(gpu)
    users = ["1", "2", "3", "4", "5", "999", "1", "2"]
    items = ["12", "31", "20", "11", "30", "10", "888", "26"]
    exclude = [["20", "13"], [], ["777"], ["30", "31", "12"], ["30"], [],
               [], ["26", "10"]]
    for ex in (None, exclude):
        want = cpu_store.rank(users, items, ex)
        got = gpu_store.rank(users, items, ex)
        assert got == want
    assert want[0] == [True] * 5 + [False, False, True]
