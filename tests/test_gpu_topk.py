"""GPU tests of the fused score + top-k kernels (topk_kernels.hip) against
the float64 oracle ``reference.topk_scores_f64``.

Exact cases use integer factors in [-3, 3]: exact in bf16, and every dot is
exact in fp32 in any summation order (|sum| <= 9 * 128 = 1152), so rows AND
scores must equal the oracle bit for bit, ties included (they are plentiful:
at most 2305 distinct scores).
"""

import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.ops import reference

import _topk_store_fixture as fx

pytestmark = pytest.mark.gpu

INF = float("inf")


def _ints(shape, seed, lo=-3, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.bfloat16)


def _run(gpu, Q, V, topk, cand=None, exclude=None, chunk_items=None):
    s, r = ops.topk_scores(
        Q.to(gpu), V.to(gpu), topk,
        cand=None if cand is None else cand.to(gpu),
        exclude=None if exclude is None else tuple(t.to(gpu)
                                                   for t in exclude),
        chunk_items=chunk_items)
    torch.cuda.synchronize()
    assert s.shape == (Q.shape[0], topk) and s.dtype == torch.float32
    assert r.shape == (Q.shape[0], topk) and r.dtype == torch.int64
    return s.cpu(), r.cpu()


def _same(a, b):
    """Bitwise-equal results (NaN == NaN)."""
    return (torch.equal(a[1], b[1])
            and torch.equal(torch.nan_to_num(a[0].double(), nan=12345.0),
                            torch.nan_to_num(b[0].double(), nan=12345.0)))


def _check_exact(gpu, Q, V, topk, cand=None, exclude=None, chunk_items=None):
    got = _run(gpu, Q, V, topk, cand, exclude, chunk_items)
    want = reference.topk_scores_f64(Q, V, topk, cand, exclude)
    assert torch.equal(got[1], want[1]), (got[1], want[1])
    assert _same(got, want)
    return got


def _csr(lists):
    ptr = torch.zeros(len(lists) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.tensor([len(x) for x in lists]), 0)
    flat = [r for rows in lists for r in sorted(rows)]
    return ptr, torch.tensor(flat, dtype=torch.int64)


# --------------------------------------------------------------- exact cross
# (nq, nc, k, topk): every value of the issue's four lists appears, topk > nc
# included; k = 1 / 10 / 100 take the scalar load path, 40 the vector path
# with a zero-filled half step.
CROSS = [
    (1, 1, 1, 1), (15, 15, 10, 10), (16, 16, 16, 64), (17, 17, 32, 128),
    (33, 1000, 40, 10), (1, 1000, 64, 64), (16, 1000, 100, 128),
    (17, 15, 128, 1), (33, 17, 64, 128), (15, 1000, 128, 10),
    (16, 1, 10, 10), (1, 16, 16, 1), (33, 1000, 1, 64), (17, 1000, 100, 1),
    (15, 1000, 32, 128), (33, 16, 40, 10),
]


@pytest.mark.parametrize("nq,nc,k,topk", CROSS)
def test_exact_cross(gpu, nq, nc, k, topk):
    Q = _ints((nq, k), 100 + nq + k)
    V = _ints((nc, k), 200 + nc + k)
    _check_exact(gpu, Q, V, topk)


# ------------------------------------------------------------------ chunking

@pytest.mark.parametrize("chunk", [16, 48, 64])
@pytest.mark.parametrize("topk", [10, 100])
def test_explicit_chunks_do_not_change_the_result(gpu, chunk, topk):
    nc = 3 * chunk + 5
    Q, V = _ints((17, 40), 1), _ints((nc, 40), 2)
    single = _check_exact(gpu, Q, V, topk, chunk_items=nc)
    assert _same(_check_exact(gpu, Q, V, topk, chunk_items=chunk), single)


@pytest.mark.parametrize("topk", [10, 128])
def test_default_chunk_edges(gpu, topk):
    nq = 17
    base = ops.topk_chunk_items(nq, 1000, topk)
    for nc in (base - 1, base, base + 1):
        # the default split of these sizes: one chunk up to base, then two
        assert ops.topk_chunk_items(nq, nc, topk) == base
        Q, V = _ints((nq, 32), 3), _ints((nc, 32), 4 + nc)
        assert _same(_check_exact(gpu, Q, V, topk),
                     _check_exact(gpu, Q, V, topk, chunk_items=nc))


# -------------------------------------------------------- threshold pressure

@pytest.mark.parametrize("topk", [10, 128])
@pytest.mark.parametrize("order", ["ascending", "descending", "equal"])
def test_threshold_pressure(gpu, order, topk):
    nc, k = 1000, 64
    q = _ints((1, k), 7)
    V = _ints((nc, k), 8)
    if order == "equal":
        V = V[:1].repeat(nc, 1)                   # a pure row-order result
    else:
        s = (V.double() @ q.double().T).squeeze(1)
        V = V[torch.sort(s, stable=True,
                         descending=order == "descending").indices]
    Q = q.repeat(18, 1)                            # two query tiles
    for chunk in (nc, 160):
        s, r = _check_exact(gpu, Q, V, topk, chunk_items=chunk)
    if order == "equal":
        assert r[17].tolist() == list(range(topk))


# ---------------------------------------------------------------------- cand

def test_cand_lists(gpu):
    nv, k = 700, 40
    Q, V = _ints((17, k), 11), _ints((nv, k), 12)
    g = torch.Generator().manual_seed(13)
    for cand in (torch.randperm(nv, generator=g)[:333],          # permuted
                 torch.arange(0, nv, 3),                          # strided
                 torch.arange(nv - 1, nv - 21, -1),               # the tail
                 torch.tensor([nv - 1])):
        for topk in (10, 64):
            s, r = _check_exact(gpu, Q, V, topk, cand=cand,
                                chunk_items=None if topk == 10 else 48)
            live = r[r >= 0]
            assert set(live.tolist()) <= set(cand.tolist())       # rows of V
            assert (r >= 0).sum(1).tolist() == [min(topk, cand.numel())] * 17


# ----------------------------------------------------------------- exclusion

def test_exclusion(gpu):
    nq, nv, k, topk = 17, 300, 32, 10
    Q, V = _ints((nq, k), 21), _ints((nv, k), 22)
    cand = torch.arange(0, nv, 2)
    _, top = reference.topk_scores_f64(Q, V, topk, cand)
    g = torch.Generator().manual_seed(23)
    cases = {
        "empty": [[] for _ in range(nq)],
        "current-top": [row.tolist() for row in top],
        "non-candidates": [list(range(1, nv, 2)) for _ in range(nq)],
        "padding": [cand[:-(q % 4 + 1)].tolist() for q in range(nq)],
        "ragged": [torch.randperm(nv, generator=g)[:(37 * q) % 290].tolist()
                   for q in range(nq)],
    }
    for name, lists in cases.items():
        for chunk in (None, 48):
            s, r = _check_exact(gpu, Q, V, topk, cand=cand,
                                exclude=_csr(lists), chunk_items=chunk)
            for q in range(nq):
                assert not set(r[q].tolist()) & set(lists[q]), name
        if name == "padding":
            assert (r >= 0).sum(1).tolist() == [q % 4 + 1 for q in range(nq)]
            assert s[0, 1:].tolist() == [-INF] * (topk - 1)
        if name == "non-candidates":
            assert torch.equal(r, top)


def test_nan_scores_rank_last(gpu):
    Q = _ints((3, 16), 31, lo=1, hi=3)
    V = _ints((40, 16), 32)
    V[5] = float("nan")
    V[9, 3] = float("nan")
    V[7] = float("inf")
    s, r = _check_exact(gpu, Q, V, 40)
    assert r[:, 0].tolist() == [7, 7, 7] and s[:, 0].tolist() == [INF] * 3
    assert r[:, -2:].tolist() == [[5, 9]] * 3 and bool(s[:, -2:].isnan().all())


# ----------------------------------------------------------------- real data

@pytest.mark.parametrize("k", [64, 100])
def test_real_valued(gpu, k):
    """Normal factors: scores within the fp32 accumulation bound of the
    float64 score of the returned row, and no better candidate left out.

    b(q, r) = 2 k 2^-24 sum_c |Q[q][c] V[r][c]| bounds |fp32 - fp64| of one
    score (the bf16 products are exact in fp32; k - 1 rounded additions).
    An unreturned u has fp32 score <= the fp32 score of every returned row,
    so s64(u) <= fp32(u) + b(u) <= fp32(r*) + b(u) <= s64(r*) + b(r*) + b(u)
    for the returned row r* of smallest s64: at most 2 max_r b(q, r) above
    it, the maximum taken over all candidates of the query."""
    nq, nv, topk = 20, 3000, 100
    g = torch.Generator().manual_seed(40 + k)
    Q = torch.randn(nq, k, generator=g).to(torch.bfloat16)
    V = torch.randn(nv, k, generator=g).to(torch.bfloat16)
    cand = torch.randperm(nv, generator=g)[:2500]
    lists = [torch.randperm(nv, generator=g)[:50 + q].tolist()
             for q in range(nq)]
    s, r = _run(gpu, Q, V, topk, cand=cand, exclude=_csr(lists))
    S64 = Q.double() @ V.double().T
    B = 2 * k * 2.0 ** -24 * (Q.double().abs() @ V.double().abs().T)
    is_cand = torch.zeros(nv, dtype=torch.bool)
    is_cand[cand] = True
    for q in range(nq):
        rows = r[q]
        assert int(rows.min()) >= 0                   # enough candidates
        assert len(set(rows.tolist())) == topk        # distinct
        assert not set(rows.tolist()) & set(lists[q])
        assert bool(is_cand[rows].all())
        assert bool((s[q, 1:] <= s[q, :-1]).all())    # non-increasing
        err = (s[q].double() - S64[q, rows]).abs()
        assert bool((err <= B[q, rows]).all()), (err / B[q, rows]).max()
        left = is_cand.clone()
        left[rows] = False
        left[torch.tensor(lists[q])] = False
        limit = S64[q, rows].min() + 2 * B[q, is_cand].max()
        assert float(S64[q, left].max()) <= float(limit)


# --------------------------------------------------------------------- store

def test_store_recommend_gpu_equals_cpu(gpu):
    cpu_store = fx.build_store(torch.device("cpu"))
    gpu_store = fx.build_store(gpu)
    users = list(fx.USERS) + ["999"]
    exclude = [["20", "13"], [], ["777"], ["30", "31", "12"], [], []]
    for n in (1, 7, 128):
        for ex in (None, exclude):
            want = cpu_store.recommend(users, n, ex)
            got = gpu_store.recommend(users, n, ex)
            assert got == want
            for u, items in zip(users[:-1], got[1]):
                gone = set(ex[users.index(u)]) if ex else set()
                assert items == fx.brute_force(cpu_store, u, n, gone)[0]
