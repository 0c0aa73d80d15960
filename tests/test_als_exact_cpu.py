"""The exact-integer fixtures of tests/_exact_fixture.py, checked on the CPU:
these tests are about the fixtures, not the kernels.

- the fp32 torch references reproduce the float64 oracle and the closed form
  ``L D L^T`` bit for bit, for every family, rank and gather dtype;
- a plain fp32 LDL^T of the kernels' shape (raw columns ``L*D``, one
  reciprocal per pivot, multiply instead of divide), right-looking and
  left-looking, returns ``x_true`` bit for bit, graded pivots included;
- the fixtures are sensitive: losing one stored entry, or moving one entry
  of L across a tile boundary, changes the answer, and a solver with a pivot
  scaled by 1 + 1e-4 or one tile update left out no longer returns x_true;
- tables and ratings survive the gather dtypes and the rating pair unchanged.
"""

import numpy as np
import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.data.blocked import CSR
from flink_ms_amd.ops import reference as R

import _exact_fixture as fx

RANKS = [16, 32, 48, 64, 80, 96, 112, 128]
GATHERS = ["bf16", "fp8"]
ROW_LENGTHS = fx.ROW_LENGTHS


def ldl_right_looking(A, b, pivot_slip=0.0, skip_tile=None):
    """fp32 LDL^T solve, right-looking: after pivot j the whole trailing
    block is updated.  Columns stay raw (L*D); 1/d once per pivot.

    The two extra arguments make it deliberately WRONG, the way a kernel
    could be: ``pivot_slip`` scales every reciprocal pivot by 1 + slip, and
    ``skip_tile = (I, J)`` leaves the first panel's update of the 16x16 tile
    (I, J) out.  The tests use them to show that they would notice."""
    A = np.array(A, dtype=np.float32)
    x = np.array(b, dtype=np.float32)
    k = A.shape[0]
    inv = np.zeros(k, dtype=np.float32)
    for j in range(k):
        inv[j] = np.float32(1.0 + pivot_slip) / A[j, j]
        col = A[j + 1:, j].copy()
        upd = np.outer(col * inv[j], col).astype(np.float32)
        if skip_tile is not None and j < 16:
            r0, c0 = (16 * t - (j + 1) for t in skip_tile)
            upd[r0:r0 + 16, c0:c0 + 16] = 0
        A[j + 1:, j + 1:] -= upd
    for j in range(k):                       # (I + Ls) y = b
        x[j + 1:] -= A[j + 1:, j] * (x[j] * inv[j])
    x *= inv                                 # w = y / D
    for c in range(k - 1, 0, -1):            # (I + Ls^T) x = w
        x[:c] -= A[c, :c] * inv[:c] * x[c]
    return x


def ldl_left_looking(A, b):
    """The same factorisation, left-looking: column j is formed from all the
    earlier columns just before it is used (another summation order)."""
    A = np.array(A, dtype=np.float32)
    x = np.array(b, dtype=np.float32)
    k = A.shape[0]
    inv = np.zeros(k, dtype=np.float32)
    for j in range(k):
        for m in range(j):
            A[j:, j] -= A[j:, m] * (A[j, m] * inv[m])
        inv[j] = np.float32(1.0) / A[j, j]
    for i in range(k):
        for j in range(i):
            x[i] -= A[i, j] * inv[j] * x[j]
    x *= inv
    for i in range(k - 1, -1, -1):
        for c in range(k - 1, i, -1):
            x[i] -= A[c, i] * inv[i] * x[c]
    return x


def _one_row_csr(p):
    return CSR(torch.tensor([0, p.n]), p.indices, p.values, 1,
               p.table.shape[0])


def _check_piece(p, gather):
    """fp32 reference == float64 oracle == closed form, and both plain LDL^T
    return x_true."""
    csr = _one_row_csr(p)
    tab = fx.to_gather(p.table, gather)
    zero = torch.zeros(p.k, p.k)
    if p.scale is None:
        A32, b32 = R.gramian_reference(fx.pair_csr(csr, gather),
                                       R._table_f32(tab), p.reg)
        A64, b64 = R.gramian_weighted_f64(csr, tab, p.reg,
                                          torch.ones(p.n), p.values, zero)
    else:
        A32, b32 = R.gramian_weighted_reference(csr, tab, p.reg, p.scale,
                                                p.values, p.base)
        A64, b64 = R.gramian_weighted_f64(csr, tab, p.reg, p.scale,
                                          p.values, p.base)
        # the base really is split off: the stored part alone is not A
        As, _ = R.gramian_weighted_reference(csr, tab, p.reg, p.scale,
                                             p.values, zero)
        assert not torch.equal(As[0], p.A)
    assert torch.equal(A32.double(), A64) and torch.equal(b32.double(), b64)
    assert torch.equal(A32[0], p.A) and torch.equal(b32[0], p.b)
    assert torch.equal(p.A, p.A.T)
    for solve in (ldl_right_looking, ldl_left_looking):
        x = torch.from_numpy(solve(p.A.numpy(), p.b.numpy()))
        assert torch.equal(x, p.x_true), solve.__name__
    return A32[0], b32[0]


@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", RANKS)
def test_ldl_family(k, gather):
    for n in (k, k + 1, 257):
        p = fx.ldl_family(k, n, seed=10 * k + n, gather=gather)
        assert p.n == n and p.reg == 0.0
        _check_piece(p, gather)
        assert bool((p.x_true != 0).any()) and bool((p.x_true == 0).any())
        # the real entries straddle the 32-entry chunks when n allows it
        real = p.table[p.indices.long()].abs().sum(1) != 0
        assert int(real.sum()) == k
        assert bool((p.values[~real] == fx.PAD_RATING).all())
        if n == 257:
            assert len({int(i) // 32 for i in real.nonzero()[:, 0]}) > 2


@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", RANKS)
def test_diag_family(k, gather):
    p = fx.diag_family(k, gather)
    want_n = {16: 28, 32: 60, 48: 60, 64: 124, 80: 124, 96: 124, 112: 124,
              128: 252}[k]
    assert p.n == want_n == fx.diag_n(k)
    A, b = _check_piece(p, gather)
    d = float(A[0, 0])
    assert d == 1.0 + 0.25 * p.n and torch.equal(A, d * torch.eye(k))
    assert torch.equal(p.x_true * d, b)
    # some ratings have a non-zero low half: the pair's second column matters
    hi = R._round_gather(p.values, gather)
    real = p.table[p.indices.long()].abs().sum(1) != 0
    assert bool(((p.values - hi)[real] != 0).any())


@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", RANKS)
def test_weighted_family(k, gather):
    for n in (k, k + 1, 129 if k < 129 else k):
        p = fx.weighted_family(k, n, seed=20 * k + n, gather=gather)
        _check_piece(p, gather)
        assert float(p.values.abs().max()) <= 16
        d = set((p.scale[p.values != fx.PAD_RATING] ** 2).tolist())
        assert d <= {1.0, 4.0}
    L, s, gd = fx.weighted_shared(k)
    assert set((s * s + gd).tolist()) == {2.0, 4.0, 8.0}


@pytest.mark.parametrize("k", RANKS)
def test_graded_system(k):
    conds = []
    for seed in range(3):
        gs = fx.graded_system(k, seed=300 + 7 * k + seed)
        assert float(gs.D.min()) >= 2.0 ** -6 and float(gs.D.max()) <= 64
        assert int(gs.x_true.abs().max()) <= 3
        for solve in (ldl_right_looking, ldl_left_looking):
            x = torch.from_numpy(solve(gs.A.numpy(), gs.b.numpy()))
            assert torch.equal(x, gs.x_true), solve.__name__
        conds.append(float(torch.linalg.cond(gs.A.double())))
        # no -0.0 in the right-hand side
        assert not bool(((gs.b == 0) & (gs.b.view(torch.int32) != 0)).any())
    assert max(conds) > 1e4, conds
    A, b, x = fx.graded_batch(k, 5, seed=1, xmax=1)
    assert A.shape == (5, k, k) and int(x.abs().max()) == 1
    assert torch.equal(ops.dequantize_fp8(ops.quantize_fp8(x)), x)


@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", RANKS)
def test_integer_gramian_case(k, gather):
    csr, tab, tab32, scale = fx.integer_gramian_case(
        k, gather, ROW_LENGTHS, seed=500 + k)
    assert csr.row_counts().tolist() == list(ROW_LENGTHS)
    zero = torch.zeros(k, k)
    A32, b32 = R.gramian_reference(fx.pair_csr(csr, gather), tab32, 0.25)
    A64, b64 = R.gramian_weighted_f64(csr, tab, 0.25, torch.ones(csr.nnz),
                                      csr.values, zero)
    assert torch.equal(A32.double(), A64) and torch.equal(b32.double(), b64)
    Aw, bw = R.gramian_weighted_reference(csr, tab, 0.25, scale, csr.values,
                                          zero)
    Aw64, bw64 = R.gramian_weighted_f64(csr, tab, 0.25, scale, csr.values,
                                        zero)
    assert torch.equal(Aw.double(), Aw64) and torch.equal(bw.double(), bw64)
    assert not torch.equal(Aw, A32)
    # the 65th rating of the 65-row is visible in its own A and b
    row = ROW_LENGTHS.index(65)
    s = int(csr.indptr[row])
    q = tab32[int(csr.indices[s + 64])]
    assert bool((q != 0).any())
    # non-integer ratings up to 129 entries, integers beyond
    long_vals = csr.values[int(csr.indptr[ROW_LENGTHS.index(160)]):]
    assert torch.equal(long_vals, long_vals.round())
    assert not torch.equal(csr.values, csr.values.round())


@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", [16, 64, 128])
def test_fixture_is_sensitive(k, gather):
    n = k + 5
    p = fx.ldl_family(k, n, seed=77 + k, gather=gather)
    csr = _one_row_csr(p)
    tab32 = p.table
    # dropping any one stored entry (real or padding) changes A, b or n
    for drop in range(n):
        keep = torch.arange(n) != drop
        sub = CSR(torch.tensor([0, n - 1]), p.indices[keep], p.values[keep],
                  1, csr.num_cols)
        A, b = R.gramian_reference(sub, tab32, 0.25)
        A0, b0 = R.gramian_reference(csr, tab32, 0.25)
        assert not (torch.equal(A, A0) and torch.equal(b, b0)), drop
        if bool((tab32[int(p.indices[drop])] != 0).any()):
            A, _ = R.gramian_reference(sub, tab32, 0.0)
            assert not torch.equal(A[0], p.A), drop
    # moving one entry of L across a tile boundary changes the solution
    if k > 16:
        rows, cols = torch.nonzero(torch.tril(p.L, -1), as_tuple=True)
        # (unless x_true agrees on the two rows and (L^T x_true)_c is zero:
        # then b is in the moved matrix's range with the same x, which
        # happens for a minority of the entries)
        L64 = p.L.double()
        d = torch.diag(torch.linalg.solve(L64, p.A.double())
                       @ torch.linalg.inv(L64.T))
        m = L64.T @ p.x_true.double()
        moved = changed = 0
        for r, c in zip(rows.tolist(), cols.tolist()):
            r2 = r + 16 if r + 16 < k else r - 16
            if r2 <= c or p.L[r2, c] != 0:
                continue
            L2 = L64.clone()
            L2[r2, c], L2[r, c] = L2[r, c], 0.0
            x2 = torch.linalg.solve((L2 * d) @ L2.T, p.b.double())
            same = torch.allclose(x2, p.x_true.double(), atol=1e-6)
            assert same == (p.x_true[r] == p.x_true[r2] and m[c] == 0)
            moved += 1
            changed += not same
        assert moved > 0 and changed > moved // 2, (moved, changed)


@pytest.mark.parametrize("k", [32, 64, 128])
def test_exact_check_sees_a_wrong_solver(k):
    """What the existing allclose(1e-3) solver tests let through -- a pivot
    scaled by 1 + 1e-4, one tile update left out -- fails the equality."""
    gs = fx.graded_system(k, seed=900 + k)
    A, b = gs.A.numpy(), gs.b.numpy()
    x = torch.from_numpy(ldl_right_looking(A, b, pivot_slip=1e-4))
    assert not torch.equal(x, gs.x_true)
    # every off-diagonal tile of L is non-empty, so the first panel's update
    # of every later diagonal tile is non-zero
    for I in range(1, k // 16):
        x = torch.from_numpy(ldl_right_looking(A, b, skip_tile=(I, I)))
        assert not torch.equal(x, gs.x_true), I


@pytest.mark.parametrize("gather", GATHERS)
def test_values_survive_the_gather_dtypes(gather):
    for k in RANKS:
        pieces = [fx.ldl_family(k, k + 3, seed=k, gather=gather),
                  fx.diag_family(k, gather),
                  fx.weighted_family(k, k + 3, seed=k, gather=gather)]
        for p in pieces:
            if gather == "fp8":
                q = ops.quantize_fp8(p.table)
                assert torch.equal(ops.dequantize_fp8(q), p.table)
                assert torch.equal(ops.fp8_rating_pair(p.values), p.values)
            else:
                assert torch.equal(p.table.to(torch.bfloat16).float(),
                                   p.table)
                assert torch.equal(ops.bf16_rating_pair(p.values), p.values)
            assert torch.equal(R.rating_pair(p.values, gather), p.values)
            if p.scale is not None:
                rows, pair = R.effective_rows(
                    _one_row_csr(p), fx.to_gather(p.table, gather), p.scale,
                    p.values)
                assert torch.equal(
                    rows, p.scale.unsqueeze(1) * p.table[p.indices.long()])
                assert torch.equal(pair, p.values)
    for name, vals in (("bf16", fx.RATINGS["bf16"]),
                       ("fp8", fx.RATINGS["fp8"])):
        v = torch.tensor(vals)
        assert torch.equal(R.rating_pair(v, name), v)


def test_combine_stacks_pieces():
    k = 32
    pieces = [fx.ldl_family(k, 40, seed=1, gather="bf16"), fx.empty_piece(k),
              fx.ldl_family(k, 32, seed=2, gather="bf16")]
    bt = fx.combine(pieces, "bf16")
    assert bt.csr.row_counts().tolist() == [40, 0, 32]
    A, b = R.gramian_reference(bt.csr, bt.table_f32, bt.reg)
    assert torch.equal(A, bt.A) and torch.equal(b, bt.b)
    x = R.als_solve_side_reference(bt.csr, bt.table_f32, bt.reg)
    assert torch.allclose(x, bt.x_true, atol=1e-4)
    assert bool((x[1] == 0).all())
