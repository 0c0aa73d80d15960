"""Exact-integer inputs for the ALS Gramian, LDL and fused kernels (CPU-only
builders, seeded; docs/KERNELS.md "Exact-integer cases").

Every family is built so that each quantity a correct kernel can form -- a
Gramian partial sum in any order, a Schur complement, a raw column ``L*D``,
a reciprocal pivot, a partial sum of either substitution -- is an integer
times a power of two with far fewer significant bits than the accumulator
keeps (24 for fp32, about 17 measured for the fp8 MFMA).  No rounding ever
happens, so the answer does not depend on the order of the operations and
the tests compare with ``torch.equal``.

The construction: ``L`` unit lower triangular with entries in {-1, 0, 1},
about three off-diagonal entries per column at random rows and at least one
in every off-diagonal 16x16 tile; ``D`` a diagonal of powers of two;
``x_true`` small integers.  ``A = L D L^T`` and ``b = A x_true``.

A ``Piece`` is one entity: its stored entries (rows of its own small factor
table, ratings), the closed-form ``A`` and ``b`` (regularisation included)
and the exact solution.  ``combine`` stacks pieces into one CSR + one table.
"""

from dataclasses import dataclass
from typing import Optional

import torch

from flink_ms_amd import ops
from flink_ms_amd.data.blocked import CSR
from flink_ms_amd.ops import reference as R

# non-integer ratings that survive the hi/lo rating pair of each gather
# dtype unchanged, with a non-zero low half (hi + lo == r exactly)
RATINGS = {"bf16": (1.0 + 2.0 ** -9, 3.0 + 2.0 ** -8, 5.0, -2.0),
           "fp8": (1.0625, 2.125, 3.0, -4.0)}
INT_RATINGS = (1.0, 3.0, 5.0, -2.0)
PAD_RATING = 5.0
# Row lengths of the multi-row Gramian case: the 32-rating chunk, the bf16
# two-chunk and fp8 four-chunk rounds, the 2-wave staging team of bf16 at
# k >= 80, and an empty row in the middle of the launch
ROW_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 0, 65, 97, 127, 128, 129, 160, 257)
# significant bits a Gramian partial sum may need (integer_gramian_case)
MAX_BITS = {"bf16": 20, "fp8": 14}
# (scale, base diagonal g, pivot d = scale^2 + g) choices of weighted_family,
# with d / scale, the factor between (L^T x)_j and ext_j
_WEIGHT_CHOICES = ((2.0, 0.0, 4.0), (1.0, 1.0, 2.0), (1.0, 3.0, 4.0),
                   (2.0, 4.0, 8.0), (1.0, 7.0, 8.0))


@dataclass(frozen=True)
class Piece:
    k: int
    indices: torch.Tensor          # int32 [n], rows of ``table``
    values: torch.Tensor           # fp32 [n]: ratings (ext when weighted)
    table: torch.Tensor            # fp32 [rows, k], exact in the gather dtype
    x_true: torch.Tensor           # fp32 [k]
    A: torch.Tensor                # fp32 [k, k] closed form, reg*n*I included
    b: torch.Tensor                # fp32 [k] closed form
    reg: float
    scale: Optional[torch.Tensor] = None   # fp32 [n], weighted pieces only
    base: Optional[torch.Tensor] = None    # fp32 [k, k], weighted pieces only
    L: Optional[torch.Tensor] = None

    @property
    def n(self):
        return int(self.indices.numel())


@dataclass(frozen=True)
class Batch:
    csr: CSR
    table: torch.Tensor            # bf16, or uint8 e4m3 bytes
    table_f32: torch.Tensor
    x_true: torch.Tensor           # fp32 [rows, k]
    A: torch.Tensor                # fp32 [rows, k, k]
    b: torch.Tensor                # fp32 [rows, k]
    reg: float
    gather: str
    scale: Optional[torch.Tensor] = None
    base: Optional[torch.Tensor] = None


def to_gather(t: torch.Tensor, gather: str) -> torch.Tensor:
    """fp32 -> the stored table dtype; asserts that nothing is rounded."""
    out = ops.quantize_fp8(t) if gather == "fp8" else t.to(torch.bfloat16)
    assert torch.equal(R._table_f32(out), t), "table not exact in " + gather
    return out


def unit_lower(k: int, g: torch.Generator) -> torch.Tensor:
    """Unit lower triangular [k, k] fp32 with entries in {-1, 0, 1}: three
    off-diagonal entries per column where the column has room, at random
    rows, plus one in every off-diagonal 16x16 tile that got none (put into
    the tile's emptiest column).  At most 7 off-diagonal entries per column,
    so |(L^T x)_j| <= 8 for x in {-1, 0, 1}^k."""
    L = torch.eye(k)
    for j in range(k - 1):
        rows = torch.randperm(k - 1 - j, generator=g)[:3] + j + 1
        L[rows, j] = (torch.randint(0, 2, (rows.numel(),), generator=g)
                      * 2 - 1).float()
    for I in range(1, k // 16):
        for J in range(I):
            if L[16 * I:16 * I + 16, 16 * J:16 * J + 16].any():
                continue
            cnt = (L[:, 16 * J:16 * J + 16] != 0).sum(0)
            c = 16 * J + int(cnt.argmin())
            r = 16 * I + int(torch.randint(0, 16, (1,), generator=g))
            L[r, c] = float(int(torch.randint(0, 2, (1,), generator=g)) * 2 - 1)
    assert torch.equal(L, torch.tril(L)) and bool((L.diagonal() == 1).all())
    assert int(((L != 0).sum(0) - 1).max()) <= 7
    for I in range(1, k // 16):
        for J in range(I):
            assert bool(L[16 * I:16 * I + 16, 16 * J:16 * J + 16].any())
    return L


def _exact32(t64: torch.Tensor) -> torch.Tensor:
    t32 = t64.to(torch.float32)
    assert torch.equal(t32.double(), t64), "not exact in fp32"
    return t32


def _closed_form(L, d, x):
    """(A, b) = (L D L^T, A x) computed in float64, exact in fp32."""
    L64 = L.double()
    A = (L64 * d.double()) @ L64.T
    return _exact32(A), _exact32(A @ x.double())


def _scatter_entries(n, k, g):
    """Positions of the k real entries among n, and where the padding goes."""
    assert n >= k
    pos = torch.randperm(n, generator=g)[:k]
    return pos


def empty_piece(k: int) -> Piece:
    z = torch.zeros(0)
    return Piece(k, z.to(torch.int32), z.clone(), torch.zeros(1, k),
                 torch.zeros(k), torch.zeros(k, k), torch.zeros(k), 0.0)


def ldl_family(k: int, n: int, seed: int, gather: str) -> Piece:
    """One entity whose Gramian is ``A = L D L^T`` with ``reg = 0``: k stored
    entries with factor rows ``s_j * L[:, j]`` (s_j in {1, 2}, d_j = s_j^2)
    and ratings ``s_j * (L^T x_true)_j`` (integers of magnitude <= 8,
    x_true in {-1, 0, 1}^k), at random positions among n; the other n - k
    entries point at an all-zero row and carry rating 5."""
    g = torch.Generator().manual_seed(seed)
    L = unit_lower(k, g)
    x = torch.randint(-1, 2, (k,), generator=g).float()
    m = L.T @ x
    s = torch.randint(1, 3, (k,), generator=g).float()
    s[m.abs() > 4] = 1.0
    r = s * m
    assert float(r.abs().max()) <= 8
    # table rows in a shuffled order, the zero row somewhere among them
    perm = torch.randperm(k + 1, generator=g)
    table = torch.zeros(k + 1, k)
    table[perm[:k]] = (L * s).T
    indices = torch.full((n,), int(perm[k]), dtype=torch.int32)
    values = torch.full((n,), PAD_RATING)
    pos = _scatter_entries(n, k, g)
    indices[pos] = perm[:k].to(torch.int32)
    values[pos] = r
    A, b = _closed_form(L, s * s, x)
    assert float(A.abs().max()) < 100 and float(b.abs().max()) < 100
    assert torch.equal(R.rating_pair(values, gather), values)
    assert torch.equal(R._round_gather(values, gather), values)   # lo == 0
    return Piece(k, indices, values, table, x, A, b, 0.0, L=L)


def diag_n(k: int) -> int:
    """n = 4 * (2^p - 1), the smallest such n >= k."""
    p = 1
    while 4 * (2 ** p - 1) < k:
        p += 1
    return 4 * (2 ** p - 1)


def diag_family(k: int, gather: str, reg: float = 0.25) -> Piece:
    """The regularised companion: the k unit vectors, each stored once, plus
    zero-row padding up to n = 4 * (2^p - 1), so that with reg = 0.25
    ``A = (1 + reg * n) * I = 2^p * I`` and ``x = b / 2^p`` exactly.  Ratings
    are non-integers with a non-zero low half of the rating pair."""
    assert reg == 0.25
    n = diag_n(k)
    g = torch.Generator().manual_seed(7000 + k)
    perm = torch.randperm(k + 1, generator=g)
    table = torch.zeros(k + 1, k)
    table[perm[:k]] = torch.eye(k)
    rset = torch.tensor(RATINGS[gather])
    values = rset[torch.randint(0, 4, (n,), generator=g)]
    indices = torch.full((n,), int(perm[k]), dtype=torch.int32)
    pos = _scatter_entries(n, k, g)
    indices[pos] = perm[:k].to(torch.int32)
    assert torch.equal(R.rating_pair(values, gather), values)
    assert not torch.equal(R._round_gather(values, gather), values)
    diag = 1.0 + reg * n
    assert diag == 2.0 ** round(torch.log2(torch.tensor(diag)).item())
    b = values[pos].clone()
    return Piece(k, indices, values, table, b / diag, diag * torch.eye(k), b,
                 reg)


_WEIGHTED_SHARED = {}


def weighted_shared(k: int):
    """(L, scale-per-column s, base diagonal g) shared by every entity of a
    weighted launch (they share the one base matrix)."""
    if k not in _WEIGHTED_SHARED:
        g = torch.Generator().manual_seed(9000 + k)
        L = unit_lower(k, g)
        cnt = (L != 0).sum(0)              # |(L^T x)_j| <= cnt_j
        s = torch.zeros(k)
        gd = torch.zeros(k)
        for j in range(k):
            ok = [c for c in _WEIGHT_CHOICES
                  if c[2] / c[0] * int(cnt[j]) <= 16]
            c = ok[int(torch.randint(0, len(ok), (1,), generator=g))]
            s[j], gd[j] = c[0], c[1]
        d = s * s + gd
        assert set(d.tolist()) == {2.0, 4.0, 8.0}
        _WEIGHTED_SHARED[k] = (L, s, gd)
    return _WEIGHTED_SHARED[k]


def weighted_base(k: int) -> torch.Tensor:
    L, _, gd = weighted_shared(k)
    return _exact32((L.double() * gd.double()) @ L.double().T)


def weighted_family(k: int, n: int, seed: int, gather: str) -> Piece:
    """One entity of the weighted kernels: stored rows ``L[:, j]`` with
    scales s_j in {1, 2}, the base ``G0 = L diag(g) L^T`` with
    ``d_j = s_j^2 + g_j`` in {2, 4, 8}, and ``ext_j = d_j (L^T x)_j / s_j``
    (integers of magnitude <= 16), so that the weighted normal equations are
    ``L D L^T x = L D L^T x_true`` exactly.  Padding: zero row, scale 1."""
    L, s, gd = weighted_shared(k)
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (k,), generator=g).float()
    d = s * s + gd
    ext = d * (L.T @ x) / s
    assert float(ext.abs().max()) <= 16 and torch.equal(ext, ext.round())
    table = torch.cat([L.T.contiguous(), torch.zeros(1, k)])
    indices = torch.full((n,), k, dtype=torch.int32)
    values = torch.full((n,), PAD_RATING)
    scale = torch.ones(n)
    pos = _scatter_entries(n, k, g)
    indices[pos] = torch.arange(k, dtype=torch.int32)
    values[pos] = ext
    scale[pos] = s
    A, b = _closed_form(L, d, x)
    assert torch.equal(R.rating_pair(values, gather), values)
    return Piece(k, indices, values, table, x, A, b, 0.0, scale=scale,
                 base=weighted_base(k), L=L)


def empty_weighted_piece(k: int) -> Piece:
    z = torch.zeros(0)
    return Piece(k, z.to(torch.int32), z.clone(), torch.zeros(1, k),
                 torch.zeros(k), weighted_base(k), torch.zeros(k), 0.0,
                 scale=z.clone(), base=weighted_base(k))


def combine(pieces, gather: str) -> Batch:
    """Stack pieces (one CSR row each) over the concatenation of their
    tables."""
    k = pieces[0].k
    reg = max(p.reg for p in pieces)
    assert all(p.k == k and (p.n == 0 or p.reg == reg) for p in pieces)
    off, idx = 0, []
    for p in pieces:
        idx.append(p.indices + off)
        off += p.table.shape[0]
    lengths = torch.tensor([p.n for p in pieces], dtype=torch.int64)
    indptr = torch.zeros(len(pieces) + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=indptr[1:])
    table = torch.cat([p.table for p in pieces])
    csr = CSR(indptr, torch.cat(idx).to(torch.int32),
              torch.cat([p.values for p in pieces]), len(pieces), off)
    weighted = pieces[0].scale is not None
    return Batch(csr, to_gather(table, gather), table,
                 torch.stack([p.x_true for p in pieces]),
                 torch.stack([p.A for p in pieces]),
                 torch.stack([p.b for p in pieces]), reg, gather,
                 torch.cat([p.scale for p in pieces]) if weighted else None,
                 pieces[0].base if weighted else None)


@dataclass(frozen=True)
class Graded:
    L: torch.Tensor
    D: torch.Tensor
    x_true: torch.Tensor
    A: torch.Tensor
    b: torch.Tensor


def graded_system(k: int, seed: int, xmax: int = 3) -> Graded:
    """One system for the solvers that are given A directly: ``D = 2^e`` with
    e in [-6, 6] (cond up to about 1e7 with L), x_true in {-xmax..xmax}^k,
    ``A = L D L^T`` and ``b = A x_true`` exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    L = unit_lower(k, g)
    D = 2.0 ** torch.randint(-6, 7, (k,), generator=g).float()
    x = torch.randint(-xmax, xmax + 1, (k,), generator=g).float()
    A, b = _closed_form(L, D, x)
    return Graded(L, D, x, A, b + 0.0)        # + 0.0: no -0.0 in b


def graded_batch(k: int, count: int, seed: int, xmax: int = 3):
    """(A [count, k, k], b [count, k], x_true [count, k])."""
    sy = [graded_system(k, seed + i, xmax) for i in range(count)]
    return (torch.stack([s.A for s in sy]).contiguous(),
            torch.stack([s.b for s in sy]).contiguous(),
            torch.stack([s.x_true for s in sy]).contiguous())


def _bits(abs_sum: torch.Tensor, granule: float) -> int:
    """Significant bits that any partial sum of terms on the grid ``granule``
    with the given sum of magnitudes can need."""
    if abs_sum.numel() == 0:
        return 0
    top = float(abs_sum.max()) / granule
    return 0 if top < 1 else int(torch.tensor(top).log2().floor()) + 1


def integer_gramian_case(k: int, gather: str, lengths, seed: int,
                         ncols: int = 50):
    """Multi-row CSR over a small-integer table (values in {-2..2} for bf16,
    {-1, 0, 1} for fp8; row 0 all zero) with ratings from ``RATINGS`` (rows
    longer than 129: integer ratings only) and scales in {1, 2} for the
    weighted form.  Asserts from sum|terms| that no partial sum of A or b,
    explicit or weighted, needs more than ``MAX_BITS[gather]`` bits.
    Returns (csr, table, table_f32, scale)."""
    g = torch.Generator().manual_seed(seed)
    lim = 2 if gather == "bf16" else 1
    table = torch.randint(-lim, lim + 1, (ncols, k), generator=g).float()
    table[0] = 0.0
    lengths = torch.tensor(list(lengths), dtype=torch.int64)
    nnz = int(lengths.sum())
    indptr = torch.zeros(lengths.numel() + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=indptr[1:])
    indices = torch.randint(0, ncols, (nnz,), generator=g).to(torch.int32)
    pick = torch.randint(0, 4, (nnz,), generator=g)
    values = torch.tensor(RATINGS[gather])[pick]
    rid = torch.repeat_interleave(torch.arange(lengths.numel()), lengths)
    long_row = lengths[rid] > 129
    values[long_row] = torch.tensor(INT_RATINGS)[pick][long_row]
    scale = torch.randint(1, 3, (nnz,), generator=g).float()
    assert torch.equal(R.rating_pair(values, gather), values)
    # granule of the b terms: the low halves of the rating pairs
    lo = (values - R._round_gather(values, gather)).abs()
    q = table[indices.long()].abs().double()
    for sc in (torch.ones(nnz), scale):
        qs = q * sc.double().unsqueeze(1)
        sumA = torch.zeros(lengths.numel(), k, k, dtype=torch.float64)
        sumA.index_add_(0, rid, qs.unsqueeze(2) * qs.unsqueeze(1))
        sumb = torch.zeros(lengths.numel(), k, dtype=torch.float64)
        sumb.index_add_(0, rid, qs * values.abs().double().unsqueeze(1))
        frac = torch.zeros(lengths.numel())
        frac.index_add_(0, rid, (lo > 0).float())
        gran = float(lo[lo > 0].min()) if bool((lo > 0).any()) else 1.0
        assert _bits(sumA, 1.0) <= MAX_BITS[gather]
        assert _bits(sumb[frac > 0], gran) <= MAX_BITS[gather]
        if bool((frac == 0).any()):
            assert _bits(sumb[frac == 0], 1.0) <= MAX_BITS[gather]
    csr = CSR(indptr, indices, values, lengths.numel(), ncols)
    return csr, to_gather(table, gather), table, scale


def pair_csr(csr: CSR, gather: str) -> CSR:
    """The CSR with every rating replaced by its dequantised hi/lo pair."""
    return CSR(csr.indptr, csr.indices, R.rating_pair(csr.values, gather),
               csr.num_rows, csr.num_cols)
