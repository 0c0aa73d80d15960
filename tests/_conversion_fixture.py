"""Edge sets, independent oracles and exact one-term systems for the e4m3 /
bf16 conversions of the ALS kernels (CPU-only builders; docs/KERNELS.md
"Conversions").

The contract (``common.hip.h``, ``ops.quantize_fp8``): e4m3 encodes round to
nearest, ties to the even byte; finite values beyond +-448 saturate; inf and
NaN become a NaN byte; decodes are exact.  bf16 encodes are RNE on the bit
pattern (overflow to inf), NaN stays NaN.

Every system built here has ONE stored entry that matters per entity, a
diagonal ``A`` made of powers of two and a right-hand side with one non-zero
element, so the arithmetic around the conversion under test is exact and the
GPU tests compare bit patterns.  tests/test_conversions_cpu.py checks these
claims (and the oracles) without a GPU.
"""

import functools
from dataclasses import dataclass
from typing import Optional

import torch

from flink_ms_amd import ops
from flink_ms_amd.data.blocked import CSR
from flink_ms_amd.ops import reference as R

INF = float("inf")
NAN = float("nan")
BEYOND_E4M3 = (465.0, 480.0, 1e4, 3.4e38)


# ------------------------------------------------------------------ oracles

@functools.lru_cache(maxsize=None)
def e4m3_table() -> torch.Tensor:
    """The 127 non-negative finite OCP e4m3fn values, by byte, in float64,
    from the format's definition (bias 7, 3 mantissa bits, subnormals at
    exponent field 0): no cast involved."""
    vals = []
    for byte in range(127):
        e, m = byte >> 3, byte & 7
        vals.append(m * 2.0 ** -9 if e == 0
                    else (1 + m / 8.0) * 2.0 ** (e - 7))
    t = torch.tensor(vals, dtype=torch.float64)
    assert bool((t[1:] > t[:-1]).all()) and float(t[-1]) == 448.0
    return t


def e4m3_oracle(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> e4m3 bytes by table search: the nearest of the 127 magnitudes,
    a tie to the even byte, anything finite past 448 to 448, inf / NaN to
    0x7F; the sign bit on top (so -0 and negative underflow give 0x80)."""
    x = x.to(torch.float32)
    tab = e4m3_table()
    a = x.abs().double()
    fin = torch.isfinite(a)
    a = torch.where(fin, a, torch.zeros_like(a)).clamp(max=448.0)
    hi = torch.searchsorted(tab, a).clamp(1, 126)     # tab[hi - 1] <= a
    lo = hi - 1
    dlo, dhi = a - tab[lo], tab[hi] - a
    pick_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    byte = torch.where(pick_hi, hi, lo)
    byte = torch.where(fin, byte, torch.full_like(byte, 0x7F))
    sign = (x.view(torch.int32) < 0).long() << 7
    return (byte | sign).to(torch.uint8)


def e4m3_decode_oracle(b: torch.Tensor) -> torch.Tensor:
    """e4m3 bytes -> fp32 by the table (0x7F / 0xFF -> NaN)."""
    b = b.long()
    mag = b & 0x7F
    v = e4m3_table()[mag.clamp(max=126)].float()
    v = torch.where(mag == 0x7F, torch.full_like(v, NAN), v)
    return torch.where((b & 0x80) != 0, -v, v)


def bf16_oracle(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 bit patterns (int16) by RNE on the bits in integer
    arithmetic; NaN -> 0x7FC0 (compare NaNs with :func:`canon_nan`)."""
    u = x.to(torch.float32).contiguous().view(torch.int32).long() & 0xFFFFFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    r = torch.where(nan, torch.full_like(r, 0x7FC0), r)
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)


def canon_nan(t: torch.Tensor) -> torch.Tensor:
    """Bit patterns (fp32 -> int32, bf16 -> int16, e4m3 bytes as they are)
    with every NaN replaced by one canonical NaN: a NaN compares as "is a
    NaN" only, its sign and payload are not pinned."""
    t = t.contiguous()
    if t.dtype == torch.float32:
        b = t.view(torch.int32).clone()
        b[(b & 0x7FFFFFFF) > 0x7F800000] = 0x7FC00000
        return b
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    if t.dtype == torch.int16:
        b = t.clone()
        b[(b.to(torch.int32) & 0x7FFF) > 0x7F80] = 0x7FC0
        return b
    assert t.dtype == torch.uint8
    b = t.clone()
    b[(b & 0x7F) == 0x7F] = 0x7F
    return b


def oracle_pair(r: torch.Tensor, gather: str) -> torch.Tensor:
    """The hi/lo rating pair of ``r``, dequantised, by the oracles alone."""
    r = r.to(torch.float32)
    if gather == "fp8":
        hi = e4m3_decode_oracle(e4m3_oracle(r))
        return hi + e4m3_decode_oracle(e4m3_oracle(r - hi))
    hi = bf16_oracle(r).view(torch.bfloat16).float()
    return hi + bf16_oracle(r - hi).view(torch.bfloat16).float()


# ---------------------------------------------------------------- edge sets

def _ulp_neighbours(x: torch.Tensor):
    return (torch.nextafter(x, torch.full_like(x, -INF)),
            torch.nextafter(x, torch.full_like(x, INF)))


@functools.lru_cache(maxsize=None)
def e4m3_midpoints() -> torch.Tensor:
    """The 126 midpoints between neighbouring non-negative e4m3 values
    (exact in fp32: checked)."""
    tab = e4m3_table()
    mid64 = (tab[1:] + tab[:-1]) / 2
    mid = mid64.float()
    assert torch.equal(mid.double(), mid64)
    return mid


@functools.lru_cache(maxsize=None)
def e4m3_edges() -> torch.Tensor:
    """The 1022 finite fp32 edge values of the e4m3 encoders: the 127
    non-negative values, the 126 midpoints, each midpoint -+ one fp32 ulp,
    464 (the midpoint of 448 and the first value beyond the range) and its
    fp32 predecessor, 465, 480, 1e4, 3.4e38, and the negatives of all."""
    mid = e4m3_midpoints()
    below, above = _ulp_neighbours(mid)
    t464 = torch.tensor([464.0])
    pos = torch.cat([e4m3_table().float(), mid, below, above, t464,
                     _ulp_neighbours(t464)[0], torch.tensor(BEYOND_E4M3)])
    out = torch.cat([pos, -pos])
    assert out.numel() == 1022 and bool(torch.isfinite(out).all())
    return out


def specials() -> torch.Tensor:
    """+-0, +-inf and a NaN."""
    return torch.tensor([0.0, -0.0, INF, -INF, NAN])


BF16_EXPONENTS = (-127, -126, -1, 0, 7, 127)


@functools.lru_cache(maxsize=None)
def bf16_values() -> torch.Tensor:
    """The 768 non-negative bf16 values with all 128 mantissas at exponents
    -127 (subnormal), -126, -1, 0, 7, 127, as int32 bf16 patterns."""
    pats = [((e + 127) << 7) | m for e in BF16_EXPONENTS for m in range(128)]
    return torch.tensor(pats, dtype=torch.int32)


def _f32_of_bits(bits: torch.Tensor) -> torch.Tensor:
    return bits.to(torch.int32).contiguous().view(torch.float32)


@functools.lru_cache(maxsize=None)
def bf16_edges() -> torch.Tensor:
    """fp32 edge values of the bf16 encoders: the values of
    :func:`bf16_values`, the midpoint to the next bf16 value, each midpoint
    -+ one fp32 ulp, the negatives of all, the largest finite fp32 (rounds
    to inf) and -0."""
    p = bf16_values() << 16
    pos = torch.cat([_f32_of_bits(p), _f32_of_bits(p + 0x8000),
                     _f32_of_bits(p + 0x7FFF), _f32_of_bits(p + 0x8001)])
    assert bool(torch.isfinite(pos).all())
    out = torch.cat([pos, -pos, torch.tensor([3.4028234663852886e38, -0.0])])
    return out


# ------------------------------------------------------------ value classes

def is_e4m3_tie(x):
    a = x.abs()
    return torch.isin(a, torch.cat([e4m3_midpoints(), torch.tensor([464.0])]))


def is_e4m3_subnormal(x):
    return (x != 0) & (x.abs() < 2.0 ** -6)


def is_e4m3_saturated(x):
    return torch.isfinite(x) & (x.abs() > 448.0)


def is_e4m3_negzero(x):
    """Values whose e4m3 image is the byte 0x80: -0 and negative underflow
    (|x| <= 2^-10, the tie going to the even byte 0)."""
    return (x.view(torch.int32) < 0) & (x.abs() <= 2.0 ** -10)


# ----------------------------------------------------------- one-term cases

@dataclass(frozen=True)
class Case:
    """Entity i has lengths[i] stored entries; the LAST one points at table
    row ``rows[i]`` with value ``values[i]`` (a rating, or ext), the ones
    before it at the all-zero row ``zero_row`` with value 1.  ``col[i]`` is
    the one column of entity i that is not zero."""
    csr: CSR
    table: torch.Tensor            # bf16, or uint8 e4m3 bytes; zero row last
    col: torch.Tensor              # int64 [N]
    reg: float
    lengths: torch.Tensor          # int64 [N]
    gather: str
    scale: Optional[torch.Tensor] = None     # fp32 [nnz]

    @property
    def n(self):
        return self.csr.num_rows

    def last(self):
        """CSR position of every entity's own entry."""
        return self.csr.indptr[1:] - 1


def _case(table, rows, values, col, reg, lengths, gather, scales=None):
    n = rows.numel()
    lengths = torch.as_tensor(lengths, dtype=torch.int64).expand(n).clone()
    indptr = torch.zeros(n + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=indptr[1:])
    nnz = int(indptr[-1])
    zero_row = table.shape[0] - 1
    assert not bool(table[zero_row].view(torch.uint8 if gather == "fp8"
                                         else torch.int16).any())
    indices = torch.full((nnz,), zero_row, dtype=torch.int32)
    vals = torch.ones(nnz)
    last = indptr[1:] - 1
    indices[last] = rows.to(torch.int32)
    vals[last] = values.float()
    scale = None
    if scales is not None:
        scale = torch.ones(nnz)
        scale[last] = scales.float()
    csr = CSR(indptr, indices, vals, n, table.shape[0])
    return Case(csr, table, col.long(), float(reg), lengths, gather, scale)


def to_gather(t32: torch.Tensor, gather: str) -> torch.Tensor:
    out = ops.quantize_fp8(t32) if gather == "fp8" else t32.to(torch.bfloat16)
    assert torch.equal(R._table_f32(out), t32), "table not exact in " + gather
    return out


def scaled_identity(k: int, t: float, gather: str) -> torch.Tensor:
    """[k + 1][k]: row j = t * e_j, the last row zero."""
    tab = torch.zeros(k + 1, k)
    tab[:k] = t * torch.eye(k)
    return to_gather(tab, gather)


def fused_ratings(gather: str, a: int) -> torch.Tensor:
    """Ratings of the image-encoder case: the e4m3 edges times 2^(1-a), so
    that x_j = 2^(a-1) * pair(r) walks the edge set again (exactly, where
    the rating pair holds r); -0 and +0 come with the set.  A rating whose
    pair is not finite in the gather dtype (3.4e38 rounds to inf in bf16) is
    left out: an inf would poison its whole row through 0 * inf."""
    r = e4m3_edges() * 2.0 ** (1 - a)
    x = 2.0 ** (a - 1) * R.rating_pair(r, gather)
    return r[torch.isfinite(x)]


def fused_case(k: int, gather: str, a: int, ratings=None, lengths=1,
               reg=None, t=None) -> Case:
    """A = 2^-2a (I + e_j e_j^T), b = 2^-a pair(r) e_j: x_j = 2^(a-1) pair(r)
    and every other element 0.  With ``reg = 0`` and ``t = 1`` (the long-row
    case) A = e_j e_j^T, whose zero pivots solve to 0: x_j = pair(r)."""
    r = fused_ratings(gather, a) if ratings is None else ratings
    t = 2.0 ** -a if t is None else t
    reg = 2.0 ** (-2 * a) if reg is None else reg
    n = r.numel()
    col = torch.arange(n) % k
    return _case(scaled_identity(k, t, gather), col, r, col, reg, lengths,
                 gather)


def fused_x(case: Case, factor: float) -> torch.Tensor:
    """Expected x [N][k] of a fused case: factor * pair(r) in column col
    (+ 0.0: b leaves an MFMA whose sum starts from +0, so a -0 pair arrives
    as +0)."""
    r = case.csr.values[case.last()]
    x = torch.zeros(case.n, case.table.shape[1])
    x[torch.arange(case.n), case.col] = \
        factor * R.rating_pair(r, case.gather) + 0.0
    return x


LONG_ROW_LENGTHS = (33, 65, 48, 64)


def long_row_case(k: int, gather: str) -> Case:
    """The fused rating-pair case on long rows: unit table row and reg = 0,
    so A = e_j e_j^T (its zero pivots solve to 0, like an empty row's) and
    x_j = pair(r).  The edge rating sits in the last slot: slot 32, 47 and 63
    of a 64-rating pair of chunks (lanes 32-63 of the split-wave EXT map of
    k_als_solve_wavefused) and slot 0 of the third chunk."""
    r = fused_ratings(gather, 1)
    lengths = torch.tensor(LONG_ROW_LENGTHS)[torch.arange(r.numel()) % 4]
    return fused_case(k, gather, 1, lengths=lengths, reg=0.0, t=1.0)


RATING_LENGTHS = (1, 33, 65, 6, 16, 27, 32, 64)


def rating_case(k: int, gather: str) -> Case:
    """Rating-pair encoders through the Gramian: unit rows, ratings from the
    gather dtype's edge set (specials included: only b[j] is read), with the
    edge rating in the last slot of rows of 1, 33 and 65 entries (slot 0 of
    the first chunk and of a one-entry tail chunk) and of 6, 16, 27, 32 and
    64 entries (slots 5, 15, 26 and 31: other lanes of the per-lane EXT
    conversion, other lanes and quad positions of the 8-lane one)."""
    edges = e4m3_edges() if gather == "fp8" else bf16_edges()
    r = torch.cat([edges, specials()])
    n = r.numel()
    col = torch.arange(n) % k
    # every rating at every length would multiply the work: the lengths
    # rotate over the ratings, with another phase at every rank
    lengths = torch.tensor(RATING_LENGTHS)[(torch.arange(n) + k // 16) % 8]
    return _case(scaled_identity(k, 1.0, gather), col, r, col, 0.25, lengths,
                 gather)


def byte_table(k: int) -> torch.Tensor:
    """uint8 [257][k]: row i holds byte i in column i mod k; row 256 zero."""
    tab = torch.zeros(257, k, dtype=torch.uint8)
    i = torch.arange(256)
    tab[i, i % k] = i.to(torch.uint8)
    return tab


DECODE_LENGTHS = (1, 5, 17, 32)


def decode_case(k: int, reg: float, lengths=DECODE_LENGTHS,
                scales=None) -> Case:
    """All 256 e4m3 bytes, one per entity, rating (ext) 1, once per row
    length (the byte's entry sits in slot length - 1 of its chunk).  With
    ``scales`` (a list): once per scale instead, rows of length 1."""
    i = torch.arange(256)
    if scales is None:
        rows = i.repeat(len(lengths))
        ln = torch.tensor(lengths).repeat_interleave(256)
        sc = None
    else:
        rows = i.repeat(len(scales))
        ln = 1
        sc = torch.tensor(scales, dtype=torch.float32).repeat_interleave(256)
    return _case(byte_table(k), rows, torch.ones(rows.numel()), rows % k, reg,
                 ln, "fp8", sc)


FP8_SCALES = (1.0, 0.75, 1.5, 3.0, 2.0 ** -7, 1.0 + 2.0 ** -20, 300.0, -1.0)
BF16_SCALES = (1.5, 1.0 + 2.0 ** -8, 3.0, 2.0 ** -10)


def bf16_scale_case(k: int) -> Case:
    """The bf16 twin of the scaled decode case: the 768 values of
    :func:`bf16_values` (every other pair negative) times BF16_SCALES; odd
    mantissas times 1.5 are exact ties, 2^-10 (= 2^-130 * 2^120) takes the
    exponent -126 / -127 rows into the subnormals."""
    pats = bf16_values().clone()
    idx = torch.arange(pats.numel())
    pats[(idx // 2) % 2 == 1] |= 0x8000
    m = pats.numel()
    tab = torch.zeros(m + 1, k, dtype=torch.int32)
    tab[idx, idx % k] = pats
    tab = torch.where(tab >= 0x8000, tab - 0x10000, tab).to(torch.int16)
    rows = idx.repeat(len(BF16_SCALES))
    sc = torch.tensor(BF16_SCALES).repeat_interleave(m)
    return _case(tab.view(torch.bfloat16), rows, torch.ones(rows.numel()),
                 rows % k, 0.25, 1, "bf16", sc)


def take(case: Case, idx: torch.Tensor) -> Case:
    """The case of the entities ``idx`` alone (same table)."""
    last = case.last()[idx]
    return _case(case.table, case.csr.indices[last], case.csr.values[last],
                 case.col[idx], case.reg, case.lengths[idx], case.gather,
                 None if case.scale is None else case.scale[last])


def own_entry(case: Case) -> torch.Tensor:
    """fp32 table element that entity i's own entry contributes."""
    rows = case.csr.indices[case.last()].long()
    return R._table_f32(case.table)[rows, case.col]


def widen_tables(k: int):
    """e4m3 tables for factor_gram, 5 rows each: byte v in column 2m, 1.0 in
    column 2m + 1 of row (m mod 5) for the k / 2 bytes of the batch, so that
    G[2m + 1][2m] = v and G[2m][2m] = v^2 stay separately readable.  Yields
    (first byte, table)."""
    per = k // 2
    one = int(ops.quantize_fp8(torch.tensor([1.0]))[0])
    for first in range(0, 256, per):
        tab = torch.zeros(5, k, dtype=torch.uint8)
        for m in range(min(per, 256 - first)):
            tab[m % 5, 2 * m] = first + m
            tab[m % 5, 2 * m + 1] = one
        yield first, tab
