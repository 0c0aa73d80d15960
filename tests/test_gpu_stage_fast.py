"""The Gramian staging only moves bytes: hold it to that, bit for bit.

Round 6 rebuilt ``stage_chunk_w`` (byte-permute transpose, one rating per
lane for the EXT rows, wide unguarded loads on full trips, 16-byte pad-row
zeroing).  None of that is arithmetic on the result, so

* the staged LDS image of one chunk is compared byte for byte with an image
  built in torch, for both gather precisions (``dbg_stage_dump_fp8`` /
  ``dbg_stage_dump``; the dump starts from a 0xA5-filled buffer, so an
  element the staging never writes shows up);
* ``als_solve_wavefused`` is compared, as bit patterns, with
  ``als_solve_wavefused_db``, which keeps the previous transpose and 8-lane
  rating conversion in its own ``stage_loads`` / ``stage_commit`` and
  accumulates the chunks in the same order (the two kernels are bit-equal
  on the parent commit as well);
* entities that end exactly where the CSR arrays end still solve to the
  fp32 reference: the wide loads of a full trip must not be taken on a tail.

The e4m3 EXT bytes follow the kernels' ``f2fp8``, which is the contract of
``ops.quantize_fp8``: round to nearest even, finite values beyond +-448
saturate (the host clamps before its cast), inf / NaN give NaN.  The pair
is ``ops.fp8_rating_pair``, which the test also checks.
"""

import functools

import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.data.blocked import CSR, csr_from_coo
from flink_ms_amd.ops import reference as R

pytestmark = pytest.mark.gpu

RANKS = [16, 32, 48, 64]
CHUNK_FILLS = [1, 2, 3, 4, 5, 8, 9, 31, 32]
TABLE_ROWS = 256
# 0, negatives, non-zero low halves, beyond the e4m3 range, one inf
SPECIAL_RATINGS = [0.0, -1.5, 3.14159, 500.0, float("inf"), 0.3, -449.0, 4.5,
                   447.9, 1e-3, -2.7, 1000.0, -0.0]
READLANE = 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _ratings32():
    g = torch.Generator().manual_seed(6)
    r = torch.rand(32, generator=g) * 4.5 + 0.5
    r[: len(SPECIAL_RATINGS)] = torch.tensor(SPECIAL_RATINGS)
    return r


def _chunk(n):
    """(indices, ratings) of one n-rating chunk: distinct table rows, the
    special ratings on different lanes for different n."""
    g = torch.Generator().manual_seed(100 + n)
    idx = torch.randperm(TABLE_ROWS, generator=g)[:n].to(torch.int32)
    return idx, torch.roll(_ratings32(), n)[:n].contiguous()


def _fp8_pair_bytes(r):
    hi = ops.quantize_fp8(r)
    lo = ops.quantize_fp8(r - ops.dequantize_fp8(hi))
    return hi, lo


def _bf16_pair_bits(r):
    hi = r.to(torch.bfloat16)
    lo = (r - hi.to(torch.float32)).to(torch.bfloat16)
    return hi.view(torch.int16), lo.view(torch.int16)


def _canon_ext_nans(img, k):
    """The image with every NaN element of the EXT rows k, k+1 replaced by
    one canonical NaN.  The inf rating makes them (e4m3 has no inf, and
    ``inf - hi`` is NaN in both precisions), and neither the sign nor the
    payload of a NaN that a subtraction or a cast produces is pinned by
    IEEE 754: they follow where a compiler puts a negation and how a cast is
    implemented, in the kernel as in the torch expression.  That the element
    IS a NaN is still compared; the factor rows are untouched."""
    img = img.clone()
    ext = img[k:k + 2]
    if img.dtype == torch.uint8:
        ext[(ext & 0x7F) == 0x7F] = 0x7F
    else:
        ext[(ext.to(torch.int32) & 0x7FFF) > 0x7F80] = 0x7FC0
    return img


def _expected_image(F, idx, hi, lo, k):
    """Gt[c][r] = F[idx[r]][c] for r < n; rows k, k+1 = hi, lo; rest 0."""
    n = idx.numel()
    img = torch.zeros(k + 16, 32, dtype=F.dtype, device=F.device)
    img[:k, :n] = F[idx.long()].t()
    img[k, :n] = hi
    img[k + 1, :n] = lo
    return img


@pytest.mark.parametrize("k", RANKS)
def test_stage_image_fp8(gpu, k):
    import flink_ms_amd._hip_ops as hip
    # every byte value in every column (7 is a unit mod 256)
    F = ((7 * torch.arange(TABLE_ROWS)[:, None] + 13 * torch.arange(k)[None])
         % 256).to(torch.uint8).to(gpu)
    assert all(F[:, c].unique().numel() == 256 for c in (0, k - 1))
    for n in CHUNK_FILLS:
        idx, r = _chunk(n)
        idx, r = idx.to(gpu), r.to(gpu)
        hi, lo = _fp8_pair_bytes(r)
        inside = torch.isfinite(r)         # the inf rating's pair is NaN
        assert torch.equal(
            (ops.dequantize_fp8(hi) + ops.dequantize_fp8(lo))[inside],
            ops.fp8_rating_pair(r)[inside])
        want = _expected_image(F, idx, hi, lo, k)
        got = torch.full(((k + 16) * 32,), 0x5A, dtype=torch.uint8,
                         device=gpu)
        hip.dbg_stage_dump_fp8(
            torch.tensor([0, n], dtype=torch.int64, device=gpu), idx, r, F,
            got, _stream())
        torch.cuda.synchronize()
        got = got.view(k + 16, 32)
        raw = (got != want).nonzero()
        print(f"fp8 k={k} n={n}: {raw.shape[0]} differing bytes before the "
              f"EXT NaNs are canonicalised",
              [(r, c, int(got[r, c]), int(want[r, c]))
               for r, c in raw[:4].tolist()])
        got, want = _canon_ext_nans(got, k), _canon_ext_nans(want, k)
        bad = (got != want).nonzero()
        assert torch.equal(got, want), (k, n, bad[:8].tolist())


@pytest.mark.parametrize("k", RANKS)
def test_stage_image_bf16(gpu, k):
    import flink_ms_amd._hip_ops as hip
    # arbitrary 16-bit patterns (NaN ones included): they are only moved
    bits = (251 * torch.arange(TABLE_ROWS)[:, None]
            + 4099 * torch.arange(k)[None] + 0x1234) & 0xFFFF
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16)
    F = bits.to(gpu)
    for n in CHUNK_FILLS:
        idx, r = _chunk(n)
        idx, r = idx.to(gpu), r.to(gpu)
        hi, lo = _bf16_pair_bits(r)
        want = _expected_image(F, idx, hi, lo, k)
        got = torch.full(((k + 16) * 32,), 1.0, dtype=torch.bfloat16,
                         device=gpu)
        hip.dbg_stage_dump(
            torch.tensor([0, n], dtype=torch.int64, device=gpu), idx, r,
            F.view(torch.bfloat16), got, _stream())
        torch.cuda.synchronize()
        got = got.view(torch.int16).view(k + 16, 32)
        raw = (got != want).nonzero()
        print(f"bf16 k={k} n={n}: {raw.shape[0]} differing words before the "
              f"EXT NaNs are canonicalised",
              [(r, c, int(got[r, c]), int(want[r, c]))
               for r, c in raw[:4].tolist()])
        got, want = _canon_ext_nans(got, k), _canon_ext_nans(want, k)
        bad = (got != want).nonzero()
        assert torch.equal(got, want), (k, n, bad[:8].tolist())


# ------------------------------------------------- whole kernel vs old staging

ROW_LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129,
               160, 257]
COLS = 40


def _csr_of(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    deg = torch.tensor(lengths)
    r_idx = torch.repeat_interleave(torch.arange(deg.numel()), deg)
    nnz = r_idx.numel()
    c_idx = torch.randint(0, COLS, (nnz,), generator=g)
    vals = torch.rand(nnz, generator=g) * 4.5 + 0.5
    return csr_from_coo(r_idx.int(), c_idx.int(), vals, deg.numel(), COLS)


@functools.lru_cache(maxsize=None)
def _edge_csr():
    csr = _csr_of(ROW_LENGTHS, 61)
    assert csr.row_counts().tolist() == ROW_LENGTHS
    return csr


@functools.lru_cache(maxsize=None)
def _fp8_factors(k):
    fac32 = torch.randn(COLS, k, generator=torch.Generator().manual_seed(k)
                        ) * 0.5
    q = ops.quantize_fp8(fac32)
    return q, ops.dequantize_fp8(q)


def _outputs(rows, k, gpu):
    return (torch.full((rows, k), float("nan"), device=gpu),
            torch.full((rows, k), float("nan"), device=gpu,
                       dtype=torch.bfloat16),
            torch.full((rows, k), 0x7F, device=gpu, dtype=torch.uint8))


def _assert_same(a, b, what):
    f32a, bfa, f8a = a
    f32b, bfb, f8b = b
    # bit patterns, so that -0.0 / NaN payloads count as differences too
    assert torch.equal(f32a.view(torch.int32), f32b.view(torch.int32)), what
    assert torch.equal(bfa.view(torch.int16), bfb.view(torch.int16)), what
    assert torch.equal(f8a, f8b), what


def _run(fn, csr, fac, reg, order, gpu):
    out = _outputs(csr.num_rows, fac.shape[1], gpu)
    fn(csr.indptr, csr.indices, csr.values, fac, out[0], out[1], out[2],
       order, reg, _stream(), READLANE)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("k", RANKS)
def test_wavefused_equals_old_staging(gpu, k, shuffled):
    import flink_ms_amd._hip_ops as hip
    csr = _edge_csr().to(gpu)
    fac = _fp8_factors(k)[0].to(gpu)
    if shuffled:
        g = torch.Generator().manual_seed(5)
        order = torch.randperm(len(ROW_LENGTHS), generator=g
                               ).to(torch.int32).to(gpu)
    else:
        order = torch.empty(0, device=gpu)
    new = _run(hip.als_solve_wavefused, csr, fac, 0.3, order, gpu)
    old = _run(hip.als_solve_wavefused_db, csr, fac, 0.3, order, gpu)
    _assert_same(new, old, f"k={k} shuffled={shuffled}")
    assert torch.isfinite(new[0]).all()
    assert new[0][0].abs().sum() == 0.0            # the empty row


# ----------------------------------------------------------------- tail safety

@pytest.mark.parametrize("last", [1, 33, 65])
@pytest.mark.parametrize("k", RANKS)
def test_last_entity_ends_with_the_arrays(gpu, k, last):
    """indices / values are exact-size tensors and the last entity's range
    is their end; its solution is held to the fp32 reference on identically
    quantized inputs (bound of test_wavefused_variants_bit_identical)."""
    csr_cpu = _csr_of([64, 3, last], 70 + last)
    assert csr_cpu.indices.numel() == 67 + last == int(csr_cpu.indptr[-1])
    csr = CSR(csr_cpu.indptr.to(gpu), csr_cpu.indices.to(gpu).clone(),
              csr_cpu.values.to(gpu).clone(), csr_cpu.num_rows, COLS)
    fac_cpu, fac32 = _fp8_factors(k)
    got = ops.als_solve_side(csr, fac_cpu.to(gpu), reg=0.3)
    torch.cuda.synchronize()
    ref_csr = CSR(csr_cpu.indptr, csr_cpu.indices,
                  ops.fp8_rating_pair(csr_cpu.values), csr_cpu.num_rows, COLS)
    ref = R.als_solve_side_reference(ref_csr, fac32, reg=0.3)
    err = float((got.cpu()[-1] - ref[-1]).abs().amax())
    bound = 5e-3 * float(ref.abs().amax())
    print(f"k={k} last={last}: max|err|={err:.3e} bound={bound:.3e}")
    assert err < bound, (k, last, err, bound)
