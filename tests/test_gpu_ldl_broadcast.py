"""Lane-broadcast variants of the k<=64 register LDL must agree bit for bit.

The readlane variants only move data: every multiply, FMA and division
keeps its operands and order, so fp32 outputs and the bf16/e4m3 byte images
are compared with ``torch.equal`` against the retained shuffle variant, on
one small CSR whose row degrees sit on the 32-rating chunk and split-wave
pair boundaries.  The default variant is also held to the fp32 reference.
"""

import functools

import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.data.blocked import CSR, csr_from_coo
from flink_ms_amd.ops import reference as R

pytestmark = pytest.mark.gpu

ROWS, COLS = 67, 40            # 67 % 4 == 3: odd tail of the 4-wave block
EDGE_DEGREES = [0, 1, 31, 32, 33, 64, 65, 97]
SHFL, PANEL, SUBST, READLANE = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def _case():
    """(cpu CSR, degrees): the edge degrees first, small random ones after."""
    g = torch.Generator().manual_seed(20)
    deg = torch.randint(0, 41, (ROWS,), generator=g)
    deg[: len(EDGE_DEGREES)] = torch.tensor(EDGE_DEGREES)
    deg = deg[torch.randperm(ROWS, generator=g)]
    r_idx = torch.repeat_interleave(torch.arange(ROWS), deg)
    nnz = r_idx.numel()
    c_idx = torch.randint(0, COLS, (nnz,), generator=g)
    vals = torch.rand(nnz, generator=g) * 4.5 + 0.5
    csr = csr_from_coo(r_idx.int(), c_idx.int(), vals, ROWS, COLS)
    assert set(EDGE_DEGREES) <= set(csr.row_counts().tolist())
    return csr, deg


@functools.lru_cache(maxsize=None)
def _factors(k, dtype):
    """(kernel input, the same values as fp32) for one rank and dtype."""
    fac32 = torch.randn(COLS, k, generator=torch.Generator().manual_seed(k)
                        ) * 0.5
    if dtype == "fp8":
        q = ops.quantize_fp8(fac32)
        return q, ops.dequantize_fp8(q)
    q = fac32.to(torch.bfloat16)
    return q, q.to(torch.float32)


def _row_order(gpu):
    g = torch.Generator().manual_seed(5)
    return torch.randperm(ROWS, generator=g).to(torch.int32).to(gpu)


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


def _run_wavefused(csr, fac, reg, order, variant, gpu, db=False):
    import flink_ms_amd._hip_ops as hip
    out = _outputs(csr.num_rows, fac.shape[1], gpu)
    fn = hip.als_solve_wavefused_db if db else hip.als_solve_wavefused
    fn(csr.indptr, csr.indices, csr.values, fac, out[0], out[1], out[2],
       order, reg, torch.cuda.current_stream().cuda_stream, variant)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("k", [16, 32, 48, 64])
def test_wavefused_variants_bit_identical(gpu, dtype, k):
    csr_cpu, deg = _case()
    csr = csr_cpu.to(gpu)
    fac_cpu, fac32 = _factors(k, dtype)
    fac = fac_cpu.to(gpu)
    order = _row_order(gpu)
    base = _run_wavefused(csr, fac, 0.3, order, SHFL, gpu)
    for variant in (PANEL, SUBST, READLANE):
        got = _run_wavefused(csr, fac, 0.3, order, variant, gpu)
        _assert_same(got, base, f"variant {variant} vs shfl")
    new = _run_wavefused(csr, fac, 0.3, order, READLANE, gpu)
    assert torch.isfinite(new[0]).all()
    assert new[0].cpu()[deg == 0].abs().sum() == 0.0
    # the variant-less call runs the default
    import flink_ms_amd._hip_ops as hip
    assert hip.BROADCAST_DEFAULT == READLANE and hip.BROADCAST_SHFL == SHFL
    dflt = ops.als_solve_side(csr, fac, reg=0.3, row_order=order)
    torch.cuda.synchronize()
    assert torch.equal(dflt.view(torch.int32), new[0].view(torch.int32))

    # the new path against fp32 ground truth on identically quantized inputs
    vals = csr_cpu.values
    if dtype == "fp8":
        ref_vals = ops.fp8_rating_pair(vals)
    else:
        hi = vals.to(torch.bfloat16).to(torch.float32)
        ref_vals = hi + (vals - hi).to(torch.bfloat16).to(torch.float32)
    ref_csr = CSR(csr_cpu.indptr, csr_cpu.indices, ref_vals, ROWS, COLS)
    ref = R.als_solve_side_reference(ref_csr, fac32, reg=0.3)
    err = float((new[0].cpu() - ref).abs().amax())
    bound = 5e-3 * float(ref.abs().amax())
    print(f"k={k} {dtype}: max|err|={err:.3e} bound={bound:.3e}")
    assert err < bound, (k, dtype, err, bound)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("k", [16, 32, 48, 64])
def test_ldl_solve_wave_reg_variants_bit_identical(gpu, dtype, k):
    import flink_ms_amd._hip_ops as hip
    csr_cpu, _ = _case()
    csr = csr_cpu.to(gpu)
    fac = _factors(k, dtype)[0].to(gpu)
    # drop the empty rows: their A is all zero, not a system to solve
    A, b = ops.gramian(csr, fac, reg=0.3)
    keep = (csr.row_counts() > 0).nonzero(as_tuple=True)[0]
    A, b = A[keep].contiguous(), b[keep].contiguous()
    st = torch.cuda.current_stream().cuda_stream
    outs = {}
    for variant in (SHFL, READLANE):
        o = _outputs(A.shape[0], k, gpu)
        hip.ldl_solve_wave_reg(A, b, o[0], o[1], o[2], st, variant)
        outs[variant] = o
    torch.cuda.synchronize()
    _assert_same(outs[READLANE], outs[SHFL], "ldl_solve_wave_reg")
    assert torch.isfinite(outs[READLANE][0]).all()


def test_wavefused_db_variants_bit_identical(gpu):
    csr = _case()[0].to(gpu)
    fac = _factors(64, "fp8")[0].to(gpu)
    order = _row_order(gpu)
    base = _run_wavefused(csr, fac, 0.3, order, SHFL, gpu, db=True)
    new = _run_wavefused(csr, fac, 0.3, order, READLANE, gpu, db=True)
    _assert_same(new, base, "wavefused_db")
    assert torch.isfinite(new[0]).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_degenerate_pivots_bit_identical(gpu, dtype):
    """reg = 0 and every rating of an entity on ONE column: A is rank 1, so
    the pivots after the first are rounding residue or <= 0 and take the
    ``dj > 0 ? 1/dj : 0`` guard."""
    g = torch.Generator().manual_seed(77)
    deg = torch.tensor([40, 5, 0, 33, 1])
    r_idx = torch.repeat_interleave(torch.arange(deg.numel()), deg)
    c_idx = torch.randint(0, COLS, (r_idx.numel(),), generator=g)
    c_idx[r_idx == 0] = 7          # 40 ratings, one column, two chunks
    c_idx[r_idx == 3] = 11         # 33 ratings: one past a chunk
    vals = torch.rand(r_idx.numel(), generator=g) * 4.5 + 0.5
    csr = csr_from_coo(r_idx.int(), c_idx.int(), vals, deg.numel(), COLS
                       ).to(gpu)
    fac = _factors(64, dtype)[0].to(gpu)
    empty = torch.empty(0, device=gpu)
    base = _run_wavefused(csr, fac, 0.0, empty, SHFL, gpu)
    for variant in (PANEL, SUBST, READLANE):
        got = _run_wavefused(csr, fac, 0.0, empty, variant, gpu)
        _assert_same(got, base, f"degenerate, variant {variant}")
        assert torch.isfinite(got[0]).all()
