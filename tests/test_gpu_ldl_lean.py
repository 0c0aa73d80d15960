"""The leaner register LDL (variant 3) against the shuffle path (variant 0),
bit for bit, on the inputs its shortcuts could get wrong.

Variant 3 packs pairs of panel updates, selects substitution results under
literal lane masks and shares one reciprocal per pivot between the
substitutions and the trailing update.  None of that may move a bit, so the
inputs here are the ones where a changed operand, a changed lane set or a
changed division would show: non-positive, denormal, huge and
inexact-reciprocal pivots on the 16-column panel edges, pivots that only
become non-positive during the elimination, rank-deficient rows without
regularisation, and ratings that are inf, nan or -0.0.
"""

import functools

import pytest
import torch

from flink_ms_amd.data.blocked import csr_from_coo

pytestmark = pytest.mark.gpu

SHFL, READLANE = 0, 3
ROWS, COLS = 67, 40            # 67 % 4 == 3: odd tail of the 4-wave block
EDGE_DEGREES = [0, 1, 31, 32, 33, 64, 65, 97]
PANEL_EDGES = [0, 15, 16, 31, 47]          # plus k - 1
PIVOTS = [0.0, -1.0, 1e-40, 1e-38, 1e38, 3.0]


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


def _edges(k):
    return sorted({p for p in PANEL_EDGES + [k - 1] if p < k})


def _spd(k, g):
    m = torch.randn(k, k + 8, generator=g) * 0.5
    return m @ m.T + 0.5 * torch.eye(k)


def _plant(a, pos, val):
    """Make ``val`` the exact pivot at ``pos``: with the row and column
    zeroed, every update of that diagonal entry subtracts 0 * x."""
    a[pos, :] = 0.0
    a[:, pos] = 0.0
    a[pos, pos] = val


@functools.lru_cache(maxsize=None)
def _systems(k):
    """(A [n, k, k], b [n, k]) on the CPU, hand-built."""
    g = torch.Generator().manual_seed(400 + k)
    edges = _edges(k)
    mats = []
    for val in PIVOTS:                     # one value on every panel edge
        a = _spd(k, g)
        for p in edges:
            _plant(a, p, val)
        mats.append(a)
    a = _spd(k, g)                         # all the values in one system
    for n, p in enumerate(edges):
        _plant(a, p, PIVOTS[n % len(PIVOTS)])
    mats.append(a)
    # pivots that turn non-positive during the elimination: off-diagonal 2
    # under a unit diagonal gives 1 - 4 = -3 from the second pivot on
    mats.append(torch.full((k, k), 2.0) - torch.eye(k))
    # rank 3, no regularisation: pivots past the third are rounding residue
    low = torch.randn(k, 3, generator=g)
    mats.append(low @ low.T)
    A = torch.stack(mats).contiguous()
    b = torch.randn(A.shape[0], k, generator=g)
    return A, b


SYSTEMS = [f"pivot={v}" for v in PIVOTS] + ["mixed", "offdiag2", "rank3"]


@functools.lru_cache(maxsize=None)
def _solved(k, gpu):
    """Both variants' outputs for all of ``_systems(k)``: one launch each."""
    import flink_ms_amd._hip_ops as hip
    A_cpu, b_cpu = _systems(k)
    A, b = A_cpu.to(gpu), b_cpu.to(gpu)
    st = torch.cuda.current_stream().cuda_stream
    outs = {}
    for variant in (SHFL, READLANE):
        o = _outputs(A.shape[0], k, gpu)
        hip.ldl_solve_wave_reg(A, b, o[0], o[1], o[2], st, variant)
        outs[variant] = o
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("system", SYSTEMS)
@pytest.mark.parametrize("k", [16, 32, 48, 64])
def test_ldl_solve_wave_reg_special_pivots(gpu, k, system):
    """One system per case, one launch per variant and k.  A 1e-40 pivot
    overflows its reciprocal and turns the whole system into NaNs; before
    the kernels stored a canonical NaN those differed between the variants
    in the sign bit (0xffc00000 against 0x7fc00000, in 4 / 33 / 51 / 69 of
    the 9*k outputs at k = 16 / 32 / 48 / 64), so these systems are the
    check on that store as well."""
    assert len(SYSTEMS) == _systems(k)[0].shape[0]
    outs = _solved(k, gpu)
    s = SYSTEMS.index(system)
    pick = lambda o: tuple(t[s] for t in o)
    _assert_same(pick(outs[READLANE]), pick(outs[SHFL]),
                 f"ldl_solve_wave_reg k={k} {system}")
    if system in ("pivot=3.0", "offdiag2"):
        assert torch.isfinite(outs[SHFL][0][s]).all()


@functools.lru_cache(maxsize=None)
def _case():
    """A CSR with the edge degrees, rank-deficient rows (degree 1, one
    column repeated) and a few non-finite / negative-zero ratings."""
    g = torch.Generator().manual_seed(21)
    deg = torch.randint(2, 41, (ROWS,), generator=g)
    deg[: len(EDGE_DEGREES)] = torch.tensor(EDGE_DEGREES)
    deg = deg[torch.randperm(ROWS, generator=g)]
    r_idx = torch.repeat_interleave(torch.arange(ROWS), deg)
    nnz = r_idx.numel()
    c_idx = torch.randint(0, COLS, (nnz,), generator=g)
    vals = torch.rand(nnz, generator=g) * 4.5 + 0.5
    rows = lambda d: (deg == d).nonzero(as_tuple=True)[0].tolist()
    # duplicate column ids: the 33- and 65-rating rows hit one column only,
    # the 97-rating row alternates between two
    c_idx[r_idx == rows(33)[0]] = 7
    c_idx[r_idx == rows(65)[0]] = 11
    sel = (r_idx == rows(97)[0]).nonzero(as_tuple=True)[0]
    c_idx[sel] = torch.tensor([3, 5]).repeat(49)[: sel.numel()]
    # non-finite and negative-zero ratings in rows of ordinary degree
    plain = [r for r in range(ROWS) if int(deg[r]) not in EDGE_DEGREES]
    for r, v in zip(plain, [float("inf"), float("nan"), -0.0, -0.0,
                            float("-inf")]):
        first = int((r_idx == r).nonzero(as_tuple=True)[0][0])
        vals[first] = v
    csr = csr_from_coo(r_idx.int(), c_idx.int(), vals, ROWS, COLS)
    assert set(EDGE_DEGREES) <= set(csr.row_counts().tolist())
    return csr, deg


@functools.lru_cache(maxsize=None)
def _factors(k, dtype):
    from flink_ms_amd import ops
    fac32 = torch.randn(COLS, k, generator=torch.Generator().manual_seed(k)
                        ) * 0.5
    if dtype == "fp8":
        return ops.quantize_fp8(fac32)
    return fac32.to(torch.bfloat16)


def _row_order(gpu):
    g = torch.Generator().manual_seed(6)
    return torch.randperm(ROWS, generator=g).to(torch.int32).to(gpu)


def _run_wavefused(csr, fac, reg, order, variant, gpu, db=False):
    import flink_ms_amd._hip_ops as hip
    out = _outputs(csr.num_rows, fac.shape[1], gpu)
    fn = hip.als_solve_wavefused_db if db else hip.als_solve_wavefused
    fn(csr.indptr, csr.indices, csr.values, fac, out[0], out[1], out[2],
       order, reg, torch.cuda.current_stream().cuda_stream, variant)
    torch.cuda.synchronize()
    return out


def _check_wavefused(gpu, dtype, k, db):
    csr_cpu, deg = _case()
    csr = csr_cpu.to(gpu)
    fac = _factors(k, dtype).to(gpu)
    order = _row_order(gpu)
    base = _run_wavefused(csr, fac, 0.0, order, SHFL, gpu, db=db)
    new = _run_wavefused(csr, fac, 0.0, order, READLANE, gpu, db=db)
    _assert_same(new, base, f"wavefused k={k} {dtype} db={db}")
    x = base[0].cpu()
    assert x[deg == 0].abs().sum() == 0.0
    fin = torch.isfinite(x).all(dim=1)
    print(f"k={k} {dtype} db={db}: {int(fin.sum())}/{ROWS} rows finite")


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("k", [48, 64])
def test_wavefused_rank_deficient_nonfinite(gpu, dtype, k):
    _check_wavefused(gpu, dtype, k, db=False)


def test_wavefused_db_rank_deficient_nonfinite(gpu):
    _check_wavefused(gpu, "fp8", 64, db=True)
