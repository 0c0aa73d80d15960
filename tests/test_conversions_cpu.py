"""CPU twin of tests/test_gpu_conversions.py: the edge sets, the host casts
against independent oracles, the saturating e4m3 contract on the host, and
the exactness claims of every fixture the GPU file feeds the kernels (each
system is formed by ``reference`` in fp32 and in float64 and must come out at
the stated values, bit for bit)."""

import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.data.blocked import CSR
from flink_ms_amd.ops import reference as R

import _conversion_fixture as cf


def _eq(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (what, bad.shape[0], bad[:6].tolist())


# --------------------------------------------------------------- edge sets

def test_e4m3_edge_set():
    e = cf.e4m3_edges()
    assert e.numel() == 1022 and e.dtype == torch.float32
    tab = cf.e4m3_table()
    assert tab.numel() == 127 and float(tab[0]) == 0.0
    assert float(tab[1]) == 2.0 ** -9 and float(tab[8]) == 2.0 ** -6
    # the table is what a decode of bytes 0..126 gives
    _eq(ops.dequantize_fp8(torch.arange(127, dtype=torch.uint8)).double(),
        tab, "table vs dequantize")
    mid = cf.e4m3_midpoints()
    assert mid.numel() == 126
    for v in (0.0, -0.0, 448.0, -448.0, 464.0, 465.0, 2.0 ** -10):
        assert bool((e == v).any()), v
    assert bool((e.view(torch.int32) == -2 ** 31).any())        # -0 itself
    assert bool(cf.is_e4m3_tie(e).sum() == 2 * 127)
    assert bool(cf.is_e4m3_subnormal(e).any())
    assert bool(cf.is_e4m3_saturated(e).any())
    assert bool(cf.is_e4m3_negzero(e).any())


def test_e4m3_encode_matches_oracle():
    x = torch.cat([cf.e4m3_edges(), cf.specials()])
    want = cf.e4m3_oracle(x)
    _eq(cf.canon_nan(ops.quantize_fp8(x)), cf.canon_nan(want), "quantize_fp8")
    # ties go to the even byte, both ways
    m = cf.e4m3_midpoints()
    _eq(ops.quantize_fp8(m) % 2, torch.zeros(126, dtype=torch.uint8), "ties")
    assert int(ops.quantize_fp8(torch.tensor([464.0]))) == 0x7E
    # a plain cast differs from the contract exactly beyond 464
    e = cf.e4m3_edges()
    plain = e.to(torch.float8_e4m3fn).view(torch.uint8)
    differs = cf.canon_nan(plain) != cf.canon_nan(cf.e4m3_oracle(e))
    beyond = torch.tensor(cf.BEYOND_E4M3)
    _eq(e[differs].sort().values, torch.cat([-beyond, beyond]).sort().values,
        "where the unclamped cast differs")
    # the oracle on a dense sweep through the body of the range as well
    g = torch.Generator().manual_seed(1)
    y = torch.randn(20000, generator=g) * torch.logspace(-4, 3, 20000)
    _eq(ops.quantize_fp8(y), cf.e4m3_oracle(y), "sweep")


def test_e4m3_decode_matches_oracle():
    b = torch.arange(256, dtype=torch.uint8)
    _eq(cf.canon_nan(ops.dequantize_fp8(b)),
        cf.canon_nan(cf.e4m3_decode_oracle(b)), "dequantize_fp8")
    fin = (b & 0x7F) != 0x7F
    _eq(ops.quantize_fp8(ops.dequantize_fp8(b))[fin], b[fin], "round trip")


def test_bf16_encode_matches_oracle():
    e = cf.bf16_edges()
    assert e.numel() == 2 * 4 * 768 + 2
    x = torch.cat([e, cf.specials()])
    _eq(cf.canon_nan(x.to(torch.bfloat16)), cf.canon_nan(cf.bf16_oracle(x)),
        "bf16 cast")
    assert bool(torch.isinf(e.to(torch.bfloat16).float()).any())  # overflow
    # every midpoint is a tie: the result has an even pattern
    p = cf.bf16_values() << 16
    mids = (p + 0x8000).view(torch.float32)
    assert bool((cf.bf16_oracle(mids) % 2 == 0).all())


# ------------------------------------------------- the contract on the host

def test_host_saturates_like_the_kernels():
    x = torch.tensor([465.0, -465.0, 1e4, -3.4e38, 448.0, 464.0, cf.INF,
                      -cf.INF, cf.NAN])
    q = ops.quantize_fp8(x)
    assert q[:6].tolist() == [0x7E, 0xFE, 0x7E, 0xFE, 0x7E, 0x7E]
    assert bool(((q[6:] & 0x7F) == 0x7F).all())
    # bf16 inputs too (-3.4e38 itself is -inf in bf16)
    assert ops.quantize_fp8(torch.tensor([465.0, -1e4, 3e38]).to(
        torch.bfloat16)).tolist() == [0x7E, 0xFE, 0x7E]
    _eq(R._round_gather(x[:6], "fp8"),
        torch.tensor([448.0, -448, 448, -448, 448, 448]), "_round_gather")
    r = torch.tensor([500.0, -1000.0, 3.4e38, 449.0])
    _eq(ops.fp8_rating_pair(r), torch.tensor([500.0, -896.0, 896.0, 449.0]),
        "fp8_rating_pair")
    assert bool(torch.isnan(ops.fp8_rating_pair(torch.tensor([cf.INF]))).all())
    # inside the range nothing changed
    e = cf.e4m3_edges()
    e = e[e.abs() <= 464.0]
    hi = e.to(torch.float8_e4m3fn).float()
    _eq(ops.fp8_rating_pair(e), hi + (e - hi).to(torch.float8_e4m3fn).float(),
        "pair inside the range")


def test_cpu_fallback_images_saturate():
    # one entity, one entry: x = 1000 * r / (1 + reg), far beyond the range
    tab = torch.zeros(2, 16)
    tab[0, 0] = 1.0
    csr = CSR(torch.tensor([0, 1]), torch.tensor([0], dtype=torch.int32),
              torch.tensor([2000.0]), 1, 2)
    o8 = torch.zeros(1, 16, dtype=torch.uint8)
    x = ops.als_solve_side(csr, ops.quantize_fp8(tab), 1.0, out_fp8=o8)
    assert float(x[0, 0]) > 448.0 and int(o8[0, 0]) == 0x7E
    o8.zero_()
    out = torch.zeros(1, 16)
    ops.als_solve_chunk(csr, ops.quantize_fp8(tab), 1.0, out, o8, None,
                        torch.tensor([0]))
    assert int(o8[0, 0]) == 0x7E
    # weighted: ext = (1 + w) / sqrt(w) beyond 448 for w < 5e-6
    s, e = ops.implicit_weights(torch.tensor([1.0]), 1e-6)
    assert float(e) > 448.0
    assert bool(torch.isfinite(ops.fp8_rating_pair(e)).all())
    A, b = R.gramian_weighted_reference(csr, ops.quantize_fp8(tab), 0.1,
                                        torch.ones(1), e, torch.zeros(16, 16))
    assert bool(torch.isfinite(b).all()) and float(b[0, 0]) == \
        float(ops.fp8_rating_pair(e))


# -------------------------------------------------- the fixtures' own claims

def _systems(case, dtype):
    """(A, b) of a case under the kernels' contract, by ``reference``."""
    scale = case.scale if case.scale is not None else torch.ones(case.csr.nnz)
    k = case.table.shape[1]
    A, b, _ = R._weighted_systems(case.csr, case.table, case.reg, scale,
                                  case.csr.values, torch.zeros(k, k), "auto",
                                  dtype)
    return A, b


def _diag_solve(A, b, rows=None):
    if rows is not None:         # entities with a NaN entry are left out
        A, b = A[rows], b[rows]
    d = A.diagonal(dim1=1, dim2=2)
    off = A - torch.diag_embed(d)
    assert not bool(off.any()), "A is not diagonal"
    return torch.where(d > 0, b / torch.where(d > 0, d, torch.ones_like(d)),
                       torch.zeros_like(b))


def _classes_present(x, what, gather):
    """The classes test_gpu_conversions asserts on the kernels' x.  With
    e4m3 gathers no x has a -0 e4m3 image: the expected x holds no -0 itself
    (fused_x) and a sum of two e4m3 values is never a non-zero below 2^-9."""
    classes = [("tie", cf.is_e4m3_tie), ("subnormal", cf.is_e4m3_subnormal),
               ("saturated", cf.is_e4m3_saturated)]
    negzero = bool(cf.is_e4m3_negzero(x.contiguous()).any())
    assert negzero == (gather == "bf16"), (what, "-0 image")
    for name, fn in classes:
        assert bool(fn(x.contiguous()).any()), (what, name)


@pytest.mark.parametrize("k, gather", [(16, "bf16"), (16, "fp8"),
                                       (112, "bf16")])
def test_fused_cases_are_exact(k, gather):
    owns = {}
    for a in (1, 4):
        case = cf.fused_case(k, gather, a)
        want = cf.fused_x(case, 2.0 ** (a - 1))
        assert bool(torch.isfinite(want).all())
        for dtype in (torch.float32, torch.float64):
            x = _diag_solve(*_systems(case, dtype))
            _eq(x, want.to(dtype), f"fused {gather} a={a} {dtype}")
        owns[a] = want[torch.arange(case.n), case.col]
        r = case.csr.values[case.last()]
        body = r.abs() * 2.0 ** (a - 1) <= 1e4
        if gather == "bf16":
            # the bf16 pair holds every edge up to 1e4 (3.4e38 rounds to inf
            # in bf16 and is left out at a = 1), so x walks the whole set,
            # the +-1-ulp neighbours of every tie included
            assert case.n == (1020 if a == 1 else 1022)
            _eq(owns[a][body], (r * 2.0 ** (a - 1))[body], "bf16 pair exact")
            assert int(body.sum()) == 1020
        else:
            assert case.n == 1022
    # what the kernels' x holds, both launches together
    _classes_present(torch.cat([owns[1], owns[4]]), f"fused {gather}",
                     gather)
    assert bool((owns[4].abs() > 448).any())
    if gather == "fp8":
        # the e4m3 pair reaches every representable value and every tie
        # whose half step is representable (ties >= 2^-5), not the ties'
        # fp32 neighbours
        own = set(owns[1].tolist())
        for v in cf.e4m3_table().float().tolist():
            assert v in own and -v in own
        ties = cf.e4m3_midpoints()
        reach = ties[ties >= 2.0 ** -5]
        assert reach.numel() == 110 and set(reach.tolist()) <= own
        assert not set(ties[ties < 2.0 ** -5].tolist()) & own


@pytest.mark.parametrize("gather", ["bf16", "fp8"])
def test_long_row_fused_case_is_exact(gather):
    case = cf.long_row_case(16, gather)
    assert sorted(set(case.lengths.tolist())) == [33, 48, 64, 65]
    want = cf.fused_x(case, 1.0)
    for dtype in (torch.float32, torch.float64):
        A, b = _systems(case, dtype)
        _eq(_diag_solve(A, b), want.to(dtype), f"long rows {gather} {dtype}")
        d = A.diagonal(dim1=1, dim2=2)
        assert float(d.sum()) == case.n          # e_j e_j^T and nothing else


@pytest.mark.parametrize("k, gather", [(16, "bf16"), (16, "fp8"),
                                       (112, "bf16")])
def test_rating_case_is_exact(k, gather):
    case = cf.rating_case(k, gather)
    assert sorted(set(case.lengths.tolist())) == sorted(cf.RATING_LENGTHS)
    if k == 112:
        # every 5th entity (5 and the 8 lengths are coprime): the whole
        # batch's A in float64 would take 600 MB
        case = cf.take(case, torch.arange(0, case.n, 5))
        assert sorted(set(case.col.tolist())) == list(range(112))
    r = case.csr.values[case.last()]
    pair = R.rating_pair(r, gather)
    # the pair from the independent oracles, not from the host casts
    indep = cf.oracle_pair(r, gather)
    _eq(cf.canon_nan(pair), cf.canon_nan(indep), "pair vs oracles")
    assert sorted(set(case.lengths.tolist())) == sorted(cf.RATING_LENGTHS)
    i = torch.arange(case.n)
    for dtype in (torch.float32, torch.float64):
        A, b = _systems(case, dtype)
        # + 0.0: the sum starts from +0, so a -0 pair arrives as +0
        _eq(cf.canon_nan(b[i, case.col].float()), cf.canon_nan(pair + 0.0),
            f"b {dtype}")
        _eq(A[i, case.col, case.col],
            (1 + 0.25 * case.lengths).to(dtype), f"A {dtype}")


@pytest.mark.parametrize("k", [16, 64])
def test_decode_case_is_exact(k):
    case = cf.decode_case(k, 0.25)
    v = cf.e4m3_decode_oracle(case.csr.indices[case.last()].to(torch.uint8))
    _eq(cf.canon_nan(cf.own_entry(case)), cf.canon_nan(v), "own entry")
    fin = torch.isfinite(v)
    assert int(fin.sum()) == 254 * len(cf.DECODE_LENGTHS)
    i = torch.arange(case.n)
    A64, b64 = _systems(case, torch.float64)
    A32, b32 = _systems(case, torch.float32)
    want_A = v.double() ** 2 + 0.25 * case.lengths
    _eq(b32[i, case.col][fin], v[fin], "b fp32")
    _eq(b64[i, case.col][fin], v[fin].double(), "b float64")
    _eq(A64[i, case.col, case.col][fin], want_A[fin], "A float64")
    _eq(A32[i, case.col, case.col][fin].double(), want_A[fin], "A fp32")
    assert bool(torch.isnan(b32[i, case.col][~fin]).all())


def test_fused_decode_bound():
    """x_j = v / (v^2 + 2^20): fp32 stays within 1e-6 of float64, one e4m3
    step of v moves it by far more than the 2^-12 the GPU test allows."""
    reg = 2.0 ** 20
    case = cf.decode_case(16, reg, lengths=(1,))
    v = cf.own_entry(case)
    fin = torch.isfinite(v)
    i = torch.arange(case.n)
    v, col, i = v[fin], case.col[fin], torch.arange(int(fin.sum()))
    x64 = _diag_solve(*_systems(case, torch.float64), rows=fin)[i, col]
    x32 = _diag_solve(*_systems(case, torch.float32), rows=fin)[i, col]
    want = v.double() / (v.double() ** 2 + reg)
    _eq(x64, want, "float64 x")
    nz = v != 0
    assert float(((x32.double() - want) / want)[nz].abs().max()) < 1e-6
    assert float(((reg - v ** 2) / (reg + v ** 2)).min()) >= 0.67
    tab = cf.e4m3_table()
    f = lambda t: t / (t * t + reg)
    step = ((f(tab[2:]) - f(tab[1:-1])) / f(tab[1:-1])).abs().min()
    assert float(step) >= 0.67 * 2.0 ** -4, float(step)


@pytest.mark.parametrize("k", [16, 64])
def test_scaled_decode_cases_are_exact(k):
    case = cf.decode_case(k, 0.25, scales=cf.FP8_SCALES)
    i = torch.arange(case.n)
    v = cf.own_entry(case)
    s = case.scale[case.last()]
    # + 0.0: the sum starts from +0, so a -0 product arrives as +0
    want = cf.e4m3_decode_oracle(cf.e4m3_oracle(s * v)) + 0.0
    nan = torch.isnan(v)
    want[nan] = cf.NAN
    for dtype in (torch.float32, torch.float64):
        _, b = _systems(case, dtype)
        _eq(cf.canon_nan(b[i, case.col].float()), cf.canon_nan(want),
            f"fp8 scaled b {dtype}")
    fin = ~nan
    assert bool(cf.is_e4m3_tie((s * v)[fin]).any())
    assert bool((want[fin].abs() == 448.0).any())
    assert bool(cf.is_e4m3_subnormal(want[fin]).any())

    case = cf.bf16_scale_case(k)
    i = torch.arange(case.n)
    v, s = cf.own_entry(case), case.scale[case.last()]
    want = cf.bf16_oracle(s * v)
    for dtype in (torch.float32, torch.float64):
        _, b = _systems(case, dtype)
        _eq(b[i, case.col].float().view(torch.int32),
            (want.view(torch.bfloat16).float() + 0.0).view(torch.int32),
            f"bf16 scaled b {dtype}")
    prod = (s * v).contiguous().view(torch.int32)
    assert int(((prod & 0xFFFF) == 0x8000).sum()) > 300          # exact ties
    assert bool(torch.isinf(want.view(torch.bfloat16).float()).any())
    sub = want.view(torch.bfloat16).float()
    assert bool(((sub != 0) & (sub.abs() < 2.0 ** -126)).any())


@pytest.mark.parametrize("k", [16, 64, 128])
def test_widen_tables_are_exact(k):
    seen = 0
    for first, tab in cf.widen_tables(k):
        G32, G64 = R.factor_gram_reference(tab), R.factor_gram_f64(tab)
        for m in range(min(k // 2, 256 - first)):
            v = cf.e4m3_decode_oracle(torch.tensor([first + m]))[0]
            seen += 1
            if torch.isnan(v):
                assert bool(torch.isnan(G32[2 * m + 1, 2 * m]))
                continue
            assert float(G32[2 * m + 1, 2 * m]) == float(v)
            assert float(G32[2 * m, 2 * m]) == float(v) ** 2
            assert float(G64[2 * m, 2 * m]) == float(v) ** 2
    assert seen == 256
