"""Every e4m3 / bf16 conversion of the ALS kernels over the whole value
range, bit for bit (tests/_conversion_fixture.py, docs/KERNELS.md
"Conversions").

The contract: e4m3 encodes round to nearest, ties to the even byte, finite
values beyond +-448 saturate, inf / NaN become a NaN byte; e4m3 decodes are
exact, subnormals included; bf16 encodes are RNE with overflow to inf.  A NaN
compares as "is a NaN" only.  The expected bytes come from the fixture's
table / integer oracles, not from a torch cast (test_conversions_cpu.py holds
the host casts to the same oracles).

Every system has one entry that matters, a diagonal A of powers of two and
one non-zero right-hand-side element, so nothing but the conversion under
test rounds and the comparisons are equalities.  The one tolerance is the
derived 2^-12 of test_fused_decode (its docstring).

Which test launches which binding and conversion site:

  binding                     conversion sites                  test
  --------------------------  --------------------------------  -------------
  ldl_solve_wave              f2fp8 / f2bf epilogue             test_direct
  ldl_solve_wave_reg [0, 3]   f2fp8 / f2bf epilogue              _solver
                                                                 _images
  als_solve_wavefused [0-3]   epilogue; rating pair (stage_     test_fused
  als_solve_wavefused_w       ext_commit, lanes 0-31 of the      _images (rows
                              split-wave map / all of it);       of 1) /
                              MFMA decode                        test_rating
  als_solve_wavefused_db      epilogue; rating pair              _pairs_long
                              (stage_loads); MFMA decode         _rows (rows
  als_solve_fused             epilogue (x8_row / xb_row);        of 33 - 65);
  als_solve_fused_w           rating pair (stage_ext_commit;     test_fused
                              stage_ext_quad_w at k = 112        _decode
                              bf16); MFMA decode
  gramian                     rating pair (stage_ext_commit;    test_rating
                              stage_ext_quad_w at k = 112        _pairs
                              bf16), slots 0 - 31, tail chunks
  gramian (e4m3)              MFMA e4m3 operand decode, all     test_mfma
                              256 bytes                          _decode
  gramian_w (e4m3)            cvt_pk_f32_fp8, cvt_pk_fp8_f32,   test_scaled
                              stage_fp8_sat                      _rounding
  gramian_w (bf16)            convertvector to bf16              _fp8 / _bf16
  factor_gram (e4m3)          stage_widen_fp8x8 (fp82f, f2bf)   test_widen

stage_ext_quad_w (the 8-lane EXT conversion) is instantiated for one shape
only, the bf16 gather at k = 112 of the block kernels and k_gramian (EXT8 in
gramian_to_lds); its e4m3 branch is never instantiated.  Hence the k = 112
bf16 cases.

The weighted twins run with scale = 1 and base = 0 here; their rescale is
held by test_scaled_rounding through gramian_w, which shares the staging.

What the fused kernels cannot show: their b comes out of an MFMA whose
accumulator starts at +0, and +0 + -0 = +0, so x never holds a -0 in its
own column (the expected x has +0 there and that column is compared as bit
patterns; the other columns are compared as numbers, the sign of a zero
that the substitutions leave there is not pinned).  With bf16 gathers the
e4m3 image byte 0x80 is reached through negative underflow instead
(asserted); with e4m3 gathers x = pair(r) is a sum of two e4m3 values, never
a non-zero below 2^-9, so only the direct-A solvers (b given as it is) write
that byte.  With e4m3 gathers the rating pair reaches every representable
value and every tie with a representable half step, not the ties' fp32
neighbours; with bf16 gathers the pair holds them all.

Failing conversions found by this file: none so far (the scratch mutants
it does catch are listed in docs/KERNELS.md "Conversions").
"""

import functools

import pytest
import torch

from flink_ms_amd import ops

import _conversion_fixture as cf

pytestmark = pytest.mark.gpu

X_SENTINEL, BF_SENTINEL, F8_SENTINEL = 12345.0, 77.0, 0x55
EXTRA_ROWS = 3


def _hip():
    import flink_ms_amd._hip_ops as hip
    return hip


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _assert_bits(got, want, what):
    """Equal bit patterns, NaNs canonicalised; the first differences named."""
    g, w = cf.canon_nan(got.cpu()), cf.canon_nan(want.cpu())
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if torch.equal(g, w):
        return
    idx = (g != w).nonzero()
    lines = [f"{tuple(i.tolist())}: got {int(g[tuple(i)]):#x} "
             f"want {int(w[tuple(i)]):#x}" for i in idx[:12]]
    raise AssertionError(f"{what}: {idx.shape[0]} of {g.numel()} elements "
                         "differ\n  " + "\n  ".join(lines))


def _check_images(what, x, ob, o8):
    """Each image present is the contract's conversion of the kernel's own
    fp32 x, by the oracles (and the host casts agree with those)."""
    xc = x.cpu()
    if ob is not None:
        want = cf.bf16_oracle(xc)
        _assert_bits(xc.to(torch.bfloat16), want, what + ": host bf16 cast")
        _assert_bits(ob, want, what + ": bf16 image")
    if o8 is not None:
        want = cf.e4m3_oracle(xc)
        _assert_bits(ops.quantize_fp8(xc), want, what + ": host e4m3 cast")
        _assert_bits(o8, want, what + ": e4m3 image")


def _outputs(rows, k, gpu):
    return (torch.full((rows, k), X_SENTINEL, device=gpu),
            torch.full((rows, k), BF_SENTINEL, device=gpu,
                       dtype=torch.bfloat16),
            torch.full((rows, k), F8_SENTINEL, device=gpu, dtype=torch.uint8))


def _check_sentinels(what, n, x, ob, o8):
    assert bool((x[n:] == X_SENTINEL).all()), what + ": x past the launch"
    if ob is not None:
        assert bool((ob[n:].float() == BF_SENTINEL).all()), \
            what + ": bf16 image past the launch"
    if o8 is not None:
        assert bool((o8[n:] == F8_SENTINEL).all()), \
            what + ": e4m3 image past the launch"


# ------------------------------------------------- 2a. direct-A solvers

def _direct_solvers(k):
    hip = _hip()

    def wave(A, b, o):
        hip.ldl_solve_wave(A, b, *o, _stream())

    def wave_reg(variant):
        def run(A, b, o):
            hip.ldl_solve_wave_reg(A, b, *o, _stream(), variant)
        return run

    return [("ldl_solve_wave", wave), ("ldl_solve_wave_reg[0]", wave_reg(0)),
            ("ldl_solve_wave_reg[3]", wave_reg(3))]


@pytest.mark.parametrize("k", [16, 64])
def test_direct_solver_images(gpu, k):
    """A = I, so x = b: row i holds one edge value in column i mod k.  The
    finite edges of both formats in one batch, the non-finite ones in a
    batch of their own (0 * inf poisons a row)."""
    finite = torch.cat([cf.e4m3_edges(), cf.bf16_edges()])
    for tag, vals in (("finite", finite), ("non-finite", cf.specials())):
        n = vals.numel()
        i = torch.arange(n)
        b = torch.zeros(n, k)
        b[i, i % k] = vals
        A = torch.eye(k, device=gpu).expand(n, k, k).contiguous()
        for name, solve in _direct_solvers(k):
            what = f"{name} k={k} {tag}"
            o = _outputs(n, k, gpu)
            solve(A, b.to(gpu), o)
            x, ob, o8 = (t.cpu() for t in o)
            _check_images(what, x, ob, o8)
            own = x[i, i % k]
            if tag == "non-finite":
                # the substitutions multiply an inf by the zeros of L, so
                # an inf b comes back as NaN: the images follow x, whatever
                assert not bool(torch.isfinite(own[2:]).any()), what
                continue
            normal = vals.abs() >= 2.0 ** -126
            _assert_bits(own[normal], vals[normal], what + ": x == b")
            for name_, fn in (("tie", cf.is_e4m3_tie),
                              ("subnormal", cf.is_e4m3_subnormal),
                              ("saturated", cf.is_e4m3_saturated),
                              ("-0 image", cf.is_e4m3_negzero)):
                assert bool(fn(own.contiguous()).any()), (what, name_)


# ----------------------------------------------------- 2b. fused kernels

def _fused_kernels(k, gather, gpu):
    """(name, fn(case on the GPU: csr, table, values, reg, outputs) -> the
    images it writes), every fused binding of this rank and gather."""
    hip = _hip()
    fp8 = gather == "fp8"
    none = torch.empty(0, device=gpu)

    def wavefused(fn, variant):
        def run(d, t, reg, o):
            fn(d.indptr, d.indices, d.values, t, *o, none, reg, _stream(),
               variant)
            return o
        return run

    def wavefused_w(d, t, reg, o):
        hip.als_solve_wavefused_w(
            d.indptr, d.indices, torch.ones_like(d.values), d.values,
            torch.zeros(k, k, device=gpu), t, *o, none, reg, _stream())
        return o

    def block(d, t, reg, o):
        x, ob, o8 = o
        hip.als_solve_fused(d.indptr, d.indices, d.values, t, x,
                            none if fp8 else ob, o8 if fp8 else none, none,
                            reg, _stream())
        return x, (None if fp8 else ob), (o8 if fp8 else None)

    def block_w(d, t, reg, o):
        x, ob, o8 = o
        hip.als_solve_fused_w(
            d.indptr, d.indices, torch.ones_like(d.values), d.values,
            torch.zeros(k, k, device=gpu), t, x, none if fp8 else ob,
            o8 if fp8 else none, none, reg, _stream())
        return x, (None if fp8 else ob), (o8 if fp8 else None)

    if k > 64:
        return [("als_solve_fused", block), ("als_solve_fused_w", block_w)]
    runs = [(f"als_solve_wavefused[{v}]",
             wavefused(hip.als_solve_wavefused, v)) for v in range(4)]
    if fp8:
        runs += [(f"als_solve_wavefused_db[{v}]",
                  wavefused(hip.als_solve_wavefused_db, v)) for v in (0, 3)]
    return runs + [("als_solve_wavefused_w", wavefused_w)]


@functools.lru_cache(maxsize=None)
def _fused_case(k, gather, a):
    case = cf.fused_case(k, gather, a)
    return case, cf.fused_x(case, 2.0 ** (a - 1))


def _check_x(what, x, want, case):
    """x == want as numbers everywhere, as bit patterns in the own column."""
    bad = (x != want).nonzero()
    assert bad.numel() == 0, (what, bad.shape[0], [
        (i, j, float(x[i, j]), float(want[i, j]))
        for i, j in bad[:8].tolist()])
    i = torch.arange(case.n)
    _assert_bits(x[i, case.col], want[i, case.col], what + ": x[j]")


def _launch(run, case, gpu):
    """One launch into outputs with EXTRA_ROWS sentinel rows behind it."""
    k = case.table.shape[1]
    o = _outputs(case.n + EXTRA_ROWS, k, gpu)
    x, ob, o8 = run(case.csr.to(gpu), case.table.to(gpu), case.reg, o)
    torch.cuda.synchronize()
    return (x.cpu(), None if ob is None else ob.cpu(),
            None if o8 is None else o8.cpu())


# k = 112 bf16: the one shape with the 8-lane EXT conversion
FUSED_SHAPES = [(k, g) for k in (16, 64, 80, 128) for g in ("bf16", "fp8")
                ] + [(112, "bf16")]


@pytest.mark.parametrize("k, gather", FUSED_SHAPES)
def test_fused_images(gpu, k, gather):
    """x_j = 2^(a-1) * pair(r) exactly: a = 1 walks the body of the range,
    a = 4 goes beyond +-448."""
    for name, run in _fused_kernels(k, gather, gpu):
        owns = []
        for a in (1, 4):
            case, want = _fused_case(k, gather, a)
            what = f"{name} k={k} {gather} a={a}"
            x, ob, o8 = _launch(run, case, gpu)
            n = case.n
            _check_sentinels(what, n, x, ob, o8)
            x, ob, o8 = (None if t is None else t[:n] for t in (x, ob, o8))
            _check_x(what, x, want, case)
            _check_images(what, x, ob, o8)
            owns.append(x[torch.arange(n), case.col])
        own = torch.cat(owns)
        classes = [("tie", cf.is_e4m3_tie),
                   ("subnormal", cf.is_e4m3_subnormal),
                   ("saturated", cf.is_e4m3_saturated)]
        if gather == "bf16":        # see the module docstring
            classes.append(("-0 image", cf.is_e4m3_negzero))
        for name_, fn in classes:
            assert bool(fn(own).any()), (name, k, gather, name_)


# ------------------------------------------------ 3. rating-pair encoders

@functools.lru_cache(maxsize=None)
def _rating_case(k, gather):
    case = cf.rating_case(k, gather)
    r = case.csr.values[case.last()]
    # + 0.0: the MFMA sum starts from +0, so a -0 pair arrives as +0
    return case, cf.oracle_pair(r, gather) + 0.0


@pytest.mark.parametrize("k, gather", [(16, "bf16"), (64, "bf16"),
                                       (16, "fp8"), (64, "fp8"),
                                       (112, "bf16")])
def test_rating_pairs(gpu, k, gather):
    """b[j] = pair(r) bit for bit over the gather dtype's whole edge set,
    with the edge rating in the last slot of rows of RATING_LENGTHS entries
    (k_gramian stages every chunk with lanes 0-31, or 0-7 at k = 112 bf16:
    slots 0, 5, 15, 26, 31 and the one-entry tail chunks of 33 and 65)."""
    case, pair = _rating_case(k, gather)
    host = ops.fp8_rating_pair if gather == "fp8" else ops.bf16_rating_pair
    _assert_bits(host(case.csr.values[case.last()]) + 0.0, pair,
                 f"host {gather} rating pair")
    A, b = ops.gramian(case.csr.to(gpu), case.table.to(gpu), case.reg)
    i = torch.arange(case.n, device=gpu)
    col = case.col.to(gpu)
    bj = b[i, col].cpu()
    for ln in cf.RATING_LENGTHS:
        sel = case.lengths == ln
        assert int(sel.sum()) > 100
        _assert_bits(bj[sel], pair[sel],
                     f"gramian {gather} k={k} rows of {ln}: b[j]")
    assert torch.equal(A[i, col, col].cpu(), 1 + case.reg * case.lengths)


@pytest.mark.parametrize("k, gather", [(16, "bf16"), (64, "bf16"),
                                       (16, "fp8"), (64, "fp8"),
                                       (112, "bf16")])
def test_rating_pairs_long_rows(gpu, k, gather):
    """Every fused kernel of the rank on rows of 33, 48, 64 and 65 entries
    with the edge rating last: lanes 32, 47 and 63 of the split-wave EXT map
    of k_als_solve_wavefused (two chunks per wave: every e4m3 rank, bf16 at
    k = 16), a third chunk, stage_loads of the pipelined kernel, and at
    k = 112 the block kernels' 8-lane conversion.  Unit table row and reg =
    0, so x_j = pair(r) (cf.long_row_case)."""
    case = cf.long_row_case(k, gather)
    want = cf.fused_x(case, 1.0)
    for name, run in _fused_kernels(k, gather, gpu):
        what = f"{name} k={k} {gather} long rows"
        x, ob, o8 = _launch(run, case, gpu)
        _check_sentinels(what, case.n, x, ob, o8)
        x, ob, o8 = (None if t is None else t[:case.n] for t in (x, ob, o8))
        _check_x(what, x, want, case)
        _check_images(what, x, ob, o8)


# ---------------------------------------------------- 4. e4m3 decoders

@pytest.mark.parametrize("k", [16, 64, 128])
def test_mfma_decode(gpu, k):
    """The MFMA's own e4m3 operand decode: b[j] = v and A[j][j] = v^2 + reg
    * n for the 254 finite bytes (v^2 needs 8 bits), NaN for 0x7F / 0xFF;
    the byte sits in slot 0, 4, 16 and 31 of its chunk."""
    case = cf.decode_case(k, 0.25)
    v = cf.e4m3_decode_oracle(case.csr.indices[case.last()].to(torch.uint8))
    A, b = ops.gramian(case.csr.to(gpu), case.table.to(gpu), case.reg)
    i = torch.arange(case.n, device=gpu)
    col = case.col.to(gpu)
    bj, ajj = b[i, col].cpu(), A[i, col, col].cpu()
    for ln in cf.DECODE_LENGTHS:
        sel = case.lengths == ln
        _assert_bits(bj[sel], (v + 0.0)[sel], f"k={k} slot {ln - 1}: b[j]")
        _assert_bits(ajj[sel], (v * v + 0.25 * case.lengths)[sel],
                     f"k={k} slot {ln - 1}: A[j][j]")
    assert int(torch.isnan(bj).sum()) == 2 * len(cf.DECODE_LENGTHS)


@pytest.mark.parametrize("k", [16, 64, 80, 128])
def test_fused_decode(gpu, k):
    """The fused e4m3 kernels cannot show A: with reg = 2^20 and rating 1,
    x_j = v / (v^2 + 2^20).  Bound 2^-12 relative to the float64 value:
    fp32 arithmetic of the one-term system stays within 1e-6 of it, and a
    decode one e4m3 step off moves x_j by at least 0.67 * 2^-4 (both shown
    in test_conversions_cpu.test_fused_decode_bound)."""
    case = cf.decode_case(k, 2.0 ** 20, lengths=(1,))
    v = cf.own_entry(case).double()
    want = v / (v * v + 2.0 ** 20)
    fin = torch.isfinite(v)
    i = torch.arange(case.n)
    for name, run in _fused_kernels(k, "fp8", gpu):
        x, _, _ = _launch(run, case, gpu)
        own = x[:case.n][i, case.col].double()
        assert bool(torch.isnan(own[~fin]).all()), name
        assert bool((own[fin & (v == 0)] == 0).all()), name
        nz = fin & (v != 0)
        rel = ((own - want) / want)[nz].abs()
        assert float(rel.max()) <= 2.0 ** -12, (
            name, k, float(rel.max()),
            int(case.csr.indices[case.last()][nz][rel.argmax()]))


def _scaled_b(case, gpu, with_A=False):
    k = case.table.shape[1]
    d = case.csr.to(gpu)
    A, b = ops.gramian(d, case.table.to(gpu), case.reg,
                       scale=case.scale.to(gpu), ext=d.values,
                       base=torch.zeros(k, k, device=gpu))
    i, col = torch.arange(case.n, device=gpu), case.col.to(gpu)
    if with_A:
        return b[i, col].cpu(), A[i, col, col].cpu()
    return b[i, col].cpu()


@pytest.mark.parametrize("k", [16, 64])
def test_scaled_rounding_fp8(gpu, k):
    """stage_rescale_fp8x4: decode, one fp32 multiply, saturate, encode.
    b[j] = the contract's e4m3 rounding of fl32(s * v), for all 256 bytes
    times FP8_SCALES (ties from 1.5 / 0.75, subnormal results from 2^-7,
    saturation from 300 and 3)."""
    case = cf.decode_case(k, 0.25, scales=cf.FP8_SCALES)
    v, s = cf.own_entry(case), case.scale[case.last()]
    want = cf.e4m3_decode_oracle(cf.e4m3_oracle(s * v)) + 0.0
    want[torch.isnan(v)] = cf.NAN
    host = ops.dequantize_fp8(ops.quantize_fp8(s * v)) + 0.0
    _assert_bits(host, want, "host quantize_fp8(s * v)")
    got = _scaled_b(case, gpu)
    for n, sc in enumerate(cf.FP8_SCALES):
        sel = slice(256 * n, 256 * n + 256)
        _assert_bits(got[sel], want[sel], f"k={k} scale {sc!r}: b[j]")


@pytest.mark.parametrize("k", [16, 64])
def test_scaled_rounding_bf16(gpu, k):
    """stage_rescale_bf16x2: b[j] = RNE_bf16(fl32(s * v)) for 768 bf16
    values times BF16_SCALES (odd mantissas times 1.5 are exact ties).
    Where the product overflows to +-inf, b[j] = inf * hi + inf * lo with
    the rating pair (1, 0) is NaN whatever the encoder does; A[j][j] = inf^2
    + reg = +inf shows that it wrote an inf and not a NaN."""
    case = cf.bf16_scale_case(k)
    v, s = cf.own_entry(case), case.scale[case.last()]
    want = cf.bf16_oracle(s * v).view(torch.bfloat16).float() + 0.0
    _assert_bits((s * v).to(torch.bfloat16).float() + 0.0, want, "host cast")
    got, ajj = _scaled_b(case, gpu, with_A=True)
    m = cf.bf16_values().numel()
    inf = torch.isinf(want)
    assert 0 < int(inf.sum()) < m // 2      # the top exponent, not the rest
    for n, sc in enumerate(cf.BF16_SCALES):
        sel = torch.zeros_like(inf)
        sel[m * n:m * n + m] = True
        _assert_bits(got[sel & ~inf], want[sel & ~inf],
                     f"k={k} scale {sc!r}: b[j]")
    assert bool((ajj[inf] == cf.INF).all()), "overflow must give inf"


@pytest.mark.parametrize("k", [16, 64, 128])
def test_widen(gpu, k):
    """stage_widen_fp8x8 (fp82f then f2bf) through factor_gram: byte v in
    column 2m and 1.0 in column 2m + 1 give G[2m+1][2m] = v and G[2m][2m] =
    v^2 exactly, NaN for the two NaN bytes."""
    for first, tab in cf.widen_tables(k):
        G = ops.factor_gram(tab.to(gpu)).cpu()
        m = torch.arange(min(k // 2, 256 - first))
        v = cf.e4m3_decode_oracle((first + m).to(torch.uint8))
        _assert_bits(G[2 * m + 1, 2 * m], v + 0.0, f"k={k} bytes {first}..: v")
        _assert_bits(G[2 * m, 2 * m], v * v, f"k={k} bytes {first}..: v^2")
