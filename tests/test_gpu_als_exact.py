"""The explicit and weighted ALS kernels on inputs whose correct answer is
exact in fp32 in every summation order (tests/_exact_fixture.py,
docs/KERNELS.md "Exact-integer cases").  Every assertion of parts a-d is an
equality; the images are compared as bit patterns.  The one tolerance in the
file is the solver conditioning ladder at the end.

Which test launches which instantiation (k = 16 * KT; "wave" ranks are
16/32/48/64, "all" adds 80/96/112/128):

  launcher                       instantiations            test
  -----------------------------  ------------------------  -------------------
  fma_gramian                    all k x {bf16, fp8}       test_gramian_exact,
                                                           test_fused_exact
                                                           (slab path)
  fma_gramian_w                  all k x {bf16, fp8}       test_gramian_exact
                                                           (base = 0),
                                                           test_weighted_exact
  fma_cholesky_solve             all k                     test_direct_solvers
                                                           _exact; on the
                                                           Gramian kernels' A
                                                           in the other two
  fma_ldl_solve_wave             wave k                    test_direct_solvers
                                                           _exact
  fma_ldl_solve_wave_reg         wave k x variants {0, 3}  test_direct_solvers
                                                           _exact; variant 3
                                                           also the slab paths
                                                           (k <= 64)
  fma_als_solve_wavefused        wave k x {bf16, fp8}      test_fused_exact
                                 x variants {0, 1, 2, 3}
  fma_als_solve_wavefused_db     wave k (fp8) x {0, 3}     test_fused_exact
  fma_als_solve_fused            all k x {bf16, fp8}       test_fused_exact
  fma_als_solve_wavefused_w      wave k x {bf16, fp8}      test_weighted_exact
  fma_als_solve_fused_w          all k x {bf16, fp8}       test_weighted_exact

Failing shapes found by this file: none so far.
"""

import functools

import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.ops import reference as R

import _exact_fixture as fx

pytestmark = pytest.mark.gpu

RANKS = [16, 32, 48, 64, 80, 96, 112, 128]
GATHERS = ["bf16", "fp8"]
ROW_LENGTHS = fx.ROW_LENGTHS
EDGE_N = (31, 32, 33, 63, 64, 65, 97, 127, 128, 129, 257)
REG = 0.25
ULP32 = 2.0 ** -23


def _hip():
    import flink_ms_amd._hip_ops as hip
    return hip


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    t = t.contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    return t


def _assert_equal(got, want, what):
    """torch.equal with the first differing positions in the message (tile,
    row quad and chunk position are readable from the indices)."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = (got != want) | (got != got)
    idx = bad.nonzero()
    lines = [f"{tuple(i.tolist())}: got {got[tuple(i)].item()!r} "
             f"want {want[tuple(i)].item()!r}" for i in idx[:12]]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} "
                         "elements differ\n  " + "\n  ".join(lines))


def _assert_same_bits(got, want, what):
    _assert_equal(_bits(got), _bits(want), what + " (bit patterns)")


def _outputs(rows, k, gpu):
    """Pre-poisoned fp32 / bf16 / e4m3 outputs: an unwritten element shows."""
    return (torch.full((rows, k), float("nan"), device=gpu),
            torch.full((rows, k), float("nan"), device=gpu,
                       dtype=torch.bfloat16),
            torch.full((rows, k), 0x7F, device=gpu, dtype=torch.uint8))


def _check_solution(what, x, ob, o8, x_true, empty=None, exact_images=False):
    """x == x_true; each image present is the RNE image of x, bit for bit
    (and equal to x_true itself where that is representable); empty rows are
    all-zero bits everywhere."""
    _assert_equal(x, x_true, what + ": x")
    xc = x.cpu()
    if ob is not None:
        _assert_same_bits(ob.cpu(), xc.to(torch.bfloat16), what + ": bf16 image")
        if exact_images:
            _assert_equal(ob.cpu().float(), x_true, what + ": bf16 image value")
    if o8 is not None:
        _assert_same_bits(o8.cpu(), ops.quantize_fp8(xc), what + ": e4m3 image")
        if exact_images:
            _assert_equal(ops.dequantize_fp8(o8.cpu()), x_true,
                          what + ": e4m3 image value")
    if empty is not None:
        assert bool(empty.any())
        for t in (x, ob, o8):
            if t is not None:
                assert not bool((_bits(t.cpu())[empty] != 0).any()), \
                    what + ": empty rows"


def _perm(n, seed, gpu):
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(n, generator=g).to(torch.int32).to(gpu)


# ------------------------------------------------- a. k_gramian, k_gramian_w

@functools.lru_cache(maxsize=None)
def _gramian_case(k, gather):
    """The multi-row integer case and its float64 oracles cast to fp32 (the
    cast is exact: checked here and in test_als_exact_cpu.py)."""
    csr, tab, tab32, scale = fx.integer_gramian_case(k, gather, ROW_LENGTHS,
                                                     seed=500 + k)
    zero = torch.zeros(k, k)
    want = []
    for sc in (torch.ones(csr.nnz), scale):
        A64, b64 = R.gramian_weighted_f64(csr, tab, REG, sc, csr.values, zero)
        A32, b32 = A64.float(), b64.float()
        assert torch.equal(A32.double(), A64)
        assert torch.equal(b32.double(), b64)
        want += [A32, b32]
    return (csr, tab, scale, *want)


@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", RANKS)
def test_gramian_exact(gpu, k, gather):
    csr, tab, scale, A_want, b_want, Aw_want, bw_want = _gramian_case(k, gather)
    hip, st = _hip(), _stream()
    d, t = csr.to(gpu), tab.to(gpu)
    rows = csr.num_rows
    none = torch.empty(0, device=gpu)
    name = f"gramian k={k} {gather}"

    A, b = ops.gramian(d, t, REG)
    _assert_equal(A, A_want, name + ": A")
    _assert_equal(b, b_want, name + ": b")
    _assert_same_bits(A, A.transpose(1, 2), name + ": A == A^T")

    # the weighted twin with base = 0: unit scales give the explicit bits,
    # scales in {1, 2} the weighted oracle
    zero = torch.zeros(k, k, device=gpu)
    ones = torch.ones(csr.nnz, device=gpu)
    A1, b1 = ops.gramian(d, t, REG, scale=ones, ext=d.values, base=zero)
    _assert_same_bits(A1, A, name + ": weighted, unit scales: A")
    _assert_same_bits(b1, b, name + ": weighted, unit scales: b")
    Aw, bw = ops.gramian(d, t, REG, scale=scale.to(gpu), ext=d.values,
                         base=zero)
    _assert_equal(Aw, Aw_want, name + ": weighted A")
    _assert_equal(bw, bw_want, name + ": weighted b")
    _assert_same_bits(Aw, Aw.transpose(1, 2), name + ": weighted A == A^T")

    # a launch schedule only reorders the blocks
    order = _perm(rows, k, gpu)
    A2 = torch.full_like(A, float("nan"))
    b2 = torch.full_like(b, float("nan"))
    hip.gramian(d.indptr, d.indices, d.values, t, A2, b2, order, REG, st)
    _assert_same_bits(A2, A, name + ": row_order A")
    _assert_same_bits(b2, b, name + ": row_order b")
    A2.fill_(float("nan"))
    b2.fill_(float("nan"))
    hip.gramian_w(d.indptr, d.indices, scale.to(gpu), d.values, zero, t, A2,
                  b2, order, REG, st)
    _assert_same_bits(A2, Aw, name + ": weighted row_order A")
    _assert_same_bits(b2, bw, name + ": weighted row_order b")

    # a sliced indptr keeps global offsets, as the slab path passes it
    A3 = torch.full_like(A, float("nan"))
    b3 = torch.full_like(b, float("nan"))
    for s, e in ((0, 5), (5, 11), (11, rows)):
        hip.gramian(d.indptr[s:e + 1], d.indices, d.values, t, A3[s:e],
                    b3[s:e], none, REG, st)
    _assert_same_bits(A3, A, name + ": sliced indptr A")
    _assert_same_bits(b3, b, name + ": sliced indptr b")


# ------------------------------------------------------ b. direct-A solvers

@functools.lru_cache(maxsize=None)
def _graded(k, xmax):
    return fx.graded_batch(k, 33, seed=1000 * xmax + 10 * k, xmax=xmax)


def _poison_upper_tiles(A):
    """NaN in every off-diagonal upper tile (tile column > tile row): the
    solvers load the lower tiles only."""
    A = A.clone()
    k = A.shape[-1]
    for I in range(k // 16):
        A[:, 16 * I:16 * I + 16, 16 * I + 16:] = float("nan")
    return A


def _direct_solvers(k):
    """(name, fn(A, b) -> (x, bf16 image or None, e4m3 image or None))."""
    hip = _hip()

    def chol(A, b):
        x = torch.full_like(b, float("nan"))
        hip.cholesky_solve(A, b, x, _stream())
        return x, None, None

    def wave(A, b):
        o = _outputs(A.shape[0], k, A.device)
        hip.ldl_solve_wave(A, b, *o, _stream())
        return o

    def wave_reg(variant):
        def run(A, b):
            o = _outputs(A.shape[0], k, A.device)
            hip.ldl_solve_wave_reg(A, b, *o, _stream(), variant)
            return o
        return run

    out = [("cholesky_solve", chol)]
    if k <= 64:
        out += [("ldl_solve_wave", wave),
                ("ldl_solve_wave_reg[0]", wave_reg(0)),
                ("ldl_solve_wave_reg[3]", wave_reg(3))]
    return out


@pytest.mark.parametrize("k", RANKS)
def test_direct_solvers_exact(gpu, k):
    """Graded pivots 2^-6 .. 2^6, batches of 33 (33 % 4 == 1: the wave
    kernels' tail block)."""
    for xmax in (3, 1):            # xmax = 1: the e4m3 image batch
        A, b, x_true = _graded(k, xmax)
        for poisoned in (False, True):
            Ag = (_poison_upper_tiles(A) if poisoned else A).to(gpu)
            for name, solve in _direct_solvers(k):
                what = (f"{name} k={k} x in +-{xmax}"
                        + (" NaN upper tiles" if poisoned else ""))
                x, ob, o8 = solve(Ag, b.to(gpu))
                _check_solution(what, x, ob, o8, x_true, exact_images=True)


# ---------------------------------------------------------- c. fused kernels

@functools.lru_cache(maxsize=None)
def _ldl_batch(k, gather):
    """One launch of the ldl family: n in {k, k+1} and every chunk edge
    >= k, an empty row in the middle, batch size = 3 mod 4."""
    ns = sorted({k, k + 1} | {n for n in EDGE_N if n >= k})
    while (len(ns) + 1) % 4 != 3:
        ns.append(k + 2 + len(ns))
    seed = 40_000 + 100 * k + (0 if gather == "bf16" else 50)
    pieces = [fx.ldl_family(k, n, seed + i, gather) for i, n in enumerate(ns)]
    pieces.insert(len(pieces) // 2, fx.empty_piece(k))
    assert len(pieces) % 4 == 3
    return fx.combine(pieces, gather)


@functools.lru_cache(maxsize=None)
def _diag_batch(k, gather):
    p = fx.diag_family(k, gather)
    return fx.combine([p, fx.empty_piece(k), p], gather)


def _fused_runs(k, gather, bt, gpu):
    """Every way to the fused explicit kernels: (name, fn(row_order or None)
    -> (x, bf16 image or None, e4m3 image or None))."""
    hip = _hip()
    fp8 = gather == "fp8"
    d, t = bt.csr.to(gpu), bt.table.to(gpu)
    rows = bt.csr.num_rows
    none = torch.empty(0, device=gpu)

    def wavefused(fn, variant):
        def run(ro):
            o = _outputs(rows, k, gpu)
            fn(d.indptr, d.indices, d.values, t, *o,
               none if ro is None else ro, bt.reg, _stream(), variant)
            return o
        return run

    def block(ro):
        x, ob, o8 = _outputs(rows, k, gpu)
        hip.als_solve_fused(d.indptr, d.indices, d.values, t, x,
                            none if fp8 else ob, o8 if fp8 else none,
                            none if ro is None else ro, bt.reg, _stream())
        return x, (None if fp8 else ob), (o8 if fp8 else None)

    def side(**kw):
        def run(ro):
            _, ob, o8 = _outputs(rows, k, gpu)
            x = ops.als_solve_side(d, t, bt.reg, out_bf16=ob, out_fp8=o8,
                                   row_order=ro, **kw)
            # the block kernel (every k > 64 call, slab_rows or not) writes
            # the image of the gather dtype only
            blk = k > 64 or kw.get("fused", False)
            return (x, None if blk and fp8 else ob,
                    None if blk and not fp8 else o8)
        return run

    runs = [("als_solve_fused", block),
            ("als_solve_side", side()),
            ("als_solve_side fused", side(fused=True)),
            ("als_solve_side slab_rows=5", side(slab_rows=5))]
    if k <= 64:
        runs += [(f"als_solve_wavefused[{v}]",
                  wavefused(hip.als_solve_wavefused, v)) for v in range(4)]
        if fp8:
            runs += [(f"als_solve_wavefused_db[{v}]",
                      wavefused(hip.als_solve_wavefused_db, v))
                     for v in (0, 3)]
    return runs


@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", RANKS)
def test_fused_exact(gpu, k, gather):
    fp8 = gather == "fp8"
    for family, bt in (("ldl", _ldl_batch(k, gather)),
                       ("diag", _diag_batch(k, gather))):
        rows = bt.csr.num_rows
        empty = bt.csr.row_counts() == 0
        d, t = bt.csr.to(gpu), bt.table.to(gpu)
        # the modular pieces first: A and b are the closed form
        A, b = ops.gramian(d, t, bt.reg)
        _assert_equal(A, bt.A, f"{family} k={k} {gather}: gramian A")
        _assert_equal(b, bt.b, f"{family} k={k} {gather}: gramian b")
        _assert_equal(ops.cholesky_solve(A, b), bt.x_true,
                      f"{family} k={k} {gather}: gramian + cholesky_solve")
        order = _perm(rows, 3 * k, gpu)
        for name, run in _fused_runs(k, gather, bt, gpu):
            for ro in (None, order):
                if ro is not None and "slab_rows" in name:
                    continue        # multi-slab runs take no schedule
                what = (f"{name} {family} k={k} {gather}"
                        + (" row_order" if ro is not None else ""))
                x, ob, o8 = run(ro)
                _check_solution(what, x, ob, o8, bt.x_true, empty,
                                exact_images=family == "ldl")
        # als_solve_chunk: a shuffled subset of the entities, scattered into
        # full-side buffers; the other rows stay untouched
        ids = _perm(rows, 5 * k, gpu)[: rows // 2 + 1]
        x, ob, o8 = _outputs(rows, k, gpu)
        block = k > 64
        ops.als_solve_chunk(d, t, bt.reg, x, None if block and not fp8 else o8,
                            None if block and fp8 else ob, ids)
        hit = torch.zeros(rows, dtype=torch.bool)
        hit[ids.cpu().long()] = True
        what = f"als_solve_chunk {family} k={k} {gather}"
        _check_solution(what, x[ids.long()],
                        None if block and fp8 else ob[ids.long()],
                        None if block and not fp8 else o8[ids.long()],
                        bt.x_true[ids.cpu().long()],
                        exact_images=family == "ldl")
        assert bool(torch.isnan(x.cpu()[~hit]).all()), what + ": other rows"
        assert bool((o8.cpu()[~hit] == 0x7F).all()), what + ": other rows"


# ---------------------------------------------------------- d. weighted twins

@functools.lru_cache(maxsize=None)
def _weighted_batch(k, gather):
    ns = sorted({k, k + 1} | {n for n in (33, 65, 129, 257) if n >= k})
    while (len(ns) + 1) % 4 != 3:
        ns.append(k + 2 + len(ns))
    seed = 60_000 + 100 * k + (0 if gather == "bf16" else 50)
    pieces = [fx.weighted_family(k, n, seed + i, gather)
              for i, n in enumerate(ns)]
    pieces.insert(len(pieces) // 2, fx.empty_weighted_piece(k))
    assert len(pieces) % 4 == 3
    return fx.combine(pieces, gather)


@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", RANKS)
def test_weighted_exact(gpu, k, gather):
    hip = _hip()
    fp8 = gather == "fp8"
    bt = _weighted_batch(k, gather)
    rows = bt.csr.num_rows
    empty = bt.csr.row_counts() == 0
    d, t = bt.csr.to(gpu), bt.table.to(gpu)
    sc, ext = bt.scale.to(gpu), d.values
    # only the lower triangle of the base may be read
    base = (torch.tril(bt.base)
            + torch.triu(torch.full((k, k), 1e30), 1)).to(gpu)
    none = torch.empty(0, device=gpu)
    name = f"k={k} {gather}"

    A, b = ops.gramian(d, t, bt.reg, scale=sc, ext=ext, base=base)
    _assert_equal(A, bt.A, f"gramian_w {name}: A")
    _assert_equal(b, bt.b, f"gramian_w {name}: b")
    _assert_same_bits(A, A.transpose(1, 2), f"gramian_w {name}: A == A^T")

    order = _perm(rows, 7 * k, gpu)
    for ro in (None, order):
        tag = name + (" row_order" if ro is not None else "")
        rarg = none if ro is None else ro
        if k <= 64:
            x, ob, o8 = _outputs(rows, k, gpu)
            hip.als_solve_wavefused_w(d.indptr, d.indices, sc, ext, base, t,
                                      x, ob, o8, rarg, bt.reg, _stream())
            _check_solution(f"als_solve_wavefused_w {tag}", x, ob, o8,
                            bt.x_true, empty, exact_images=True)
        x, ob, o8 = _outputs(rows, k, gpu)
        hip.als_solve_fused_w(d.indptr, d.indices, sc, ext, base, t, x,
                              none if fp8 else ob, o8 if fp8 else none, rarg,
                              bt.reg, _stream())
        _check_solution(f"als_solve_fused_w {tag}", x, None if fp8 else ob,
                        o8 if fp8 else None, bt.x_true, empty,
                        exact_images=True)
        # the wrapper's default path for this rank
        _, ob, o8 = _outputs(rows, k, gpu)
        x = ops.als_solve_side(d, t, bt.reg, out_bf16=ob, out_fp8=o8,
                               row_order=ro, scale=sc, ext=ext, base=base)
        _check_solution(f"als_solve_side weighted {tag}", x,
                        None if k > 64 and fp8 else ob,
                        None if k > 64 and not fp8 else o8, bt.x_true, empty,
                        exact_images=True)
    # gramian_w + the unchanged solvers: the slab path (k <= 64; above, the
    # wrapper takes the block kernel whatever slab_rows says) and by hand
    _, ob, o8 = _outputs(rows, k, gpu)
    x = ops.als_solve_side(d, t, bt.reg, out_bf16=ob, out_fp8=o8,
                           slab_rows=4, scale=sc, ext=ext, base=base)
    _check_solution(f"als_solve_side weighted slab_rows=4 {name}", x,
                    None if k > 64 and fp8 else ob,
                    None if k > 64 and not fp8 else o8, bt.x_true, empty,
                    exact_images=True)
    _assert_equal(ops.cholesky_solve(A, b), bt.x_true,
                  f"gramian_w + cholesky_solve {name}")


# ------------------------------------------- 4. solver conditioning ladder

@functools.lru_cache(maxsize=None)
def _ladder(k, cond):
    """33 systems A = Q diag(lambda) Q^T, lambda log-spaced over ``cond``,
    symmetrised and cast to fp32; b normal.  Returns (A, b, x64, x32)."""
    g = torch.Generator().manual_seed(int(cond) + k)
    Q, _ = torch.linalg.qr(torch.randn(33, k, k, generator=g,
                                       dtype=torch.float64))
    lam = torch.logspace(0, -torch.log10(torch.tensor(cond)).item(), k,
                         dtype=torch.float64)
    A = (Q * lam) @ Q.transpose(1, 2)
    A = ((A + A.transpose(1, 2)) / 2).float().contiguous()
    b = torch.randn(33, k, generator=g)
    x64 = torch.linalg.solve(A.double(), b.double().unsqueeze(2)).squeeze(2)
    x32 = R.cholesky_solve_reference(A, b)
    return A, b, x64, x32


@pytest.mark.parametrize("cond", [1e1, 1e3, 1e5])
@pytest.mark.parametrize("k", [16, 64, 128])
def test_solver_conditioning_ladder(gpu, k, cond):
    """The K3-K5 criterion, batch-max and forward error on purpose:
    max|x - x64| <= 4 * max|x32 - x64| + 4 * 2^-23 * max|x64|, x64 =
    torch.linalg.solve in float64 on the fp32 A and b, x32 =
    R.cholesky_solve_reference.  A plain fp32 LDL^T of the kernels' shape
    (test_als_exact_cpu.ldl_right_looking) stays below 2.4x on these nine
    ladder points; per-system and backward-error ratios of an honest solver
    reach 6x and 3.7x, so those are not asserted."""
    A, b, x64, x32 = _ladder(k, cond)
    ref = float((x32.double() - x64).abs().max())
    tol = 4.0 * ref + 4.0 * ULP32 * float(x64.abs().max())
    for name, solve in _direct_solvers(k):
        x, _, _ = solve(A.to(gpu), b.to(gpu))
        err = float((x.cpu().double() - x64).abs().max())
        print(f"ladder {name} k={k} cond={cond:.0e}: err {err:.3e} "
              f"fp32-reference {ref:.3e} ratio {err / ref:.2f} tol {tol:.3e}")
        assert err <= tol, (name, k, cond, err, tol)
