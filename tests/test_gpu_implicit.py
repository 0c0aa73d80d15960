"""The weighted (implicit-feedback) ALS kernels and ``k_factor_gram`` on the
GPU, against the explicit kernels, the fp32 reference and the float64
oracles of ``flink_ms_amd.ops.reference``.

Tolerances are derived (docs/KERNELS.md "Implicit feedback"):
- staging: none -- the weighted kernel with ``base = 0`` stages the same
  bytes in the same order as the explicit kernel on the expanded table
  ``F~[j] = round_D(s_j * F[indices[j]])``, so A and b are ``torch.equal``;
- base / factor Gram: the project's dot bound ``2 * n * 2^-24 * sum|terms|``
  per entry (n counts every addition, it also covers a truncating
  accumulator);
- fused solves, bf16 gathers: 4x the fp32 torch reference's distance from
  the float64 oracle on the same effective rows plus 4 fp32 ulps of
  ``max|x|`` (the K3-K5 convention of test_gpu_svm_serve.py).
- fused solves, e4m3 gathers: that criterion does not hold for fp8 MFMA
  accumulation.  ``v_mfma_f32_16x16x32_fp8_fp8`` sums its 32 products with
  about 2^-17 relative precision: the Gramian of the EXPLICIT kernel is
  6-7e-6 off the float64 one (bf16: 1e-7), identically with and without a
  base, and solving the kernel's own A, b in float64 reproduces the whole
  error of x.  The explicit kernel on the expanded-table form of the
  base = 0 problems misses the 4x criterion itself -- measured
  |x - x_f64| / (fp32 reference's distance), wave kernel k = 16/32/48/64:
  2.5 / 82 / 50 / 154, block kernel k = 80/128: 38 / 38 -- so, as the
  design note provides for, the factor is twice the explicit kernel's
  worst measured ratio per path (FP8_EXPLICIT_RATIO) in place of 4.  The
  weighted kernels measured 51 / 46 / 41 / 71 (wave) and 64 / 43 (block)
  with a base, and were bit-equal to the explicit kernel at base = 0 in
  every case.  Each run prints the explicit kernel's ratio again.

Data keeps |scale * f| <= 64 and |ext| <= 64 (no e4m3 saturation), reg > 0.
"""

import functools

import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.data.blocked import CSR
from flink_ms_amd.models.als import ALSConfig, ALSTrainer
from flink_ms_amd.ops import reference as R

import _implicit_fixture as fx

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
ULP32 = 2.0 ** -23
ALPHA = 100.0           # |r| = 4 -> alpha*|r| = 400, scale 20, ext 20.05
REG = 0.25
NCOLS = 50
GATHERS = ["fp8", "bf16"]
# worst measured ratio of the EXPLICIT e4m3 kernel to the fp32 reference's
# distance from the oracle (module docstring); bf16 keeps the plain 4x
FP8_EXPLICIT_RATIO = fx.FP8_EXPLICIT_RATIO


def _factor(gather, path):
    return 2.0 * FP8_EXPLICIT_RATIO[path] if gather == "fp8" else 4.0


@functools.lru_cache(maxsize=None)
def _case(k, gather):
    """CPU-side problem, built once per (k, gather) and never modified."""
    csr = fx.csr_with_row_lengths(fx.ROW_LENGTHS, NCOLS, seed=100 + k)
    tab = fx.factor_table(NCOLS, k, seed=200 + k, gather=gather)
    s, e = ops.implicit_weights(csr.values, ALPHA)
    assert (csr.values < 0).any() and (csr.values == 0).any()
    assert float((ALPHA * csr.values.abs()).max()) >= 400.0
    rows, pair = R.effective_rows(csr, tab, s, e)
    assert float(rows.abs().max()) <= 64 and float(e.abs().max()) <= 64
    return csr, tab, s, e, rows


def _expanded(csr, rows, e, gather):
    """The explicit form of a weighted problem: one table row per stored
    entry, already scaled and rounded; ratings = ext."""
    tab = ops.quantize_fp8(rows) if gather == "fp8" else rows.to(torch.bfloat16)
    nnz = csr.indices.numel()
    return CSR(csr.indptr, torch.arange(nnz, dtype=torch.int32), e.clone(),
               csr.num_rows, nnz), tab


def _dev(csr, gpu):
    return csr.to(gpu)


# ------------------------------------------------------------ 1. staging

@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", [16, 32, 48, 64, 128])
def test_weighted_staging_is_exact(gpu, k, gather):
    csr, tab, s, e, rows = _case(k, gather)
    xcsr, xtab = _expanded(csr, rows, e, gather)
    A0, b0 = ops.gramian(_dev(xcsr, gpu), xtab.to(gpu), REG)
    zero = torch.zeros(k, k, device=gpu)
    A1, b1 = ops.gramian(_dev(csr, gpu), tab.to(gpu), REG, scale=s.to(gpu),
                         ext=e.to(gpu), base=zero)
    assert torch.equal(A1, A0)
    assert torch.equal(b1, b0)
    # a launch schedule only reorders blocks
    import flink_ms_amd._hip_ops as hip
    g = torch.Generator().manual_seed(k)
    order = torch.randperm(csr.num_rows, generator=g).to(torch.int32).to(gpu)
    A2 = torch.full_like(A1, float("nan"))
    b2 = torch.full_like(b1, float("nan"))
    d = _dev(csr, gpu)
    hip.gramian_w(d.indptr, d.indices, s.to(gpu), e.to(gpu), zero,
                  tab.to(gpu), A2, b2, order, REG,
                  torch.cuda.current_stream().cuda_stream)
    assert torch.equal(A2, A1) and torch.equal(b2, b1)


# --------------------------------------------------------------- 2. base

@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", [16, 64, 128])
def test_base_is_added_within_the_dot_bound(gpu, k, gather):
    csr, tab, s, e, rows = _case(k, gather)
    base = fx.random_base(k, seed=k)
    kw = dict(scale=s.to(gpu), ext=e.to(gpu))
    A0, b0 = ops.gramian(_dev(csr, gpu), tab.to(gpu), REG,
                         base=torch.zeros(k, k, device=gpu), **kw)
    A1, b1 = ops.gramian(_dev(csr, gpu), tab.to(gpu), REG,
                         base=base.to(gpu), **kw)
    assert torch.equal(b1, b0)
    # only the lower triangle of base may be read
    junk = torch.tril(base) + torch.triu(torch.full((k, k), 1e30), 1)
    A2, _ = ops.gramian(_dev(csr, gpu), tab.to(gpu), REG, base=junk.to(gpu),
                        **kw)
    assert torch.equal(A2, A1)
    n = csr.row_counts().double()
    rid = torch.repeat_interleave(torch.arange(csr.num_rows),
                                  csr.row_counts())
    absum = torch.zeros(csr.num_rows, k, k, dtype=torch.float64)
    r64 = rows.double().abs()
    absum.index_add_(0, rid, r64.unsqueeze(2) * r64.unsqueeze(1))
    bound = (2 * (n + 2) * U32).view(-1, 1, 1) * (base.double().abs() + absum)
    diff = (A1.cpu().double() - (A0.cpu().double() + base.double())).abs()
    print(f"k={k} {gather}: max diff {float(diff.max()):.3e}, "
          f"max diff/bound {float((diff / bound).max()):.3f}")
    assert bool((diff <= bound).all())


# ------------------------------------------------------- 3. fused solves

def _solve_gpu(gpu, csr, tab, s, e, base, k, row_order=None, fused=False):
    fp8 = tab.dtype == torch.uint8
    kp = (k + 15) // 16 * 16
    ob = None if fp8 else torch.full((csr.num_rows, kp), float("nan"),
                                     dtype=torch.bfloat16, device=gpu)
    o8 = (torch.full((csr.num_rows, kp), 0x7F, dtype=torch.uint8, device=gpu)
          if fp8 else None)
    x = ops.als_solve_side(_dev(csr, gpu), tab.to(gpu), REG, out_bf16=ob,
                           out_fp8=o8, row_order=row_order, fused=fused,
                           scale=s.to(gpu), ext=e.to(gpu), base=base.to(gpu))
    torch.cuda.synchronize()
    return x, (o8 if fp8 else ob)


def _check_solve(name, gpu, csr, tab, s, e, rows, base, k, fused):
    gather = R.gather_of(tab)
    x64 = R.als_solve_weighted_f64(csr, tab, REG, s, e, base)
    x32 = R.als_solve_weighted_reference(csr, tab, REG, s, e, base)
    cpu = float((x32.double() - x64).abs().max())
    factor = _factor(gather, "block" if fused else "wave")
    tol = factor * cpu + 4.0 * ULP32 * float(x64.abs().max())

    x, img = _solve_gpu(gpu, csr, tab, s, e, base, k, fused=fused)
    err = float((x.cpu().double() - x64).abs().max())

    # the yardstick's yardstick: the explicit kernel on the expanded table
    # of the base = 0 problem, against the same criterion
    zero = torch.zeros_like(base)
    z64 = R.als_solve_weighted_f64(csr, tab, REG, s, e, zero)
    z32 = R.als_solve_weighted_reference(csr, tab, REG, s, e, zero)
    zcpu = float((z32.double() - z64).abs().max())
    ztol = factor * zcpu + 4.0 * ULP32 * float(z64.abs().max())
    xz, _ = _solve_gpu(gpu, csr, tab, s, e, zero, k, fused=fused)
    if k % 16 == 0:
        xcsr, xtab = _expanded(csr, rows, e, gather)
        xe = ops.als_solve_side(_dev(xcsr, gpu), xtab.to(gpu), REG,
                                fused=fused)
        eerr = float((xe.cpu().double() - z64).abs().max())
        same = torch.equal(xe, xz)
    else:
        eerr, same = float("nan"), None
    zerr = float((xz.cpu().double() - z64).abs().max())
    print(f"{name}: weighted err {err:.3e} cpu-fp32 {cpu:.3e} tol {tol:.3e} "
          f"ratio {err / max(cpu, 1e-300):.2f} | base=0: weighted {zerr:.3e} "
          f"explicit {eerr:.3e} (ratio {eerr / max(zcpu, 1e-300):.1f}) "
          f"cpu-fp32 {zcpu:.3e} tol {ztol:.3e} "
          f"bit-equal to explicit: {same}")
    assert err <= tol, (name, err, tol)
    assert zerr <= ztol, (name, zerr, ztol)
    if same is not None:
        assert float((xe - xz).abs().max()) <= ztol

    # empty rows: zeros in the fp32 output and in the emitted image
    empty = (csr.row_counts() == 0).to(gpu)
    assert bool(empty.any())
    assert bool((x[empty] == 0).all())
    assert bool((img[empty].view(torch.uint8) == 0).all())
    # the image is the RNE image of the fp32 output
    kp = img.shape[1]
    xp = torch.zeros(csr.num_rows, kp, device=gpu)
    xp[:, :k] = x
    want = ops.quantize_fp8(xp) if gather == "fp8" else xp.to(torch.bfloat16)
    assert torch.equal(img.view(torch.uint8), want.view(torch.uint8))
    # deterministic, and a launch schedule permutes nothing but the order
    x2, img2 = _solve_gpu(gpu, csr, tab, s, e, base, k, fused=fused)
    assert torch.equal(x2, x) and torch.equal(img2.view(torch.uint8),
                                              img.view(torch.uint8))
    order = torch.randperm(
        csr.num_rows, generator=torch.Generator().manual_seed(k)
    ).to(torch.int32).to(gpu)
    x3, img3 = _solve_gpu(gpu, csr, tab, s, e, base, k, row_order=order,
                          fused=fused)
    assert torch.equal(x3, x) and torch.equal(img3.view(torch.uint8),
                                              img.view(torch.uint8))


@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", [16, 32, 48, 64])
def test_wavefused_weighted_solve(gpu, k, gather):
    csr, tab, s, e, rows = _case(k, gather)
    _check_solve(f"wave k={k} {gather}", gpu, csr, tab, s, e, rows,
                 fx.random_base(k, seed=k), k, fused=False)


def test_wavefused_weighted_solve_rank_10_padded(gpu):
    csr = fx.csr_with_row_lengths(fx.ROW_LENGTHS, NCOLS, seed=110)
    tab = fx.factor_table(NCOLS, 10, seed=210, gather="bf16")
    s, e = ops.implicit_weights(csr.values, ALPHA)
    rows, _ = R.effective_rows(csr, tab, s, e)
    _check_solve("wave k=10 bf16 (padded)", gpu, csr, tab, s, e, rows,
                 fx.random_base(10, seed=10), 10, fused=False)


@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", [80, 128])
def test_block_fused_weighted_solve(gpu, k, gather):
    csr, tab, s, e, rows = _case(k, gather)
    _check_solve(f"block k={k} {gather}", gpu, csr, tab, s, e, rows,
                 fx.random_base(k, seed=k), k, fused=True)


@pytest.mark.parametrize("gather", GATHERS)
def test_modular_weighted_path_matches_fused(gpu, gather):
    """gramian_w + the unchanged solvers (slab path) against the oracle."""
    k = 32
    csr, tab, s, e, rows = _case(k, gather)
    base = fx.random_base(k, seed=k)
    x64 = R.als_solve_weighted_f64(csr, tab, REG, s, e, base)
    x32 = R.als_solve_weighted_reference(csr, tab, REG, s, e, base)
    tol = (_factor(gather, "wave") * float((x32.double() - x64).abs().max())
           + 4.0 * ULP32 * float(x64.abs().max()))
    x = ops.als_solve_side(_dev(csr, gpu), tab.to(gpu), REG, slab_rows=4,
                           scale=s.to(gpu), ext=e.to(gpu), base=base.to(gpu))
    err = float((x.cpu().double() - x64).abs().max())
    print(f"modular k={k} {gather}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    assert bool((x[(csr.row_counts() == 0).to(gpu)] == 0).all())


# ---------------------------------------------------------- 4. factor Gram

@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", [16, 64, 128])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000])
def test_factor_gram(gpu, n, k, gather):
    tab = fx.factor_table(n, k, seed=300 + n + k, gather=gather)
    g64 = R.factor_gram_f64(tab)
    a = R._table_f32(tab).double().abs()
    absum = a.T @ a
    pad = torch.cat([tab, torch.zeros(40, k, dtype=tab.dtype)])
    for rpp in (None, 32, 96):
        per = rpp or ops.factor_gram_rows_per_part(n, k)
        parts = -(-n // per)
        G = ops.factor_gram(tab.to(gpu), rows_per_part=rpp)
        assert G.shape == (k, k) and G.dtype == torch.float32
        err = (G.cpu().double() - g64).abs()
        bound = 2 * (n + parts) * U32 * absum
        assert bool((err <= bound).all()), (n, k, gather, rpp,
                                            float((err / bound).max()))
        assert torch.equal(G, G.T)
        assert torch.equal(ops.factor_gram(tab.to(gpu), rows_per_part=rpp), G)
        # trailing all-zero rows (padded shards) change nothing
        assert torch.equal(
            ops.factor_gram(pad.to(gpu), rows_per_part=per), G)


def test_factor_gram_pads_odd_ranks(gpu):
    tab = fx.factor_table(77, 10, seed=5, gather="bf16")
    G = ops.factor_gram(tab.to(gpu))
    assert G.shape == (10, 10)
    g64 = R.factor_gram_f64(tab)
    a = tab.double().abs()
    assert bool(((G.cpu().double() - g64).abs()
                 <= 2 * (77 + 3) * U32 * (a.T @ a)).all())


# ------------------------------------------------------------ 5. end to end

NU, NI, RANK, ITERS, E2E_ALPHA, E2E_REG = 3000, 1000, 16, 5, 10.0, 0.1


def _train(device, u, i, r, **kw):
    cfg = ALSConfig(iterations=ITERS, num_factors=RANK, lambda_=E2E_REG,
                    implicit_prefs=True, alpha=E2E_ALPHA, **kw)
    tr = ALSTrainer(cfg)
    tr.ctx.device = device
    tr.setup(u.long(), i.long(), r, NU, NI)
    csr = fx.user_item_csr(u, i, r, NU, NI)
    objs = []
    for _ in range(ITERS):
        tr.step()
        m = tr.model()
        objs.append(R.implicit_objective(csr, m.user_factors.float().cpu(),
                                         m.item_factors.float().cpu(),
                                         E2E_ALPHA, E2E_REG))
    return objs, tr.model()


def test_end_to_end_planted_preferences(gpu):
    u, i, r = fx.planted_implicit(NU, NI, 20, 10, seed=77)
    cpu, _ = _train(torch.device("cpu"), u, i, r, dtype=torch.float32)
    bf16, _ = _train(gpu, u, i, r, dtype=torch.bfloat16)
    fp8, m8 = _train(gpu, u, i, r, factor_dtype="fp8")
    print(f"objective (full grid, float64) per iteration:\n  cpu fp32 {cpu}\n"
          f"  gpu bf16 {bf16}\n  gpu fp8  {fp8}\n"
          f"  bf16/cpu {bf16[-1] / cpu[-1]:.4f}  fp8/bf16 "
          f"{fp8[-1] / bf16[-1]:.4f}")
    assert bf16[-1] <= 1.10 * cpu[-1]
    assert bf16[-1] < bf16[0]
    assert all(v == v and v < float("inf") for v in fp8)
    assert torch.isfinite(m8.user_factors).all()
    assert torch.isfinite(m8.item_factors).all()
