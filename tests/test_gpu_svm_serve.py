"""Exact-order parity tests for the SDCA, margins and serving kernels.

Every kernel result is compared with a float64 oracle of the same contract
(``flink_ms_amd.ops.reference.*_f64``) on the same fp32/bf16 inputs, which
are exact in float64.  Tolerances are derived, not picked:

- SDCA: the fp32 torch reference is run on the same inputs and its max abs
  distance from the float64 oracle is measured on the CPU.  The kernel gets
  4x that (a wave-tree sum and a sequential sum order the same fp32
  additions differently) plus a floor of 4 fp32 ulps (4 * 2^-23) of
  ``max|v|`` for ``v`` and of 1.0 (the top of alpha's range) for ``alpha``:
  one step is about eight fp32 roundings (1 - y*dot, nsq*scale, the divide,
  the add, the subtract, c, c*x and the atomic add) of half an ulp each,
  which the torch reference does not pay because it does its scalar math in
  Python floats.
- dots (margins, predict_dot, the SGD error): ``2 * n * 2^-24 * sum|terms|``
  per row, n the number of terms, from the data of that row.
- bf16 factor updates: within one bf16 ulp of the float64 result rounded to
  nearest-even, and at most 1 % of the elements different from it at all.

All SDCA cases use ``lambda * n`` that is a power of two, so the fp32
``scale`` the kernel receives is exact, and the SGD cases use a learning rate
and regularisers that are exact in fp32.
"""

import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.data.blocked import CSR
from flink_ms_amd.ops import reference as R

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24          # fp32 unit roundoff (half an ulp of 1.0)
ULP32 = 2.0 ** -23
# row lengths around the 64-lane wave and its second trip; rotated so that
# the 1-, 3- and 5-row cases still get a long, an empty and a tail row
ROW_LENS = [129, 0, 65, 200, 1, 63, 64, 127, 128]
KS = [1, 10, 16, 63, 64, 65, 100, 128]
LR, UREG, IREG = 0.125, 0.03125, 0.0625   # exact in fp32, user != item


# ------------------------------------------------------------------ helpers

def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4
                               else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _csr_from_rows(idx_rows, val_rows, num_cols):
    counts = torch.tensor([0] + [len(r) for r in idx_rows], dtype=torch.int64)
    empty_i = torch.zeros(0, dtype=torch.int32)
    empty_v = torch.zeros(0, dtype=torch.float32)
    return CSR(torch.cumsum(counts, 0),
               torch.cat([empty_i] + [r.to(torch.int32) for r in idx_rows]),
               torch.cat([empty_v] + [r.to(torch.float32) for r in val_rows]),
               len(idx_rows), num_cols)


def _sdca_yardstick(csr, y, alpha0, v0, lamb, n_global, order):
    """Float64 oracle, and the tolerances scaled from how far the fp32 torch
    reference lands from it on the same inputs (module docstring)."""
    a64, v64 = R.sdca_sequential_f64(csr, y, alpha0, v0, lamb, n_global, order)
    a32, v32 = alpha0.clone(), v0.clone()
    R.sdca_epoch_reference(csr, y, a32, v32, lamb, n_global, order)
    cpu_a = float((a32.double() - a64).abs().max())
    cpu_v = float((v32.double() - v64).abs().max())
    tol_a = 4.0 * cpu_a + 4.0 * ULP32
    tol_v = 4.0 * cpu_v + 4.0 * ULP32 * float(v64.abs().max())
    return a64, v64, cpu_a, cpu_v, tol_a, tol_v


def _check_sdca(name, a_g, v_g, yard):
    a64, v64, cpu_a, cpu_v, tol_a, tol_v = yard
    err_a = float((a_g.double() - a64).abs().max())
    err_v = float((v_g.double() - v64).abs().max())
    print(f"{name}: alpha err kernel {err_a:.3e} cpu-fp32 {cpu_a:.3e} "
          f"tol {tol_a:.3e} | v err kernel {err_v:.3e} cpu-fp32 {cpu_v:.3e} "
          f"tol {tol_v:.3e}")
    assert err_a <= tol_a, (name, err_a, tol_a)
    assert err_v <= tol_v, (name, err_v, tol_v)


def _gpu_sdca(gpu, csr, y, alpha0, v0, lamb, n_global, perm):
    a, v = alpha0.clone().to(gpu), v0.clone().to(gpu)
    ops.sdca_pass(csr.to(gpu), y.to(gpu), a, v, lamb, n_global,
                  perm=None if perm is None else perm.to(gpu))
    torch.cuda.synchronize()
    return a.cpu(), v.cpu()


# ----------------------------------------------- SDCA, conflict-free exact

def _disjoint_case(nrows, seed):
    """Samples with pairwise-disjoint feature supports: every schedule gives
    the same answer.  Row kinds rotate through ROW_LENS, an all-zero row and
    a row with repeated feature ids; alpha0 rotates through exactly 0,
    exactly 1 and interior."""
    g = torch.Generator().manual_seed(seed)
    kinds = ROW_LENS + ["zero", "dup"]
    lens = []
    for j in range(nrows):
        kd = kinds[j % len(kinds)]
        lens.append(5 if kd == "zero" else 70 if kd == "dup" else kd)
    total = sum(lens)
    num_cols = total + 64                      # 64+ features nobody touches
    ids = torch.randperm(num_cols, generator=g)[:total]
    idx_rows, val_rows = [], []
    pos = 0
    for j, n in enumerate(lens):
        kd = kinds[j % len(kinds)]
        idx = ids[pos:pos + n].clone()
        pos += n
        sign = torch.randint(0, 2, (n,), generator=g) * 2.0 - 1.0
        val = (0.5 + torch.rand(n, generator=g)) * sign
        # ||x||^2 about 0.5 (scale is 2): mean of (0.5 + U)^2 is 13/12
        val = val * (0.5 / (13.0 / 12.0) / max(n, 1)) ** 0.5
        if kd == "zero":
            val = torch.zeros(n)
        if kd == "dup":
            idx[69] = idx[5]     # one copy in the first 64, one in the tail
            idx[20] = idx[7]     # both copies in the first 64
        idx_rows.append(idx)
        val_rows.append(val)
    csr = _csr_from_rows(idx_rows, val_rows, num_cols)
    y = torch.randint(0, 2, (nrows,), generator=g) * 2.0 - 1.0
    interior = 0.1 + 0.8 * torch.rand(nrows, generator=g)
    kind_a = torch.arange(nrows) % 3
    alpha0 = torch.where(kind_a == 0, torch.zeros(nrows),
                         torch.where(kind_a == 1, torch.ones(nrows), interior))
    v0 = torch.randn(num_cols, generator=g) * 1.5
    touched = torch.zeros(num_cols, dtype=torch.bool)
    touched[csr.indices.long()] = True
    structural_skip = torch.tensor(
        [n == 0 or kinds[j % len(kinds)] == "zero"
         for j, n in enumerate(lens)])
    return csr, y, alpha0, v0, touched, structural_skip


@pytest.mark.parametrize("with_perm", [False, True])
@pytest.mark.parametrize("nrows", [1, 3, 5, 67, 300])
def test_sdca_conflict_free_matches_f64(gpu, nrows, with_perm):
    lamb, n_global = 2.0 ** -11, 1024          # scale = 2, n_global != nrows
    csr, y, alpha0, v0, touched, skip = _disjoint_case(nrows, seed=100)
    g = torch.Generator().manual_seed(7 + nrows)
    perm = (torch.randperm(nrows, generator=g).to(torch.int32)
            if with_perm else None)
    yard = _sdca_yardstick(csr, y, alpha0, v0, lamb, n_global, perm)
    a64, v64 = yard[0], yard[1]

    # what the data must exercise (decided on the float64 oracle)
    scale = 1.0 / (lamb * n_global)
    a0 = alpha0.double()
    rows = torch.repeat_interleave(torch.arange(nrows), csr.row_counts())
    nsq = torch.zeros(nrows, dtype=torch.float64).index_add_(
        0, rows, csr.values.double() ** 2)
    live = ~skip
    marg = y.double() * R.svm_margins_f64(csr, v0)
    step = torch.zeros(nrows, dtype=torch.float64)
    step[live] = (1.0 - marg[live]) / (nsq[live] * scale)
    raw = a0 + step
    # no-write rows: already at the bound the step pushes against, with the
    # unclipped value clear of it by far more than any rounding
    no_write = live & (((a0 == 0) & (raw < -1e-3))
                       | ((a0 == 1) & (raw > 1 + 1e-3)))
    if nrows >= 67:
        assert (live & (a0 > 0) & (a64 == 0)).any()       # clipped low
        assert (live & (a0 < 1) & (a64 == 1)).any()       # clipped high
        assert (live & (a64 > 0) & (a64 < 1) & (a64 != a0)).any()
        assert (no_write & (a0 == 0)).any() and (no_write & (a0 == 1)).any()
        assert skip.sum() >= 2

    a_g, v_g = _gpu_sdca(gpu, csr, y, alpha0, v0, lamb, n_global, perm)
    _check_sdca(f"conflict-free nrows={nrows} perm={with_perm}", a_g, v_g, yard)
    assert _same_bits(v_g[~touched], v0[~touched])
    frozen = skip | no_write
    assert _same_bits(a_g[frozen], alpha0[frozen])
    # rows that must not write leave their features alone too
    quiet = csr.indices.long()[frozen[rows]]
    assert _same_bits(v_g[quiet], v0[quiet])


# ------------------------------------------ SDCA, staged sequential order

def test_sdca_staged_launches_match_sequential_f64(gpu):
    """Samples share features across stages; each stage (one launch over a
    contiguous row range) is internally feature-disjoint, so the result is
    the float64 sequential pass in stage order: a later launch must read
    what the earlier ones wrote."""
    stages, per, group, pick = 4, 40, 12, 8
    ncols = per * group
    nrows = stages * per
    lamb, n_global = 2.0 ** -9, 256            # scale = 2
    g = torch.Generator().manual_seed(31)
    idx_rows, val_rows = [], []
    for _ in range(stages):
        feats = torch.randperm(ncols, generator=g)
        for r in range(per):
            mine = feats[r * group:(r + 1) * group]
            idx_rows.append(mine[torch.randperm(group, generator=g)[:pick]])
            sign = torch.randint(0, 2, (pick,), generator=g) * 2.0 - 1.0
            val_rows.append((0.5 + torch.rand(pick, generator=g)) * sign
                            * (0.5 / (13.0 / 12.0) / pick) ** 0.5)
    csr = _csr_from_rows(idx_rows, val_rows, ncols)
    y = torch.randint(0, 2, (nrows,), generator=g) * 2.0 - 1.0
    alpha0 = torch.rand(nrows, generator=g)
    alpha0[::5] = 0.0
    alpha0[1::5] = 1.0
    v0 = torch.randn(ncols, generator=g) * 0.5
    yard = _sdca_yardstick(csr, y, alpha0, v0, lamb, n_global, None)
    # the stages really interact: one pass over everything from the initial
    # v (no read-after-update at all) is far from the sequential answer
    _, v_stale = R.sdca_sequential_f64(csr, y, alpha0, v0, lamb, n_global,
                                       stale_reads=True)
    assert float((v_stale - yard[1]).abs().max()) > 100 * yard[5]

    raw = ops._require_hip()
    csr_g = csr.to(gpu)
    y_g, a_g, v_g = y.to(gpu), alpha0.clone().to(gpu), v0.clone().to(gpu)
    nsq_g = ops.csr_row_norms_sq(csr_g)
    no_perm = torch.empty(0, device=gpu)
    for s in range(stages):
        a, b = s * per, (s + 1) * per
        raw.sdca_pass(csr_g.indptr[a:b + 1], csr_g.indices, csr_g.values,
                      y_g[a:b], nsq_g[a:b], no_perm, a_g[a:b], v_g,
                      1.0 / (lamb * n_global),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check_sdca("staged", a_g.cpu(), v_g.cpu(), yard)


# ------------------------------------------- SDCA, same-wave freshness (K3)

@pytest.mark.parametrize("with_perm", [False, True])
@pytest.mark.parametrize("nrows", [48, 1040])
def test_sdca_wave_sees_its_own_updates(gpu, nrows, with_perm):
    """docs/KERNELS.md K3: a wave walks its samples sequentially and sees its
    own earlier updates of v.  Schedule position p uses features private to
    class p mod W (W = launched waves), so each wave runs a chain of steps on
    addresses no other wave touches, and the exact answer is the float64
    sequential pass in schedule order.  nrows = 48 is 12 * W for the minimum
    W = 4 (one block); nrows = 1040 spreads 68 waves over 17 blocks."""
    W = ops.sdca_num_waves(nrows)
    if nrows == 48:
        assert W == 4 and ops.sdca_num_waves(12 * W) == W
    assert W % 4 == 0 and nrows // W >= 12
    pool, pick = 8, 5
    lamb, n_global = 2.0 ** -11, 4096          # scale = 0.5, ||x||^2 ~ 5.4
    g = torch.Generator().manual_seed(500 + nrows)
    perm = (torch.randperm(nrows, generator=g).to(torch.int32)
            if with_perm else torch.arange(nrows, dtype=torch.int32))
    idx_rows = [None] * nrows
    val_rows = [None] * nrows
    for p in range(nrows):
        c = p % W
        feats = c * pool + torch.randperm(pool, generator=g)[:pick]
        sign = torch.randint(0, 2, (pick,), generator=g) * 2.0 - 1.0
        idx_rows[int(perm[p])] = feats
        val_rows[int(perm[p])] = (0.5 + torch.rand(pick, generator=g)) * sign
    csr = _csr_from_rows(idx_rows, val_rows, W * pool)
    y = torch.randint(0, 2, (nrows,), generator=g) * 2.0 - 1.0
    alpha0 = torch.zeros(nrows)
    v0 = torch.zeros(W * pool)
    yard = _sdca_yardstick(csr, y, alpha0, v0, lamb, n_global, perm)
    a64, v64, _, _, tol_a, tol_v = yard
    # a solver whose steps read the v of the start of the pass (stale reads)
    # lands orders of magnitude outside the tolerance: the test can tell
    a_st, v_st = R.sdca_sequential_f64(csr, y, alpha0, v0, lamb, n_global,
                                       perm, stale_reads=True)
    gap_a = float((a_st - a64).abs().max())
    gap_v = float((v_st - v64).abs().max())
    print(f"freshness nrows={nrows} W={W}: stale-vs-sequential gap "
          f"alpha {gap_a:.3e} v {gap_v:.3e}")
    assert gap_a > 100 * tol_a and gap_v > 100 * tol_v

    a_g, v_g = _gpu_sdca(gpu, csr, y, alpha0, v0, lamb, n_global,
                         perm if with_perm else None)
    _check_sdca(f"freshness nrows={nrows} W={W} perm={with_perm}",
                a_g, v_g, yard)


# ------------------------------------------------------------------ margins

def _check_margins(name, gpu, csr, w):
    m64 = R.svm_margins_f64(csr, w)
    mag = R.svm_margins_f64(
        CSR(csr.indptr, csr.indices, csr.values.abs(), csr.num_rows,
            csr.num_cols), w.abs())
    bound = 2.0 * csr.row_counts().double() * U32 * mag
    m_g = ops.svm_margins(csr.to(gpu), w.to(gpu))
    torch.cuda.synchronize()
    m_g = m_g.cpu()
    err = (m_g.double() - m64).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max err {float(err.max()):.3e}, worst err/bound "
          f"{worst:.3f}")
    assert (err <= bound).all(), (name, worst)
    empty = csr.row_counts() == 0
    assert _same_bits(m_g[empty], torch.zeros(int(empty.sum())))
    return m_g


def test_svm_margins_row_lengths_match_f64(gpu):
    g = torch.Generator().manual_seed(41)
    ncols = 500
    idx_rows, val_rows = [], []
    for n in ROW_LENS * 3 + [70]:
        idx = torch.randint(0, ncols, (n,), generator=g)   # with replacement
        if n == 70:
            idx[69] = idx[5]
        idx_rows.append(idx)
        val_rows.append(torch.randn(n, generator=g))
    csr = _csr_from_rows(idx_rows, val_rows, ncols)
    w = torch.randn(ncols, generator=g)
    _check_margins("margins row lengths", gpu, csr, w)


def test_svm_margins_grid_stride_matches_f64(gpu):
    """8200 rows need 2050 blocks of four waves, above the 2048-block grid
    cap: the last rows are served by the grid-stride trip."""
    g = torch.Generator().manual_seed(42)
    nrows, ncols = 8200, 300
    counts = torch.randint(1, 4, (nrows,), generator=g)
    nnz = int(counts.sum())
    indptr = torch.zeros(nrows + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(counts, 0)
    csr = CSR(indptr,
              torch.randint(0, ncols, (nnz,), generator=g).to(torch.int32),
              torch.randn(nnz, generator=g), nrows, ncols)
    w = torch.randn(ncols, generator=g)
    _check_margins("margins grid stride", gpu, csr, w)


# -------------------------------------------------------------- predict_dot

def _edge_indices(nq, n, g, first_last):
    """Repeated indices that include the table's first and last rows."""
    idx = torch.randint(0, n, (nq,), generator=g)
    edges = [0, n - 1] if first_last else [n - 1, 0]
    for j in range(min(nq, 4)):
        idx[j] = edges[j % 2]
    idx[nq - 1] = edges[1] if nq > 1 else edges[0]
    return idx


@pytest.mark.parametrize("nq", [1, 5, 8200])
@pytest.mark.parametrize("k", KS)
def test_predict_dot_matches_f64(gpu, k, nq):
    g = torch.Generator().manual_seed(1000 * k + nq)
    nu, ni = 37, 29
    U = torch.randn(nu, k, generator=g).to(torch.bfloat16)
    V = torch.randn(ni, k, generator=g).to(torch.bfloat16)
    u = _edge_indices(nq, nu, g, True)
    i = _edge_indices(nq, ni, g, False)
    d64 = R.predict_dot_f64(U, V, u, i)
    bound = 2.0 * k * U32 * (U[u].double() * V[i].double()).abs().sum(-1)
    out = ops.predict_dot(U.to(gpu), V.to(gpu), u.to(gpu), i.to(gpu))
    torch.cuda.synchronize()
    err = (out.cpu().double() - d64).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"predict_dot k={k} nq={nq}: max err {float(err.max()):.3e}, "
          f"worst err/bound {worst:.3f}")
    assert (err <= bound).all(), worst


def test_predict_dot_rejects_rank_above_128(gpu):
    U = torch.zeros(4, 129, dtype=torch.bfloat16, device=gpu)
    idx = torch.zeros(2, dtype=torch.int64, device=gpu)
    with pytest.raises(RuntimeError):
        ops.predict_dot(U, U.clone(), idx, idx)
    torch.cuda.synchronize()


# --------------------------------------------------------------- sgd_update

def _rne_bf16(x64):
    """float64 -> bf16, one round-to-nearest-even (no detour through fp32)."""
    m, e = torch.frexp(x64)
    return torch.ldexp(torch.round(m * 256.0), e - 8).to(torch.bfloat16)


def _bf16_ordinal(t):
    """bf16 -> integer that counts representable values in order, so that
    neighbours differ by one (both zeros map to 0)."""
    b = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b < 0x8000, b, 0x8000 - b)


def _sgd_case(k, nq, seed):
    g = torch.Generator().manual_seed(seed)
    nu, ni = nq + 3, nq + 5
    U = (torch.randn(nu, k, generator=g) * 0.3).to(torch.bfloat16)
    V = (torch.randn(ni, k, generator=g) * 0.3).to(torch.bfloat16)
    u = torch.randperm(nu, generator=g)[:nq]       # no in-batch collisions
    i = torch.randperm(ni, generator=g)[:nq]
    r = torch.rand(nq, generator=g) * 4.5 + 0.5
    return U, V, u, i, r


def _bf16_mismatch(got, want):
    d = (_bf16_ordinal(got) - _bf16_ordinal(want)).abs()
    return int(d.max()), float((d != 0).double().mean())


def _check_sgd(name, U, V, u, i, r, U_g, V_g, err_g):
    """U_g, V_g, err_g: CPU copies of what the kernel left."""
    p, q = U[u], V[i]
    pn64, qn64, err64 = R.sgd_update_f64(p, q, r, LR, UREG, IREG)
    k = U.shape[1]
    # err = r - sum p_c q_c is a sum of k + 1 terms
    bound = 2.0 * (k + 1) * U32 * (
        r.double().abs() + (p.double() * q.double()).abs().sum(-1))
    e = (err_g.double() - err64).abs()
    assert (e <= bound).all(), (name, float((e / bound).max()))
    want = torch.cat([_rne_bf16(pn64), _rne_bf16(qn64)])
    # the cap below is only fair if plain fp32 arithmetic meets it here
    pn32, qn32, _ = R.sgd_update_reference(p.float(), q.float(), r,
                                           LR, UREG, IREG)
    cpu_max, cpu_share = _bf16_mismatch(
        torch.cat([pn32, qn32]).to(torch.bfloat16), want)
    assert cpu_max <= 1 and cpu_share <= 0.01, (name, cpu_max, cpu_share)
    got_max, got_share = _bf16_mismatch(torch.cat([U_g[u], V_g[i]]), want)
    print(f"{name}: err worst err/bound {float((e / bound).max()):.3f}; "
          f"bf16 elements off RNE(f64): kernel {got_share:.5%} (max "
          f"{got_max} ulp), cpu-fp32 {cpu_share:.5%}")
    assert got_max <= 1, name
    assert got_share <= 0.01, (name, got_share)
    # rows not named in the batch are bit-unchanged
    ku = torch.ones(U.shape[0], dtype=torch.bool)
    ku[u] = False
    kv = torch.ones(V.shape[0], dtype=torch.bool)
    kv[i] = False
    assert _same_bits(U_g[ku], U[ku]) and _same_bits(V_g[kv], V[kv])


def _gpu_sgd(gpu, U, V, u, i, r):
    Ug, Vg = U.clone().to(gpu), V.clone().to(gpu)
    err = ops.sgd_update(Ug, Vg, u.to(gpu), i.to(gpu), r.to(gpu),
                         LR, UREG, IREG)
    torch.cuda.synchronize()
    return Ug.cpu(), Vg.cpu(), err.cpu()


@pytest.mark.parametrize("k", KS)
def test_sgd_update_matches_f64(gpu, k):
    U, V, u, i, r = _sgd_case(k, 300, seed=2000 + k)
    _check_sgd(f"sgd_update k={k}", U, V, u, i, r, *_gpu_sgd(gpu, U, V, u, i, r))


def test_sgd_update_grid_stride_matches_f64(gpu):
    """8200 queries exceed the 2048-block grid cap (four per block)."""
    U, V, u, i, r = _sgd_case(10, 8200, seed=2999)
    _check_sgd("sgd_update nq=8200", U, V, u, i, r,
               *_gpu_sgd(gpu, U, V, u, i, r))


@pytest.mark.parametrize("k", [10, 100])
def test_sgd_update_same_tensor_for_users_and_items(gpu, k):
    """The serving store passes one mirror tensor as both U and V, users and
    items in disjoint rows: same bits as with two tensors."""
    U, V, u, i, r = _sgd_case(k, 300, seed=2500 + k)
    U2, V2, err2 = _gpu_sgd(gpu, U, V, u, i, r)
    nu = U.shape[0]
    M = torch.cat([U, V]).to(gpu)
    err1 = ops.sgd_update(M, M, u.to(gpu), (i + nu).to(gpu), r.to(gpu),
                          LR, UREG, IREG)
    torch.cuda.synchronize()
    M = M.cpu()
    assert _same_bits(M[:nu], U2) and _same_bits(M[nu:], V2)
    assert _same_bits(err1.cpu(), err2)
    _check_sgd(f"sgd_update mirror k={k}", U, V, u, i, r, M[:nu], M[nu:],
               err1.cpu())


def _with_row_restored(T_g, T, row):
    """The kernel's table with one (separately checked) row put back."""
    out = T_g.clone()
    out[row] = T[row]
    return out


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("kind", ["inf", "nan", "payload_nan"])
def test_sgd_update_non_finite_rating(gpu, kind, k):
    """NaN in, NaN out on every touched element (never a finite value or a
    signed zero); inf as torch's bf16 cast gives it; neighbours unharmed."""
    U, V, u, i, r = _sgd_case(k, 3, seed=2700 + k)
    special = {
        "inf": torch.tensor([float("inf")]),
        "nan": torch.tensor([float("nan")]),
        "payload_nan": torch.tensor([0x7FFFFFFF],
                                    dtype=torch.int32).view(torch.float32),
    }[kind]
    r[1] = special[0]
    assert _same_bits(r[1:2], special)
    U_g, V_g, err_g = _gpu_sgd(gpu, U, V, u, i, r)
    pn32, qn32, err32 = R.sgd_update_reference(U[u].float(), V[i].float(), r,
                                               LR, UREG, IREG)
    want = torch.cat([pn32[1], qn32[1]]).to(torch.bfloat16)
    got = torch.cat([U_g[u[1]], V_g[i[1]]])
    if kind == "inf":
        assert torch.isinf(err_g[1]) and err_g[1] > 0
        assert torch.isinf(want).all()           # factors are non-zero
        assert _same_bits(got, want)
    else:
        assert torch.isnan(err_g[1])
        assert torch.isnan(want).all()
        assert torch.isnan(got).all(), got
    # the finite queries of the same batch are as exact as ever
    keep = torch.tensor([0, 2])
    _check_sgd(f"sgd_update {kind} neighbours k={k}", U, V, u[keep], i[keep],
               r[keep], _with_row_restored(U_g, U, u[1]),
               _with_row_restored(V_g, V, i[1]), err_g[keep])


# ---------------------------------------------------- binding size checks
#
# Short tensors are views into full-size buffers, so nothing here could touch
# memory outside an allocation even if a check were missing.

def _sdca_args(gpu):
    csr, y, alpha0, v0, _, _ = _disjoint_case(5, seed=9)
    csr = csr.to(gpu)
    n = csr.num_rows
    return dict(
        indptr=csr.indptr, indices=csr.indices, values=csr.values,
        y=y.to(gpu), norms_sq=ops.csr_row_norms_sq(csr),
        perm=torch.arange(n + 1, dtype=torch.int32, device=gpu) % n,
        alpha=alpha0.to(gpu), v=v0.to(gpu)), n


def _call_sdca(a):
    ops._require_hip().sdca_pass(
        a["indptr"], a["indices"], a["values"], a["y"], a["norms_sq"],
        a["perm"], a["alpha"], a["v"], 2.0,
        torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("short", ["y", "norms_sq", "alpha", "perm_short",
                                   "perm_long", "values"])
def test_sdca_pass_rejects_wrong_sizes(gpu, short):
    a, n = _sdca_args(gpu)
    alpha, v = a["alpha"], a["v"]
    alpha0, v0 = alpha.clone(), v.clone()
    if short == "perm_short":
        a["perm"] = a["perm"][:n - 1]
    elif short == "perm_long":
        pass                                   # n + 1 entries as built
    else:
        a["perm"] = a["perm"][:n]
        a[short] = a[short][:a[short].numel() - 1]
    with pytest.raises(RuntimeError):
        _call_sdca(a)
    torch.cuda.synchronize()
    assert _same_bits(alpha.cpu(), alpha0.cpu())
    assert _same_bits(v.cpu(), v0.cpu())


def test_svm_margins_rejects_short_out(gpu):
    a, n = _sdca_args(gpu)
    out = torch.zeros(n, device=gpu)
    with pytest.raises(RuntimeError):
        ops._require_hip().svm_margins(
            a["indptr"], a["indices"], a["values"], a["v"], out[:n - 1],
            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (out == 0).all()


@pytest.mark.parametrize("short", ["i_idx", "out"])
def test_predict_dot_rejects_wrong_sizes(gpu, short):
    U = torch.ones(6, 10, dtype=torch.bfloat16, device=gpu)
    a = dict(u_idx=torch.zeros(4, dtype=torch.int64, device=gpu),
             i_idx=torch.zeros(4, dtype=torch.int64, device=gpu),
             out=torch.zeros(4, device=gpu))
    full_out = a["out"]
    a[short] = a[short][:3]
    with pytest.raises(RuntimeError):
        ops._require_hip().predict_dot(
            U, U.clone(), a["u_idx"], a["i_idx"], a["out"],
            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (full_out == 0).all()


@pytest.mark.parametrize("short", ["i_idx", "r", "err_out", "rank"])
def test_sgd_update_rejects_wrong_sizes(gpu, short):
    U = torch.ones(6, 10, dtype=torch.bfloat16, device=gpu)
    V = torch.ones(6, 11 if short == "rank" else 10, dtype=torch.bfloat16,
                   device=gpu)
    a = dict(u_idx=torch.arange(4, dtype=torch.int64, device=gpu),
             i_idx=torch.arange(4, dtype=torch.int64, device=gpu),
             r=torch.ones(4, device=gpu), err_out=torch.zeros(4, device=gpu))
    if short != "rank":
        a[short] = a[short][:3]
    with pytest.raises(RuntimeError):
        ops._require_hip().sgd_update(
            U, V, a["u_idx"], a["i_idx"], a["r"], a["err_out"], LR, UREG,
            IREG, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (U == 1).all() and (V == 1).all()
