"""Pure-PyTorch reference implementations of the hot ops.

Every HIP kernel in ``flink_ms_amd/ops/csrc/`` has a reference here computing
the same contract in plain fp32 torch.  These are (a) the numerics oracle for
the GPU parity tests and (b) the CPU execution path (this framework's tests
must run without a GPU).  The SVM and serving ops also have float64 oracles
(``*_f64``): the fp32 inputs are exact in float64, so they give the true
result of the contract, against which both the fp32 reference and the
kernels are measured.

Op contracts mirror the reference's hot loops:
- K1 Gramian assembly: per entity u, ``A_u = sum_{i in R(u)} q_i q_i^T
  + lambda * n_u * I``, ``b_u = sum r_ui q_i`` (flink-ml blocked ALS normal
  equations, driven by reference flink-als/.../ALSImpl.scala:52; weighted-
  lambda regularization).
- K2 batched Cholesky solve ``p_u = A_u^{-1} b_u``.
- K3 SDCA inner loop (flink-ml CoCoA localSDCA, driven by
  flink-svm/.../SVMImpl.scala:29): hinge-loss dual coordinate ascent.
- K4 online-SGD factor update (als-ms/.../qs/SGD.java:182-207).
- K5 prediction dots (flink-queryable-client/.../ALSPredict.java:74-83).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from ..data.blocked import CSR


# ------------------------------------------------------------------ K1 + K2

def gramian_reference(
    csr: CSR,
    factors: torch.Tensor,
    reg: float,
    chunk: int = 8192,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Assemble per-row normal equations.

    factors: [num_cols, k] (any float dtype; accumulated in fp32).
    Returns (A [num_rows, k, k] fp32 with ``reg * n_row * I`` folded in,
    b [num_rows, k] fp32).
    """
    k = factors.shape[1]
    n_rows = csr.num_rows
    dev = factors.device
    A = torch.zeros(n_rows, k, k, dtype=torch.float32, device=dev)
    b = torch.zeros(n_rows, k, dtype=torch.float32, device=dev)
    counts = csr.row_counts()
    row_ids = torch.repeat_interleave(
        torch.arange(n_rows, dtype=torch.int64, device=dev), counts
    )
    nnz = csr.nnz
    f32 = factors.to(torch.float32)
    for s in range(0, nnz, chunk):
        e = min(s + chunk, nnz)
        q = f32[csr.indices[s:e].long()]            # [c, k]
        r = csr.values[s:e].to(torch.float32)
        rid = row_ids[s:e]
        A.index_add_(0, rid, q.unsqueeze(2) * q.unsqueeze(1))
        b.index_add_(0, rid, q * r.unsqueeze(1))
    diag = torch.arange(k, device=dev)
    A[:, diag, diag] += reg * counts.to(torch.float32).unsqueeze(1)
    return A, b


def cholesky_solve_reference(A: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Batched SPD solve ``p = A^-1 b``; rows with singular A (no ratings and
    reg*0 diagonal) come back as zeros, matching the kernel contract."""
    k = A.shape[-1]
    diag = torch.arange(k, device=A.device)
    singular = A[:, diag, diag].abs().amax(dim=1) == 0
    A_safe = A.clone()
    A_safe[singular] = torch.eye(k, device=A.device, dtype=A.dtype)
    L = torch.linalg.cholesky(A_safe)
    p = torch.cholesky_solve(b.unsqueeze(2), L).squeeze(2)
    p[singular] = 0
    return p


def als_solve_side_reference(
    csr: CSR,
    other_factors: torch.Tensor,
    reg: float,
) -> torch.Tensor:
    """One ALS half-iteration (solve all entities of one side) in fp32."""
    A, b = gramian_reference(csr, other_factors, reg)
    return cholesky_solve_reference(A, b)


# ------------------------------------------- weighted K1 + K2 (implicit ALS)
#
# Contract of the weighted kernels (docs/KERNELS.md "Implicit feedback"):
# per stored entry j a scale s_j and an EXT value e_j, and one symmetric base
# matrix G0 [k][k]:
#   row~_j = round_D(s_j * F[indices[j]])        one fp32 multiply, RNE to D
#   A = G0 + sum_j row~_j row~_j^T + reg * n * I
#   b = sum_j pair_D(e_j) * row~_j               x = A^-1 b; n == 0 -> x = 0
# ``gather`` names D: 'fp8' (e4m3), 'bf16', or None (fp32 tables: nothing is
# rounded and pair_D is the identity).

E4M3_MAX = 448.0


def quantize_fp8(t: torch.Tensor) -> torch.Tensor:
    """fp32/bf16 -> OCP e4m3fn bytes (uint8) under the one contract of every
    e4m3 encoder of the project, the kernels' ``f2fp8`` included: round to
    nearest, ties to the even byte; finite values beyond +-448 SATURATE to
    +-448 (0x7E / 0xFE); inf and NaN become a NaN byte.  A plain torch cast
    differs above the range: it makes everything past 464 a NaN."""
    t = torch.where(torch.isfinite(t), t.clamp(-E4M3_MAX, E4M3_MAX), t)
    return t.to(torch.float8_e4m3fn).view(torch.uint8)


def _round_gather(t: torch.Tensor, gather: Optional[str]) -> torch.Tensor:
    if gather == "fp8":
        return quantize_fp8(t).view(torch.float8_e4m3fn).to(torch.float32)
    if gather == "bf16":
        return t.to(torch.bfloat16).to(torch.float32)
    if gather is None:
        return t
    raise ValueError(f"gather must be 'fp8', 'bf16' or None, got {gather!r}")


def rating_pair(r: torch.Tensor, gather: Optional[str]) -> torch.Tensor:
    """pair_D: the hi/lo EXT-column representation of ``r`` in the gather
    dtype, dequantized (hi = round_D(r), lo = round_D(r - hi))."""
    r = r.to(torch.float32)
    if gather is None:
        return r
    hi = _round_gather(r, gather)
    return hi + _round_gather(r - hi, gather)


def gather_of(factors: torch.Tensor) -> Optional[str]:
    """The gather dtype a factor table selects: uint8 = e4m3 bytes, bf16,
    anything else = unrounded fp32."""
    if factors.dtype == torch.uint8:
        return "fp8"
    if factors.dtype == torch.bfloat16:
        return "bf16"
    return None


def _table_f32(factors: torch.Tensor) -> torch.Tensor:
    if factors.dtype == torch.uint8:
        return factors.view(torch.float8_e4m3fn).to(torch.float32)
    return factors.to(torch.float32)


def effective_rows(csr: CSR, factors: torch.Tensor, scale: torch.Tensor,
                   ext: torch.Tensor, gather="auto",
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(row~ [nnz, k], pair_D(ext) [nnz]) in fp32: exactly the operands the
    weighted kernels feed their MFMAs, one row per stored entry."""
    if gather == "auto":
        gather = gather_of(factors)
    q = _table_f32(factors)[csr.indices.long()]
    rows = _round_gather(scale.to(torch.float32).unsqueeze(1) * q, gather)
    return rows, rating_pair(ext, gather)


def _weighted_systems(csr, factors, reg, scale, ext, base, gather, dtype,
                      chunk=8192):
    if gather == "auto":
        gather = gather_of(factors)
    k = factors.shape[1]
    n_rows = csr.num_rows
    dev = factors.device
    counts = csr.row_counts()
    A = base.to(dtype).unsqueeze(0).repeat(n_rows, 1, 1)
    b = torch.zeros(n_rows, k, dtype=dtype, device=dev)
    row_ids = torch.repeat_interleave(
        torch.arange(n_rows, dtype=torch.int64, device=dev), counts)
    f32 = _table_f32(factors)
    for s in range(0, csr.nnz, chunk):
        e = min(s + chunk, csr.nnz)
        q = _round_gather(
            scale[s:e].to(torch.float32).unsqueeze(1)
            * f32[csr.indices[s:e].long()], gather).to(dtype)
        r = rating_pair(ext[s:e], gather).to(dtype)
        rid = row_ids[s:e]
        A.index_add_(0, rid, q.unsqueeze(2) * q.unsqueeze(1))
        b.index_add_(0, rid, q * r.unsqueeze(1))
    diag = torch.arange(k, device=dev)
    A[:, diag, diag] += reg * counts.to(dtype).unsqueeze(1)
    return A, b, counts


def gramian_weighted_reference(csr: CSR, factors: torch.Tensor, reg: float,
                               scale: torch.Tensor, ext: torch.Tensor,
                               base: torch.Tensor, gather="auto",
                               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Weighted normal equations in fp32: (A [rows, k, k], b [rows, k])."""
    A, b, _ = _weighted_systems(csr, factors, reg, scale, ext, base, gather,
                                torch.float32)
    return A, b


def gramian_weighted_f64(csr: CSR, factors: torch.Tensor, reg: float,
                         scale: torch.Tensor, ext: torch.Tensor,
                         base: torch.Tensor, gather="auto",
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Float64 oracle of the weighted normal equations on the exact
    effective rows (row~ and pair_D(ext) are formed in fp32, as the contract
    says, and are exact in float64; everything after is float64)."""
    A, b, _ = _weighted_systems(csr, factors, reg, scale, ext, base, gather,
                                torch.float64)
    return A, b


def _solve_nonempty(A, b, counts):
    k = A.shape[-1]
    empty = counts == 0
    A = A.clone()
    A[empty] = torch.eye(k, dtype=A.dtype, device=A.device)
    x = torch.linalg.solve(A, b.unsqueeze(2)).squeeze(2)
    x[empty] = 0
    return x


def als_solve_weighted_reference(csr: CSR, factors: torch.Tensor, reg: float,
                                 scale: torch.Tensor, ext: torch.Tensor,
                                 base: torch.Tensor, gather="auto",
                                 ) -> torch.Tensor:
    """One weighted ALS half-iteration in fp32 (Cholesky); rows without
    stored entries come back as zeros."""
    A, b, counts = _weighted_systems(csr, factors, reg, scale, ext, base,
                                     gather, torch.float32)
    k = A.shape[-1]
    empty = counts == 0
    A[empty] = torch.eye(k, dtype=A.dtype, device=A.device)
    L = torch.linalg.cholesky(A)
    x = torch.cholesky_solve(b.unsqueeze(2), L).squeeze(2)
    x[empty] = 0
    return x


def als_solve_weighted_f64(csr: CSR, factors: torch.Tensor, reg: float,
                           scale: torch.Tensor, ext: torch.Tensor,
                           base: torch.Tensor, gather="auto") -> torch.Tensor:
    """Float64 oracle of the weighted solve on the exact effective rows."""
    A, b, counts = _weighted_systems(csr, factors, reg, scale, ext, base,
                                     gather, torch.float64)
    return _solve_nonempty(A, b, counts)


def factor_gram_reference(factors: torch.Tensor,
                          rows: Optional[torch.Tensor] = None
                          ) -> torch.Tensor:
    """G = F^T F in fp32 over every row of the table, or over the row list
    ``rows`` (repeats count once per occurrence)."""
    if rows is not None:
        factors = factors[rows.long()]
    f = _table_f32(factors)
    return f.T @ f


def factor_gram_f64(factors: torch.Tensor,
                    rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Float64 oracle of the factor Gram matrix (table entries are exact),
    over every row or over the row list ``rows``."""
    if rows is not None:
        factors = factors[rows.long()]
    f = _table_f32(factors).to(torch.float64)
    return f.T @ f


def implicit_weights_reference(values: torch.Tensor, alpha: float,
                               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scale, ext) of confidence-weighted ALS, in fp32 (Spark semantics:
    negative and zero stored values are legal):
      w = alpha * |r|,  s = sqrt(w),  e = (1 + w) / s if r > 0 else 0,
      w == 0 -> s = e = 0."""
    r = values.to(torch.float32)
    w = float(alpha) * r.abs()
    s = torch.sqrt(w)
    pos = (r > 0) & (w > 0)
    e = torch.where(pos, (1.0 + w) / torch.where(pos, s, torch.ones_like(s)),
                    torch.zeros_like(s))
    return s, e


def implicit_dense_f64(csr: CSR, Y: torch.Tensor, alpha: float,
                       reg: float) -> torch.Tensor:
    """Textbook dense Hu-Koren-Volinsky update, float64, for tiny problems:
    for every row u of ``csr`` (rows x all columns of Y)
      x_u = (Y^T C_u Y + reg * n_u * I)^-1 Y^T C_u p_u,
    c = 1 + alpha * |r| on stored entries and 1 elsewhere, p = [r > 0],
    n_u = stored entries of the row (rows without any give 0)."""
    Y = Y.to(torch.float64)
    m, k = Y.shape
    indptr = csr.indptr.tolist()
    out = torch.zeros(csr.num_rows, k, dtype=torch.float64)
    eye = torch.eye(k, dtype=torch.float64)
    for u in range(csr.num_rows):
        s, e = indptr[u], indptr[u + 1]
        if s == e:
            continue
        idx = csr.indices[s:e].long()        # one entry per (row, column)
        r = csr.values[s:e].to(torch.float64)
        c = torch.ones(m, dtype=torch.float64)
        c[idx] = 1.0 + float(alpha) * r.abs()
        p = torch.zeros(m, dtype=torch.float64)
        p[idx] = (r > 0).to(torch.float64)
        A = Y.T @ (c.unsqueeze(1) * Y) + reg * (e - s) * eye
        out[u] = torch.linalg.solve(A, Y.T @ (c * p))
    return out


def implicit_objective(csr: CSR, X: torch.Tensor, Y: torch.Tensor,
                       alpha: float, reg: float) -> float:
    """Confidence-weighted objective over the FULL rows x columns grid, in
    float64: sum c (p - x^T y)^2 + reg * (sum n_u |x_u|^2 + sum n_i |y_i|^2),
    c = 1 + alpha |r| and p = [r > 0] on the stored entries of ``csr`` (rows
    = X, columns = Y), c = 1 and p = 0 elsewhere; n = stored entries per row
    / per column.  The unobserved part is sum((X^T X) * (Y^T Y)), so the cost
    is O(nnz k + (rows + cols) k^2), not the grid's."""
    X = X.to(torch.float64).cpu()
    Y = Y.to(torch.float64).cpu()
    counts = csr.row_counts().cpu()
    rid = torch.repeat_interleave(torch.arange(csr.num_rows), counts)
    cid = csr.indices.long().cpu()
    r = csr.values.to(torch.float64).cpu()
    pred = (X[rid] * Y[cid]).sum(dim=1)
    w = float(alpha) * r.abs()
    p = (r > 0).to(torch.float64)
    # every grid cell at c = 1, p = 0, then the stored entries' correction
    total = ((X.T @ X) * (Y.T @ Y)).sum()
    total = total + ((1.0 + w) * (p - pred) ** 2 - pred ** 2).sum()
    ccount = torch.zeros(Y.shape[0], dtype=torch.float64)
    ccount.index_add_(0, cid, torch.ones_like(r))
    total = total + reg * ((counts.to(torch.float64)
                            * (X * X).sum(dim=1)[: csr.num_rows]).sum()
                           + (ccount * (Y * Y).sum(dim=1)).sum())
    return float(total)


# ---------------------------------------------------------------------- K3

def sdca_epoch_reference(
    csr: CSR,
    y: torch.Tensor,
    alpha: torch.Tensor,
    v: torch.Tensor,
    lamb: float,
    n_global: int,
    perm: Optional[torch.Tensor] = None,
) -> None:
    """One sequential SDCA pass over the local shard, in place.

    Hinge-loss dual coordinate ascent (Shalev-Shwartz & Zhang; the solver
    inside flink-ml's CoCoA localSDCA):
      for each sample i:  g = 1 - y_i <v, x_i>
                          dalpha = clip_[0,1](alpha_i + g * lamb * n / ||x||^2) - alpha_i
                          alpha_i += dalpha ; v += dalpha * y_i * x_i / (lamb * n)
    ``v`` is the local primal image (w + local delta); ``alpha`` the duals
    (stored pre-multiplied by y, in [0, 1]).
    """
    indptr = csr.indptr.tolist()
    idx = csr.indices.long()
    val = csr.values
    order = range(csr.num_rows) if perm is None else perm.tolist()
    scale = 1.0 / (lamb * n_global)
    for i in order:
        s, e = indptr[i], indptr[i + 1]
        if s == e:
            continue
        xi_idx = idx[s:e]
        xi_val = val[s:e]
        norm_sq = float((xi_val * xi_val).sum())
        if norm_sq == 0.0:
            continue
        yi = float(y[i])
        margin = yi * float((v[xi_idx] * xi_val).sum())
        grad = (1.0 - margin) / (norm_sq * scale)
        a_new = min(1.0, max(0.0, float(alpha[i]) + grad))
        dalpha = a_new - float(alpha[i])
        if dalpha != 0.0:
            alpha[i] = a_new
            # accumulate: a feature id repeated inside the row gets the SUM
            # of its updates (v += c * x_i), as the kernel's atomics give it
            v.index_add_(0, xi_idx, (dalpha * yi * scale) * xi_val)


def sdca_sequential_f64(
    csr: CSR,
    y: torch.Tensor,
    alpha: torch.Tensor,
    v: torch.Tensor,
    lamb: float,
    n_global: int,
    order=None,
    stale_reads: bool = False,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Float64 oracle of one SDCA pass over an explicit sample order.

    Same contract as :func:`sdca_epoch_reference`, every quantity in float64
    (the fp32 inputs are exact in it), accumulate semantics for repeated
    feature ids.  ``order`` is the sequence of sample ids to visit (default
    ``0..num_rows-1``).  Inputs are left alone; returns ``(alpha, v)`` as new
    float64 tensors.

    ``stale_reads=True`` is the deliberately WRONG variant in which every
    step computes its margin from the initial ``v`` (updates still
    accumulate): what a solver that never sees its own earlier updates would
    give.  Tests use it to show they can tell the two apart.
    """
    indptr = csr.indptr.tolist()
    idx = csr.indices.long().cpu()
    val = csr.values.to(torch.float64).cpu()
    y64 = y.to(torch.float64).cpu()
    a64 = alpha.to(torch.float64).cpu().clone()
    v64 = v.to(torch.float64).cpu().clone()
    v_read = v64.clone() if stale_reads else v64
    if order is None:
        order = range(csr.num_rows)
    elif isinstance(order, torch.Tensor):
        order = order.tolist()
    scale = 1.0 / (lamb * n_global)
    for i in order:
        s, e = indptr[i], indptr[i + 1]
        if s == e:
            continue
        xi_idx = idx[s:e]
        xi_val = val[s:e]
        norm_sq = float((xi_val * xi_val).sum())
        if norm_sq == 0.0:
            continue
        yi = float(y64[i])
        a_old = float(a64[i])
        margin = yi * float((v_read[xi_idx] * xi_val).sum())
        grad = (1.0 - margin) / (norm_sq * scale)
        a_new = min(1.0, max(0.0, a_old + grad))
        dalpha = a_new - a_old
        if dalpha != 0.0:
            a64[i] = a_new
            v64.index_add_(0, xi_idx, (dalpha * yi * scale) * xi_val)
    return a64, v64


def svm_margins_f64(csr: CSR, w: torch.Tensor) -> torch.Tensor:
    """Float64 oracle of the CSR decision values ``<w, x_i>``."""
    return svm_margins_reference(
        CSR(csr.indptr, csr.indices, csr.values.to(torch.float64),
            csr.num_rows, csr.num_cols),
        w.to(torch.float64))


def svm_margins_reference(csr: CSR, w: torch.Tensor) -> torch.Tensor:
    """Decision values ``<w, x_i>`` for every row of the CSR."""
    row_ids = torch.repeat_interleave(
        torch.arange(csr.num_rows, dtype=torch.int64, device=w.device),
        csr.row_counts(),
    )
    contrib = w[csr.indices.long()] * csr.values
    out = torch.zeros(csr.num_rows, dtype=w.dtype, device=w.device)
    out.index_add_(0, row_ids, contrib)
    return out


def hinge_objective(csr: CSR, y: torch.Tensor, w: torch.Tensor, lamb: float) -> float:
    """Primal SVM objective ``lamb/2 ||w||^2 + mean(hinge)``."""
    margins = svm_margins_reference(csr, w)
    hinge = torch.clamp(1.0 - y * margins, min=0.0)
    return float(0.5 * lamb * (w * w).sum() + hinge.mean())


# ---------------------------------------------------------------------- K4

def sgd_update_reference(
    p: torch.Tensor,
    q: torch.Tensor,
    r: torch.Tensor,
    lr: float,
    user_reg: float,
    item_reg: float,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Batched online-SGD factor update, v1 'simultaneous' semantics.

    Both updates are computed from the OLD copies (reference SGD.java:199-207
    — unlike SGDV0.java:188-197 which updates in place).  Returns
    (p_new, q_new, err).
    """
    err = r - (p * q).sum(dim=-1)
    e = err.unsqueeze(-1)
    p_new = p + lr * (e * q - user_reg * p)
    q_new = q + lr * (e * p - item_reg * q)
    return p_new, q_new, err


def sgd_update_f64(
    p: torch.Tensor,
    q: torch.Tensor,
    r: torch.Tensor,
    lr: float,
    user_reg: float,
    item_reg: float,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Float64 oracle of the v1 SGD update: ``(p_new, q_new, err)`` in
    float64 from the gathered old rows (bf16/fp32 inputs are exact in it)."""
    return sgd_update_reference(
        p.to(torch.float64), q.to(torch.float64), r.to(torch.float64),
        lr, user_reg, item_reg)


# ---------------------------------------------------------------------- K5

def predict_dot_f64(
    user_factors: torch.Tensor,
    item_factors: torch.Tensor,
    u_idx: torch.Tensor,
    i_idx: torch.Tensor,
) -> torch.Tensor:
    """Float64 oracle of the batched predictions ``dot(U[u], V[i])``."""
    p = user_factors[u_idx.long()].to(torch.float64)
    q = item_factors[i_idx.long()].to(torch.float64)
    return (p * q).sum(dim=-1)



def predict_dot_reference(
    user_factors: torch.Tensor,
    item_factors: torch.Tensor,
    u_idx: torch.Tensor,
    i_idx: torch.Tensor,
) -> torch.Tensor:
    """Batched ALS predictions ``dot(U[u], V[i])`` in fp32."""
    p = user_factors[u_idx.long()].to(torch.float32)
    q = item_factors[i_idx.long()].to(torch.float32)
    return (p * q).sum(dim=-1)


# ------------------------------------------------------------------ top-N

def _topk_scores(Q, V, topk, cand, exclude, dtype):
    nq = Q.shape[0]
    rows = (torch.arange(V.shape[0], dtype=torch.int64) if cand is None
            else cand.long().cpu())
    # candidates in ascending row order: every later sort is stable, so
    # equal scores keep it ("lower row of V first")
    rows = rows[torch.argsort(rows, stable=True)]
    S = Q.to(dtype).cpu() @ V.cpu()[rows].to(dtype).T          # [nq, nc]
    nan = torch.isnan(S)
    dead = torch.zeros_like(nan)
    if exclude is not None:
        ptr, ex = exclude
        ptr = ptr.long().cpu()
        ex = ex.long().cpu()
        for q in range(nq):
            dead[q] = torch.isin(rows, ex[int(ptr[q]):int(ptr[q + 1])])
    order = torch.sort(torch.where(nan, torch.full_like(S, -torch.inf), S),
                       dim=1, descending=True, stable=True).indices
    # numbers, then NaN scores, then excluded rows
    cls = (nan.to(torch.int8) + 2 * dead.to(torch.int8)).clamp_(max=2)
    order = order.gather(
        1, torch.sort(cls.gather(1, order), dim=1, stable=True).indices)
    out_s = torch.full((nq, topk), -torch.inf, dtype=dtype)
    out_r = torch.full((nq, topk), -1, dtype=torch.int64)
    n = min(topk, rows.numel())
    head = order[:, :n]
    live = ~dead.gather(1, head)
    out_s[:, :n] = torch.where(live, S.gather(1, head), out_s[:, :n])
    out_r[:, :n] = torch.where(live, rows[head], out_r[:, :n])
    return out_s, out_r


def topk_scores_reference(
    Q: torch.Tensor,
    V: torch.Tensor,
    topk: int,
    cand: Optional[torch.Tensor] = None,
    exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-N by ``score(q, r) = dot(Q[q], V[r])`` in fp32 over the rows
    ``cand`` of V (``None`` = all rows), without the rows
    ``excl_rows[excl_ptr[q]:excl_ptr[q+1]]`` of ``exclude = (excl_ptr,
    excl_rows)``.  Order: score descending, lower row first among equal
    scores, NaN scores after every number.  Returns (scores [nq, topk],
    rows int64 [nq, topk]); short results end in row -1 / score -inf."""
    return _topk_scores(Q, V, int(topk), cand, exclude, torch.float32)


def topk_scores_f64(
    Q: torch.Tensor,
    V: torch.Tensor,
    topk: int,
    cand: Optional[torch.Tensor] = None,
    exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Float64 oracle of :func:`topk_scores_reference` (same contract,
    scores in float64; bf16/fp32 inputs are exact in it)."""
    return _topk_scores(Q, V, int(topk), cand, exclude, torch.float64)


# ------------------------------------------------------------ rank counts

def _rank_counts(Q, V, q_idx, t_idx, cand, exclude, dtype, skip=None):
    # skip: the row not to count per pair (-1 = none) where that is not the
    # target row itself (targets appended to V as rows that are no candidates)
    Q, V = Q.cpu(), V.cpu()
    q_idx, t_idx = q_idx.long().cpu(), t_idx.long().cpu()
    skip = t_idx if skip is None else skip.long().cpu()
    P, nv = q_idx.numel(), V.shape[0]
    is_cand = torch.ones(nv, dtype=torch.bool)
    if cand is not None:
        is_cand = torch.zeros(nv, dtype=torch.bool)
        is_cand[cand.long().cpu()] = True
    if exclude is not None:
        ptr, ex = (t.long().cpu() for t in exclude)
    greater = torch.zeros(P, dtype=torch.int64)
    equal = torch.zeros(P, dtype=torch.int64)
    score = torch.zeros(P, dtype=dtype)
    Vd = V.to(dtype)
    step = max(1, (1 << 24) // nv)         # score blocks of <= 2^24 entries
    for s in range(0, P, step):
        qi, ti = q_idx[s:s + step], t_idx[s:s + step]
        b = qi.numel()
        # targets and candidates out of ONE product: equal vectors tie
        S = Q[qi].to(dtype) @ Vd.T                              # [b, nv]
        live = is_cand.expand(b, nv).clone()
        if exclude is not None:
            for j in range(b):
                q = int(qi[j])
                live[j, ex[int(ptr[q]):int(ptr[q + 1])]] = False
        live[torch.arange(b), ti] = False                       # the target
        sk = skip[s:s + b]
        live[torch.arange(b)[sk >= 0], sk[sk >= 0]] = False
        ts = S.gather(1, ti.unsqueeze(1))
        # the order word of topk_key: NaN below -inf and equal to NaN;
        # float comparison already has -0 == +0
        nan, tnan = torch.isnan(S), torch.isnan(ts)
        gt = ~nan & (tnan | (S > ts))
        eq = (nan & tnan) | (S == ts)
        greater[s:s + b] = (gt & live).sum(1)
        equal[s:s + b] = (eq & live).sum(1)
        score[s:s + b] = ts.squeeze(1)
    return greater, equal, score


def rank_counts_reference(
    Q: torch.Tensor,
    V: torch.Tensor,
    q_idx: torch.Tensor,
    t_idx: torch.Tensor,
    cand: Optional[torch.Tensor] = None,
    exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Where the target of each (query, target) pair ranks.  For pair ``p``
    with query ``Q[q_idx[p]]`` and target row ``t = t_idx[p]`` of V:
    ``score[p] = dot(Q[q_idx[p]], V[t])`` in fp32, and ``greater[p]`` /
    ``equal[p]`` count the rows ``r != t`` of ``cand`` (``None`` = all rows
    of V) outside ``excl_rows[excl_ptr[q]:excl_ptr[q+1]]``, ``q =
    q_idx[p]`` (``exclude = (excl_ptr [nq + 1], excl_rows)``, indexed by
    QUERY row), whose score is strictly above / equal to the target's.
    Scores compare as in :func:`topk_scores_reference`: NaN below every
    number and equal to NaN, -0 equal to +0; the row plays no part.  The
    target never counts, candidate or not, excluded or not.  Returns
    (greater int64 [P], equal int64 [P], score [P])."""
    return _rank_counts(Q, V, q_idx, t_idx, cand, exclude, torch.float32)


def rank_counts_f64(
    Q: torch.Tensor,
    V: torch.Tensor,
    q_idx: torch.Tensor,
    t_idx: torch.Tensor,
    cand: Optional[torch.Tensor] = None,
    exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Float64 oracle of :func:`rank_counts_reference` (same contract,
    scores in float64; bf16/fp32 inputs are exact in it)."""
    return _rank_counts(Q, V, q_idx, t_idx, cand, exclude, torch.float64)
