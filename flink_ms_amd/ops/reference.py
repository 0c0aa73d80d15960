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
