"""Op dispatch: HIP kernels on GPU, torch reference on CPU.

On a GPU box the HIP extension (``flink_ms_amd/_hip_ops.so``, built in-tree
by ``flink_ms_amd.ops.build``) is REQUIRED: a missing extension raises
instead of silently falling back to eager torch, so benchmarks and GPU tests
always exercise the native path.  On CPU-only machines the pure-torch
reference implementations (``flink_ms_amd.ops.reference``) run instead.
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from ..data.blocked import CSR
from . import reference

_hip_ops = None
_hip_import_error: Optional[BaseException] = None
try:
    from flink_ms_amd import _hip_ops  # type: ignore[no-redef]
except BaseException as e:  # pragma: no cover - exercised on unbuilt trees
    _hip_import_error = e


def hip_available() -> bool:
    return _hip_ops is not None


def _require_hip():
    if _hip_ops is None:
        raise RuntimeError(
            "flink_ms_amd HIP extension is not built but a GPU tensor was "
            "passed; run `python -m flink_ms_amd.ops.build` "
            f"(import error: {_hip_import_error!r})"
        )
    return _hip_ops


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _pad_k(t: torch.Tensor) -> torch.Tensor:
    """Pad factor columns to the next multiple of 16 (kernel tile width)."""
    k = t.shape[1]
    kp = ((k + 15) // 16) * 16
    if kp == k:
        return t
    out = torch.zeros(t.shape[0], kp, dtype=t.dtype, device=t.device)
    out[:, :k] = t
    return out


_EMPTY = {}


def _empty(device) -> torch.Tensor:
    key = str(device)
    if key not in _EMPTY:
        _EMPTY[key] = torch.empty(0, device=device)
    return _EMPTY[key]


# ------------------------------------------------------------- fp8 e4m3

def quantize_fp8(t: torch.Tensor) -> torch.Tensor:
    """fp32/bf16 -> OCP e4m3fn bytes (uint8).  The byte image is what the
    fp8 Gramian kernels gather (one cache line per k<=64 factor row) and
    what the factor exchange ships over xGMI (half the bf16 bytes).

    The contract of the kernels' ``f2fp8``, on the host too: round to
    nearest, ties to the even byte; finite values beyond +-448 saturate to
    +-448; inf and NaN become a NaN byte.  (A plain torch cast turns
    everything above 464 into NaN, which would poison every entity that
    gathers the value.)"""
    return reference.quantize_fp8(t)


def dequantize_fp8(t: torch.Tensor) -> torch.Tensor:
    """uint8 e4m3 bytes -> fp32 (exact: every e4m3 value is a float)."""
    return t.view(torch.float8_e4m3fn).to(torch.float32)


def fp8_rating_pair(r: torch.Tensor) -> torch.Tensor:
    """The EXT-column rating representation of the fp8 Gramian: e4m3 hi/lo
    pair with r ~= hi + lo (max relative error ~1.9e-3, see
    benchmarks/fp8_convergence_study.py).  Returns the dequantized
    effective rating, for CPU references that must match the kernel: both
    halves go through :func:`quantize_fp8`, so a finite rating beyond the
    e4m3 range saturates (hi = +-448, lo = the saturated rest) exactly as
    the kernels' staging does; inf and NaN give NaN."""
    return reference.rating_pair(r, "fp8")


def bf16_rating_pair(r: torch.Tensor) -> torch.Tensor:
    """The bf16 twin of :func:`fp8_rating_pair`: the bf16 hi/lo EXT pair of
    the bf16 Gramian, dequantized (relative error ~2^-17)."""
    return reference.rating_pair(r, "bf16")


# -------------------------------------------------------------------- ALS

def implicit_weights(values: torch.Tensor, alpha: float
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-entry ``(scale, ext)`` of confidence-weighted (implicit-feedback)
    ALS for the weighted solves, computed once at setup in fp32 torch:
    ``w = alpha*|r|``, ``scale = sqrt(w)``, ``ext = (1 + w) / scale`` where
    ``r > 0`` else 0 (``w == 0`` gives 0, 0).  With ``base`` = the Gram
    matrix of ALL opposite-side factors this makes the weighted solve the
    Hu-Koren-Volinsky update.  Kernels and references both take the two
    tensors as given: no square root is ever taken in a kernel."""
    return reference.implicit_weights_reference(values, alpha)


def _weights(scale, ext, base, nnz: int, k: int):
    """Validate the (scale, ext, base) triple of a weighted solve: all three
    or none.  Returns None (explicit path) or the triple."""
    given = [t is not None for t in (scale, ext, base)]
    if not any(given):
        return None
    if not all(given):
        raise ValueError("scale, ext and base go together: pass all three "
                         "(weighted normal equations) or none")
    if scale.dim() != 1 or ext.dim() != 1 or scale.numel() != nnz \
            or ext.numel() != nnz:
        raise ValueError(f"scale and ext must be 1-D with one element per "
                         f"stored entry ({nnz})")
    if base.dim() != 2 or base.shape[0] != k or base.shape[1] != k:
        raise ValueError(f"base must be [{k}][{k}], got {tuple(base.shape)}")
    return scale, ext, base


def _gpu_weights(w, kp: int):
    """fp32 contiguous scale / ext and the base matrix zero-padded to the
    kernels' [kp][kp]."""
    scale, ext, base = w
    base = base.to(torch.float32)
    k = base.shape[0]
    if k != kp:
        padded = torch.zeros(kp, kp, dtype=torch.float32, device=base.device)
        padded[:k, :k] = base
        base = padded
    return (scale.to(torch.float32).contiguous(),
            ext.to(torch.float32).contiguous(), base.contiguous())


# Lane-broadcast variants of the k<=64 register LDL (WREG_BC_* in
# als_kernels.hip).  All of them compute bit-identical results; the
# non-default ones are measured ablations (docs/KERNELS.md, round 3).
_WREG_BROADCAST = {"shfl": 0, "panel": 1, "subst": 2, "readlane": 3}


def _wreg_broadcast() -> int:
    """``FMA_WREG_BROADCAST`` selects the variant: ``readlane`` (default:
    v_readlane broadcasts, branch-free substitutions), ``shfl`` (the LDS
    shuffle path), or the ladder steps ``panel`` / ``subst`` (wave-fused
    kernel only)."""
    name = os.environ.get("FMA_WREG_BROADCAST", "readlane")
    if name not in _WREG_BROADCAST:
        raise ValueError(
            f"FMA_WREG_BROADCAST={name!r}: expected one of "
            f"{sorted(_WREG_BROADCAST)}")
    return _WREG_BROADCAST[name]


def _launch_fused(ops, indptr, csr: CSR, fac, out, ob, o8, ro, reg,
                  block: bool, allow_db: bool = False, w=None) -> None:
    """Launch the fused Gramian+solve kernel for ``fac``'s rank and dtype:
    the wave-fused kernel for k <= 64, the block-fused kernel for k > 64 or
    ``block=True``.  ``indptr`` bounds the launch (nrows = len - 1); ``ob``
    / ``o8`` / ``ro`` are the optional bf16 / e4m3 images and launch
    schedule (empty = absent).  The block kernel writes only the image of
    the gather dtype.  ``w`` = (scale, ext, base) selects the weighted twins
    (default broadcast level only)."""
    fp8 = fac.dtype == torch.uint8
    if w is not None:
        args = (indptr, csr.indices, *w, fac, out)
        if block or fac.shape[1] > 64:
            none = _empty(fac.device)
            ops.als_solve_fused_w(*args, none if fp8 else ob,
                                  o8 if fp8 else none, ro, float(reg),
                                  _stream())
        else:
            ops.als_solve_wavefused_w(*args, ob, o8, ro, float(reg),
                                      _stream())
        return
    args = (indptr, csr.indices, csr.values, fac, out)
    if block or fac.shape[1] > 64:
        none = _empty(fac.device)
        ops.als_solve_fused(*args, none if fp8 else ob, o8 if fp8 else none,
                            ro, float(reg), _stream())
        return
    fn = ops.als_solve_wavefused
    if allow_db and fp8 and os.environ.get("FMA_WAVEFUSED_DB") == "1":
        fn = ops.als_solve_wavefused_db
    fn(*args, ob, o8, ro, float(reg), _stream(), _wreg_broadcast())


def als_solve_side(
    csr: CSR,
    other_factors: torch.Tensor,
    reg: float,
    out_bf16: Optional[torch.Tensor] = None,
    out_fp8: Optional[torch.Tensor] = None,
    row_order: Optional[torch.Tensor] = None,
    fused: bool = False,
    slab_rows: Optional[int] = None,
    *,
    scale: Optional[torch.Tensor] = None,
    ext: Optional[torch.Tensor] = None,
    base: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """One ALS half-iteration: solve every row entity of ``csr`` against the
    opposite side's factors.  Returns fp32 [num_rows, k]; optionally also
    writes the bf16 (or e4m3 ``out_fp8``) image for the next half-iteration.

    GPU paths (fastest first; see docs/KERNELS.md for the measured ladder):
    - k <= 64 DEFAULT: the wave-fused kernel — Gramian MFMAs accumulate
      straight into the register LDL's lower-triangle C-fragments (one
      wave per entity, no A in HBM, no barriers; split-wave dual-chunk
      staging).  ``FMA_WAVEFUSED_DB=1`` selects the software-pipelined
      ablation, ``FMA_WREG_BROADCAST=shfl`` the LDS-shuffle broadcasts.
    - k > 64 (or ``fused=True``): the block-fused kernel (triangular LDS
      A image, 4 blocks/CU).
    - ``slab_rows`` (k <= 64; ignored above, where the block-fused kernel
      runs): the modular gramian -> batched-solve path, kept for parity
      tests and A-materializing consumers.
    ``other_factors`` dtype selects the gather precision: uint8 = e4m3
    bytes (one cache line per k<=64 row — the flagship path), anything
    else is cast to bf16.

    ``scale`` / ``ext`` / ``base`` (all three or none): the weighted normal
    equations of implicit-feedback ALS -- per stored entry a row scale and
    an EXT value (:func:`implicit_weights`), and the [k][k] base matrix
    (:func:`factor_gram` of the whole opposite side).  ``csr.values`` is
    not read then.  ``None`` is the explicit path, untouched.
    """
    w = _weights(scale, ext, base, csr.indices.numel(),
                 other_factors.shape[1])
    if other_factors.is_cuda:
        ops = _require_hip()
        fp8 = other_factors.dtype == torch.uint8
        if fp8:
            fac = other_factors.contiguous()   # pre-padded e4m3 byte image
            if fac.shape[1] % 16:
                raise ValueError("fp8 factor image must be 16-col padded")
        else:
            fac = _pad_k(other_factors.to(torch.bfloat16).contiguous())
        k = fac.shape[1]
        ob = out_bf16 if out_bf16 is not None else _empty(fac.device)
        o8 = out_fp8 if out_fp8 is not None else _empty(fac.device)
        ro = row_order if row_order is not None else _empty(fac.device)
        korig = other_factors.shape[1]
        if w is not None:
            w = _gpu_weights(w, k)
        if fused or k > 64 or slab_rows is None:
            # block-fused for k > 64 (and explicit fused=True), else the
            # k<=64 default: wave-fused Gramian+LDL — one wave per entity,
            # A lives only in MFMA C-fragments.  Neither pays the modular
            # path's nrows*k*k A round trip through HBM (the r2 profile
            # showed that path bound by exactly that write+read traffic)
            out = torch.empty(csr.num_rows, k, dtype=torch.float32,
                              device=fac.device)
            _launch_fused(ops, csr.indptr, csr, fac, out, ob, o8, ro, reg,
                          block=fused, allow_db=True, w=w)
        else:
            # slab the normal equations: A is nrows*k*k fp32, which at the
            # 1B-rating configs would exceed HBM if materialized whole.
            # A sliced indptr keeps GLOBAL offsets into indices/values, so
            # each slab call reuses the full nnz arrays untouched.
            # Measured (gpu_debug/slab_pipeline_timing.py): bigger slabs
            # are monotonically faster (fewer launch/tail bubbles), so the
            # cap is generous — 4 GiB of A in 288 GB HBM3E; two-stream
            # gramian/solve pipelining across slabs was NEUTRAL at every
            # slab size (the gramian saturates the CUs on its own) and is
            # kept out.
            cap = max(1, (4 << 30) // (k * k * 4))
            slab = slab_rows or max(1, min(csr.num_rows, cap))
            out = torch.empty(csr.num_rows, k, dtype=torch.float32,
                              device=fac.device)
            A = torch.empty(slab, k, k, dtype=torch.float32,
                            device=fac.device)
            b = torch.empty(slab, k, dtype=torch.float32, device=fac.device)
            # degree-descending schedule: only meaningful when one slab
            # covers the side (the gramian then scatters A/b by entity and
            # the solve stays order-agnostic); multi-slab runs skip it
            use_ro = ro if slab >= csr.num_rows else _empty(fac.device)
            for s in range(0, csr.num_rows, slab):
                e = min(s + slab, csr.num_rows)
                As, bs = A[: e - s], b[: e - s]
                if w is not None:
                    ops.gramian_w(csr.indptr[s:e + 1], csr.indices, *w, fac,
                                  As, bs, use_ro, float(reg), _stream())
                else:
                    ops.gramian(csr.indptr[s:e + 1], csr.indices,
                                csr.values, fac, As, bs, use_ro, float(reg),
                                _stream())
                obs = ob[s:e] if ob.numel() > 0 else ob
                o8s = o8[s:e] if o8.numel() > 0 else o8
                # k <= 64 here: larger ranks took the block-fused kernel
                ops.ldl_solve_wave_reg(As, bs, out[s:e], obs, o8s,
                                       _stream(), _wreg_broadcast())
        return out[:, :korig] if korig != k else out
    if w is not None:                        # CPU: the weighted reference
        out = reference.als_solve_weighted_reference(
            csr, other_factors, reg, *w)
        if out_fp8 is not None:
            out_fp8.copy_(quantize_fp8(out[:, : out_fp8.shape[1]]))
        if out_bf16 is not None:
            out_bf16.copy_(out[:, : out_bf16.shape[1]].to(torch.bfloat16))
        return out
    if other_factors.dtype == torch.uint8:   # CPU fp8 emulation
        out = reference.als_solve_side_reference(
            csr, dequantize_fp8(other_factors), reg)
        if out_fp8 is not None:
            out_fp8.copy_(quantize_fp8(out[:, : out_fp8.shape[1]]))
        return out
    return reference.als_solve_side_reference(csr, other_factors, reg)


def als_solve_chunk(
    csr: CSR,
    other_factors: torch.Tensor,
    reg: float,
    out_f32: torch.Tensor,
    out_fp8: Optional[torch.Tensor],
    out_bf16: Optional[torch.Tensor],
    entity_ids: torch.Tensor,
    *,
    scale: Optional[torch.Tensor] = None,
    ext: Optional[torch.Tensor] = None,
    base: Optional[torch.Tensor] = None,
) -> None:
    """Solve ONE slab of row entities (``entity_ids``) into the FULL-side
    output buffers (scatter by entity id through the kernels' row_order
    argument).  This is the building block of the overlapped C1 exchange:
    the trainer solves slab i while slab i-1's factors are already in
    flight over xGMI (SURVEY.md §7 hard part).  ``scale`` / ``ext`` /
    ``base``: the weighted solve, as in :func:`als_solve_side`.  An empty
    ``entity_ids`` leaves the buffers alone (the launchers refuse
    nrows = 0)."""
    w = _weights(scale, ext, base, csr.indices.numel(),
                 other_factors.shape[1])
    if entity_ids.numel() == 0:
        return
    if other_factors.is_cuda:
        ops = _require_hip()
        fp8 = other_factors.dtype == torch.uint8
        fac = (other_factors.contiguous() if fp8
               else other_factors.to(torch.bfloat16).contiguous())
        ids = entity_ids.to(torch.int32).contiguous()
        sub_indptr = csr.indptr  # full: kernels index it via row_order
        o8 = out_fp8 if out_fp8 is not None else _empty(fac.device)
        ob = out_bf16 if out_bf16 is not None else _empty(fac.device)
        # row_order-driven launch needs indptr[0:nrows+1] only for bounds;
        # pass a view sized to the slab so nrows = len(ids)
        ip = sub_indptr[: ids.numel() + 1]
        if w is not None:
            w = _gpu_weights(w, fac.shape[1])
        _launch_fused(ops, ip, csr, fac, out_f32, ob, o8, ids, reg,
                      block=False, w=w)
        return
    # CPU (gloo tests): contiguous id range sliced out of the CSR
    a = int(entity_ids.min())
    b = int(entity_ids.max()) + 1
    nnz0, nnz1 = int(csr.indptr[a]), int(csr.indptr[b])
    sub = CSR(csr.indptr[a:b + 1] - nnz0, csr.indices[nnz0:nnz1],
              csr.values[nnz0:nnz1], b - a, csr.num_cols)
    if w is not None:
        out = reference.als_solve_weighted_reference(
            sub, other_factors, reg, w[0][nnz0:nnz1], w[1][nnz0:nnz1], w[2])
    else:
        fac32 = (dequantize_fp8(other_factors)
                 if other_factors.dtype == torch.uint8
                 else other_factors.to(torch.float32))
        out = reference.als_solve_side_reference(sub, fac32, reg)
    out_f32[a:b] = out
    if out_fp8 is not None:
        out_fp8[a:b] = quantize_fp8(out[:, : out_fp8.shape[1]])
    if out_bf16 is not None:
        out_bf16[a:b] = out[:, : out_bf16.shape[1]].to(torch.bfloat16)


def gramian(csr: CSR, factors: torch.Tensor, reg: float, *,
            scale: Optional[torch.Tensor] = None,
            ext: Optional[torch.Tensor] = None,
            base: Optional[torch.Tensor] = None,
            ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Standalone K1 (parity tests / modular path).  ``factors`` as uint8 =
    e4m3 bytes -> the fp8 gather kernel; else bf16.  ``scale`` / ``ext`` /
    ``base``: the weighted normal equations, as in :func:`als_solve_side`."""
    w = _weights(scale, ext, base, csr.indices.numel(), factors.shape[1])
    if factors.is_cuda:
        ops = _require_hip()
        fp8 = factors.dtype == torch.uint8
        fac = (factors.contiguous() if fp8
               else _pad_k(factors.to(torch.bfloat16).contiguous()))
        k = fac.shape[1]
        A = torch.empty(csr.num_rows, k, k, dtype=torch.float32, device=fac.device)
        b = torch.empty(csr.num_rows, k, dtype=torch.float32, device=fac.device)
        if w is not None:
            ops.gramian_w(csr.indptr, csr.indices, *_gpu_weights(w, k), fac,
                          A, b, _empty(fac.device), float(reg), _stream())
        else:
            ops.gramian(csr.indptr, csr.indices, csr.values, fac, A, b,
                        _empty(fac.device), float(reg), _stream())
        korig = factors.shape[1]
        if korig != k:
            return A[:, :korig, :korig], b[:, :korig]
        return A, b
    if w is not None:
        return reference.gramian_weighted_reference(csr, factors, reg, *w)
    if factors.dtype == torch.uint8:
        return reference.gramian_reference(csr, dequantize_fp8(factors), reg)
    return reference.gramian_reference(csr, factors, reg)


def _gram_rows(rows: torch.Tensor, ntable: int) -> torch.Tensor:
    """Validate a ``factor_gram`` row list against a table of ``ntable``
    rows: 1-D int64 / int32, every entry a row of the table."""
    if rows.dim() != 1 or rows.dtype not in (torch.int64, torch.int32):
        raise ValueError("rows must be a 1-D int64 or int32 tensor")
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= ntable):
        raise ValueError(f"rows entries must be rows of factors "
                         f"(0..{ntable - 1})")
    return rows


def factor_gram(factors: torch.Tensor,
                rows_per_part: Optional[int] = None, *,
                rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``G = F^T F`` [k][k] fp32 over every row of a factor table: the base
    matrix of the implicit-feedback solves.  On the GPU the table is read
    as stored (uint8 = e4m3 bytes, else bf16; e4m3 is widened exactly to
    bf16 in staging) and contracted by the bf16 MFMA; per-wave partial sums over ``rows_per_part`` rows (``None`` =
    the launcher's choice, see :func:`factor_gram_rows_per_part`) are added
    in a fixed order, so the result is bit-reproducible and exactly
    symmetric; it depends on ``rows_per_part`` only within fp32 rounding.
    Ranks up to 128.

    ``rows`` (int64 or int32, 1-D): sum over these rows of the table only,
    ``G = sum_j F[rows[j]] F[rows[j]]^T`` -- the live rows of a serving
    table, read in place (no compacted copy).  Rows may repeat (a repeated
    row counts once per occurrence) and come in any order; every entry must
    be a row of the table, which is checked here (the kernel does not).
    Parts are over list positions, so with the same ``rows_per_part`` the
    GPU result is bit-equal to ``factor_gram(F[rows])``: the same MFMA
    sequence, hence as reproducible and exactly symmetric.  An empty list
    gives zeros.  The GPU path takes tables of fewer than 2^31 rows.  A
    table whose rank is not a multiple of 16 (or that is not stored as
    bf16 / e4m3) pays one padded (converted) copy of the whole table per
    call."""
    if factors.dim() != 2:
        raise ValueError("factors must be 2-D")
    if rows is not None:
        rows = _gram_rows(rows, factors.shape[0])
    if factors.is_cuda:
        ops = _require_hip()
        fp8 = factors.dtype == torch.uint8
        if fp8:
            fac = factors.contiguous()
            if fac.shape[1] % 16:
                raise ValueError("fp8 factor image must be 16-col padded")
        else:
            fac = _pad_k(factors.to(torch.bfloat16).contiguous())
        k, korig = fac.shape[1], factors.shape[1]
        if k > 128:
            raise ValueError(f"factor_gram handles rank <= 128, got {korig}")
        if rows is not None:
            if fac.shape[0] >= 2 ** 31:
                raise ValueError("factor_gram(rows=) handles tables of fewer "
                                 f"than 2^31 rows, got {fac.shape[0]}")
            if rows.numel() == 0:
                return torch.zeros(korig, korig, dtype=torch.float32,
                                   device=fac.device)
            G = ops.factor_gram_rows(
                fac, rows.to(device=fac.device, dtype=torch.int32)
                .contiguous(), int(rows_per_part or 0), _stream())
            return G[:korig, :korig] if korig != k else G
        if fac.shape[0] == 0:
            return torch.zeros(korig, korig, dtype=torch.float32,
                               device=fac.device)
        G = ops.factor_gram(fac, int(rows_per_part or 0), _stream())
        return G[:korig, :korig] if korig != k else G
    return reference.factor_gram_reference(factors, rows)


def factor_gram_rows_per_part(n: int, k: int) -> int:
    """Rows per part a GPU ``factor_gram`` over an [n][k] table uses when
    ``rows_per_part`` is not given (k the 16-padded rank)."""
    return int(_require_hip().factor_gram_rows_per_part(int(n), int(k)))


def cholesky_solve(A: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    if A.is_cuda:
        ops = _require_hip()
        A = A.contiguous()
        b = b.contiguous()
        x = torch.empty_like(b)
        ops.cholesky_solve(A, b, x, _stream())
        return x
    return reference.cholesky_solve_reference(A, b)


# -------------------------------------------------------------------- SVM

def sdca_pass(
    csr: CSR,
    y: torch.Tensor,
    alpha: torch.Tensor,
    v: torch.Tensor,
    lamb: float,
    n_global: int,
    norms_sq: Optional[torch.Tensor] = None,
    perm: Optional[torch.Tensor] = None,
) -> None:
    """One local SDCA pass over the shard, updating alpha and v in place."""
    if v.is_cuda:
        ops = _require_hip()
        if norms_sq is None:
            norms_sq = csr_row_norms_sq(csr)
        p = perm.to(torch.int32) if perm is not None else _empty(v.device)
        ops.sdca_pass(csr.indptr, csr.indices, csr.values, y, norms_sq, p,
                      alpha, v, 1.0 / (lamb * n_global), _stream())
        return
    reference.sdca_epoch_reference(csr, y, alpha, v, lamb, n_global, perm)


def sdca_num_waves(nrows: int) -> int:
    """Waves one GPU ``sdca_pass`` over ``nrows`` samples is launched with.

    Wave ``w`` of ``W`` walks schedule positions ``w, w + W, w + 2W, ...``
    sequentially (position ``p`` is sample ``perm[p]``, or ``p`` without a
    permutation)."""
    return int(_require_hip().sdca_num_waves(int(nrows)))


def csr_row_norms_sq(csr: CSR) -> torch.Tensor:
    row_ids = torch.repeat_interleave(
        torch.arange(csr.num_rows, dtype=torch.int64, device=csr.device),
        csr.row_counts(),
    )
    out = torch.zeros(csr.num_rows, dtype=torch.float32, device=csr.device)
    out.index_add_(0, row_ids, csr.values * csr.values)
    return out


def svm_margins(csr: CSR, w: torch.Tensor) -> torch.Tensor:
    if w.is_cuda:
        ops = _require_hip()
        out = torch.empty(csr.num_rows, dtype=torch.float32, device=w.device)
        ops.svm_margins(csr.indptr, csr.indices, csr.values, w.contiguous(),
                        out, _stream())
        return out
    return reference.svm_margins_reference(csr, w)


# ---------------------------------------------------------------- serving

def predict_dot(U: torch.Tensor, V: torch.Tensor, u_idx: torch.Tensor,
                i_idx: torch.Tensor) -> torch.Tensor:
    if U.is_cuda:
        ops = _require_hip()
        out = torch.empty(u_idx.numel(), dtype=torch.float32, device=U.device)
        ops.predict_dot(U.to(torch.bfloat16).contiguous(),
                        V.to(torch.bfloat16).contiguous(), u_idx.long(),
                        i_idx.long(), out, _stream())
        return out
    return reference.predict_dot_reference(U, V, u_idx, i_idx)


def topk_scores(Q: torch.Tensor, V: torch.Tensor, topk: int,
                cand: Optional[torch.Tensor] = None,
                exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                chunk_items: Optional[int] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-N recommendations: for every query row of ``Q`` [nq, k] the
    ``topk`` best rows of ``V`` [nv, k] by dot product, fused score +
    selection on the GPU (the [nq, nv] score matrix is never materialized).

    ``cand``: int64 rows of V to consider (``None`` = all).  ``exclude`` =
    ``(excl_ptr [nq + 1], excl_rows)``: per query an ascending slice of V
    rows never to return.  ``chunk_items`` overrides the launcher's split
    of the candidates (tests; the result does not depend on it).

    Returns (scores fp32 [nq, topk], rows int64 [nq, topk]): score
    descending, lower row first among equal scores, NaN scores last, short
    results padded with row -1 / score -inf."""
    topk = int(topk)
    if not 1 <= topk <= 128:
        raise ValueError(f"topk must be in 1..128, got {topk}")
    if Q.dim() != 2 or V.dim() != 2 or Q.shape[1] != V.shape[1]:
        raise ValueError("Q and V must be 2-D with one rank")
    nq, nv = Q.shape[0], V.shape[0]
    if cand is not None:
        cand = cand.long().contiguous()
        if cand.dim() != 1 or cand.numel() == 0:
            raise ValueError("cand must be 1-D and non-empty")
        if int(cand.min()) < 0 or int(cand.max()) >= nv:
            raise ValueError(f"cand entries must be rows of V (0..{nv - 1})")
    if exclude is not None:
        ptr, ex = exclude
        ptr = ptr.long().contiguous()
        ex = ex.long().contiguous()
        if ptr.dim() != 1 or ptr.numel() != nq + 1 or ex.dim() != 1:
            raise ValueError("exclude must be (excl_ptr [nq + 1], excl_rows)")
        if (int(ptr[0]) < 0 or int(ptr[-1]) > ex.numel()
                or bool((ptr[1:] < ptr[:-1]).any())):
            raise ValueError("excl_ptr must be non-decreasing offsets into "
                             "excl_rows")
        exclude = (ptr, ex)
    if Q.is_cuda:
        ops = _require_hip()
        none = _empty(Q.device)
        ptr, ex = exclude if exclude is not None else (none, none)
        return tuple(ops.topk_scores(
            Q.to(torch.bfloat16).contiguous(),
            V.to(torch.bfloat16).contiguous(),
            cand.to(Q.device) if cand is not None else none,
            ptr.to(Q.device), ex.to(Q.device), topk,
            int(chunk_items or 0), _stream()))
    return reference.topk_scores_reference(Q, V, topk, cand, exclude)


def topk_chunk_items(nq: int, nc: int, topk: int) -> int:
    """Candidates per chunk that a GPU ``topk_scores`` over ``nq`` queries
    and ``nc`` candidates uses when ``chunk_items`` is not given: one wave
    scores one (16-query tile, chunk) pair."""
    return int(_require_hip().topk_chunk_items(int(nq), int(nc), int(topk)))


def _rank_args(nq: int, nv: int, q_idx, cand, exclude):
    """Validate and normalise the index arguments of the rank-count entry
    points.  Returns (q_idx, cand, exclude) as contiguous int64, the
    exclusion slices reduced to candidate rows."""
    q_idx = q_idx.long().contiguous()
    if q_idx.dim() != 1:
        raise ValueError("q_idx must be 1-D")
    if q_idx.numel() and (int(q_idx.min()) < 0 or int(q_idx.max()) >= nq):
        raise ValueError(f"q_idx entries must be rows of Q (0..{nq - 1})")
    if cand is not None:
        cand = cand.long().contiguous()
        if cand.dim() != 1 or cand.numel() == 0:
            raise ValueError("cand must be 1-D and non-empty")
        if int(cand.min()) < 0 or int(cand.max()) >= nv:
            raise ValueError(f"cand entries must be rows of V (0..{nv - 1})")
        if torch.unique(cand).numel() != cand.numel():
            raise ValueError("cand must not repeat a row")
    if exclude is not None:
        ptr, ex = exclude
        ptr = ptr.long().contiguous()
        ex = ex.long().contiguous()
        if ptr.dim() != 1 or ptr.numel() != nq + 1 or ex.dim() != 1:
            raise ValueError("exclude must be (excl_ptr [nq + 1], excl_rows)")
        if (int(ptr[0]) < 0 or int(ptr[-1]) > ex.numel()
                or bool((ptr[1:] < ptr[:-1]).any())):
            raise ValueError("excl_ptr must be non-decreasing offsets into "
                             "excl_rows")
        ex = ex[int(ptr[0]):int(ptr[-1])]
        ptr = ptr - ptr[0]
        if ex.numel():
            if int(ex.min()) < 0 or int(ex.max()) >= nv:
                raise ValueError(
                    f"excl_rows entries must be rows of V (0..{nv - 1})")
            # strictly ascending inside every slice: a step down or a repeat
            # is only allowed where the next slice starts
            rising = torch.ones(ex.numel(), dtype=torch.bool,
                                device=ex.device)
            rising[1:] = ex[1:] > ex[:-1]
            starts = ptr[:-1][ptr[:-1] < ex.numel()]
            rising[starts] = True
            if not bool(rising.all()):
                raise ValueError("every exclusion slice must be strictly "
                                 "ascending")
            if cand is not None:
                # excluded rows that are no candidates were never counted
                is_cand = torch.zeros(nv, dtype=torch.bool, device=ex.device)
                is_cand[cand.to(ex.device)] = True
                keep = is_cand[ex]
                kept = torch.zeros(ex.numel() + 1, dtype=torch.int64,
                                   device=ex.device)
                kept[1:] = torch.cumsum(keep, 0)
                ptr = kept[ptr]
                ex = ex[keep]
        exclude = (ptr.contiguous(), ex.contiguous())
    return q_idx, cand, exclude


def rank_counts_vectors(Q: torch.Tensor, V: torch.Tensor, T: torch.Tensor,
                        q_idx: torch.Tensor, skip: torch.Tensor,
                        cand: Optional[torch.Tensor] = None,
                        exclude: Optional[Tuple[torch.Tensor,
                                                torch.Tensor]] = None,
                        chunk_items: Optional[int] = None
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """:func:`rank_counts` with the targets given as VECTORS ``T`` [P, k]
    plus ``skip`` [P], the row of V not to count (-1 = none), instead of as
    rows of V: the form the serving store needs, where a target may live in
    another factor table than the one being scanned."""
    if (Q.dim() != 2 or V.dim() != 2 or T.dim() != 2
            or Q.shape[1] != V.shape[1] or Q.shape[1] != T.shape[1]):
        raise ValueError("Q, V and T must be 2-D with one rank")
    nq, nv = Q.shape[0], V.shape[0]
    q_idx, cand, exclude = _rank_args(nq, nv, q_idx, cand, exclude)
    skip = skip.long().contiguous()
    P = q_idx.numel()
    if T.shape[0] != P or skip.dim() != 1 or skip.numel() != P:
        raise ValueError("T and skip must hold one entry per pair")
    if P and (int(skip.min()) < -1 or int(skip.max()) >= nv):
        raise ValueError(f"skip entries must be -1 or rows of V "
                         f"(0..{nv - 1})")
    dev = Q.device
    if P == 0:
        return (torch.zeros(0, dtype=torch.int64, device=dev),
                torch.zeros(0, dtype=torch.int64, device=dev),
                torch.zeros(0, dtype=torch.float32, device=dev))
    if Q.is_cuda:
        ops = _require_hip()
        none = _empty(dev)
        ptr, ex = exclude if exclude is not None else (none, none)
        return tuple(ops.rank_counts(
            Q.to(torch.bfloat16).contiguous(),
            V.to(torch.bfloat16).contiguous(),
            T.to(device=dev, dtype=torch.bfloat16).contiguous(),
            q_idx.to(dev), skip.to(dev),
            cand.to(dev) if cand is not None else none,
            ptr.to(dev), ex.to(dev), int(chunk_items or 0), _stream()))
    # CPU: the fp32 reference over V with the targets appended as extra
    # rows that are no candidates
    rows = (torch.arange(nv, dtype=torch.int64) if cand is None
            else cand.cpu())
    Vx = torch.cat([V.cpu().float(), T.cpu().float()])
    return reference._rank_counts(Q, Vx, q_idx, nv + torch.arange(P), rows,
                                  exclude, torch.float32, skip=skip)


def rank_counts(Q: torch.Tensor, V: torch.Tensor, q_idx: torch.Tensor,
                t_idx: torch.Tensor, cand: Optional[torch.Tensor] = None,
                exclude: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                chunk_items: Optional[int] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Where a target item ranks for a query, fused score + count on the
    GPU (the [P, nv] score matrix is never materialized).  For pair ``p``,
    query ``Q[q_idx[p]]`` and target row ``t = t_idx[p]`` of V:

    ``score[p]``   ``dot(Q[q_idx[p]], V[t])`` accumulated in fp32;
    ``greater[p]`` candidate rows ``r != t`` outside the query's exclusion
                   slice that score strictly above the target;
    ``equal[p]``   those that score equal to it.

    Scores compare as in :func:`topk_scores` (NaN below every number and
    equal to NaN, -0 equal to +0) and are the same bits; the row plays no
    part, so every tie convention follows from the two counts.  ``cand``:
    int64 rows of V without repeats (``None`` = all).  ``exclude =
    (excl_ptr [nq + 1], excl_rows)`` is indexed by QUERY row, each slice
    strictly ascending: a sorted, deduplicated training CSR as it stands.
    The target never counts, candidate or not, excluded or not.
    ``chunk_items`` overrides the launcher's split of the candidates
    (tests; the result does not depend on it).

    Returns (greater int64 [P], equal int64 [P], score fp32 [P])."""
    if Q.dim() != 2 or V.dim() != 2 or Q.shape[1] != V.shape[1]:
        raise ValueError("Q and V must be 2-D with one rank")
    nv = V.shape[0]
    t_idx = t_idx.long().contiguous()
    if t_idx.dim() != 1 or t_idx.numel() != q_idx.numel():
        raise ValueError("q_idx and t_idx must be 1-D of one length")
    if t_idx.numel() and (int(t_idx.min()) < 0 or int(t_idx.max()) >= nv):
        raise ValueError(f"t_idx entries must be rows of V (0..{nv - 1})")
    if Q.is_cuda:
        t_dev = t_idx.to(V.device)
        return rank_counts_vectors(Q, V, V[t_dev], q_idx, t_dev, cand,
                                   exclude, chunk_items)
    q_idx, cand, exclude = _rank_args(Q.shape[0], nv, q_idx, cand, exclude)
    return reference.rank_counts_reference(Q, V, q_idx, t_idx, cand, exclude)


def rank_chunk_items(P: int, nc: int) -> int:
    """Candidates per chunk that a GPU ``rank_counts`` over ``P`` pairs and
    ``nc`` candidates uses when ``chunk_items`` is not given: one wave
    scans one (16-pair tile, chunk)."""
    chunk = int(_require_hip().rank_chunk_items(int(P), int(nc)))
    if chunk < 0:
        raise ValueError("need P, nc >= 1 and nc < 2^31")
    return chunk


def sgd_update(U: torch.Tensor, V: torch.Tensor, u_idx: torch.Tensor,
               i_idx: torch.Tensor, r: torch.Tensor, lr: float,
               user_reg: float, item_reg: float) -> torch.Tensor:
    """In-place online SGD step on the bf16 factor store; returns errors."""
    if U.is_cuda:
        ops = _require_hip()
        err = torch.empty(u_idx.numel(), dtype=torch.float32, device=U.device)
        ops.sgd_update(U, V, u_idx.long(), i_idx.long(), r, err,
                       float(lr), float(user_reg), float(item_reg), _stream())
        return err
    u = u_idx.long()
    i = i_idx.long()
    p = U[u].to(torch.float32)
    q = V[i].to(torch.float32)
    p_new, q_new, err = reference.sgd_update_reference(
        p, q, r, lr, user_reg, item_reg)
    U[u] = p_new.to(U.dtype)
    V[i] = q_new.to(V.dtype)
    return err
