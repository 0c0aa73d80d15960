"""Argument validation of the weighted-ALS bindings (``gramian_w``,
``als_solve_fused_w``, ``als_solve_wavefused_w``, ``factor_gram``).

Same pattern as test_hip_topk_args.py: metadata checks run first and the
device check last, so every rejected shape is testable on CPU tensors
wherever the extension is built; a fully valid CPU call must then die on the
device check, never launch.
"""

import pytest
import torch

from flink_ms_amd import ops

if not ops.hip_available():
    pytest.skip("HIP extension not built", allow_module_level=True)

import flink_ms_amd._hip_ops as hip  # noqa: E402

NROWS, NNZ, NCOLS, K = 4, 12, 9, 16


def _args(k=K, fp8=False):
    fac = (torch.zeros(NCOLS, k, dtype=torch.uint8) if fp8
           else torch.zeros(NCOLS, k, dtype=torch.bfloat16))
    return dict(
        indptr=torch.arange(0, NNZ + 1, NNZ // NROWS, dtype=torch.int64),
        indices=torch.zeros(NNZ, dtype=torch.int32),
        scale=torch.ones(NNZ), ext=torch.ones(NNZ),
        base=torch.zeros(k, k), factors=fac,
        out_f32=torch.zeros(NROWS, k), out_bf16=torch.empty(0),
        out_fp8=torch.empty(0), row_order=torch.empty(0))


def _solve(fn):
    def call(a):
        return fn(a["indptr"], a["indices"], a["scale"], a["ext"], a["base"],
                  a["factors"], a["out_f32"], a["out_bf16"], a["out_fp8"],
                  a["row_order"], 0.1, 0)
    return call


def _gramian(a):
    k = a["factors"].shape[1]
    return hip.gramian_w(a["indptr"], a["indices"], a["scale"], a["ext"],
                         a["base"], a["factors"], torch.zeros(NROWS, k, k),
                         torch.zeros(NROWS, k), a["row_order"], 0.1, 0)


CALLS = {"gramian_w": _gramian,
         "als_solve_fused_w": _solve(hip.als_solve_fused_w),
         "als_solve_wavefused_w": _solve(hip.als_solve_wavefused_w)}

BAD = [
    ("scale-dtype", "scale must be", dict(scale=torch.ones(NNZ).double())),
    ("ext-dtype", "ext must be", dict(ext=torch.ones(NNZ).half())),
    ("scale-short", "scale must be 1-D with one element per stored entry",
     dict(scale=torch.ones(NNZ - 1))),
    ("ext-long", "ext must be 1-D with one element per stored entry",
     dict(ext=torch.ones(NNZ + 1))),
    ("scale-2d", "scale must be 1-D", dict(scale=torch.ones(NNZ, 1))),
    ("ext-noncontig", "ext must be contiguous",
     dict(ext=torch.ones(2 * NNZ)[::2])),
    ("base-dtype", "base must be", dict(base=torch.zeros(K, K).double())),
    ("base-shape", "base must be \\[16\\]\\[16\\]",
     dict(base=torch.zeros(K, K + 16))),
    ("base-flat", "base must be \\[16\\]\\[16\\]",
     dict(base=torch.zeros(K * K))),
    ("base-noncontig", "base must be contiguous",
     dict(base=torch.zeros(K, 2 * K)[:, ::2])),
    ("indices-dtype", "indices must be",
     dict(indices=torch.zeros(NNZ, dtype=torch.int64))),
    ("row-order", "row_order must be empty or 1-D",
     dict(row_order=torch.zeros(NROWS + 1, dtype=torch.int32))),
]


@pytest.mark.parametrize("fn", sorted(CALLS))
@pytest.mark.parametrize("name,match,change", BAD, ids=[b[0] for b in BAD])
def test_weighted_bindings_reject_bad_metadata(fn, name, match, change):
    a = _args()
    a.update(change)
    with pytest.raises(RuntimeError, match=f"{fn}: {match}"):
        CALLS[fn](a)


@pytest.mark.parametrize("fn", sorted(CALLS))
@pytest.mark.parametrize("fp8", [False, True])
def test_weighted_bindings_device_check_is_last(fn, fp8):
    with pytest.raises(RuntimeError, match=f"{fn}: .* must be on the GPU"):
        CALLS[fn](_args(fp8=fp8))


def test_wavefused_w_rejects_rank_above_64():
    with pytest.raises(RuntimeError, match="at most 64"):
        CALLS["als_solve_wavefused_w"](_args(k=80))


def test_fused_w_rejects_the_other_dtypes_image():
    a = _args()
    a["out_fp8"] = torch.zeros(NROWS, K, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="out_fp8 must be empty with bf16"):
        CALLS["als_solve_fused_w"](a)


def test_factor_gram_binding_checks():
    tab = torch.zeros(10, K, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="factor_gram: factors must be"):
        hip.factor_gram(tab.float(), 0, 0)
    with pytest.raises(RuntimeError, match="need a multiple of 16"):
        hip.factor_gram(torch.zeros(10, 10, dtype=torch.bfloat16), 0, 0)
    with pytest.raises(RuntimeError, match="at most 128"):
        hip.factor_gram(torch.zeros(10, 144, dtype=torch.bfloat16), 0, 0)
    with pytest.raises(RuntimeError, match="at least one row"):
        hip.factor_gram(tab[:0], 0, 0)
    with pytest.raises(RuntimeError, match="rows_per_part must be >= 0"):
        hip.factor_gram(tab, -1, 0)
    with pytest.raises(RuntimeError, match="factors must be on the GPU"):
        hip.factor_gram(tab, 0, 0)
    # the launcher's split: multiples of the 32-row stage chunk
    assert hip.factor_gram_rows_per_part(1, 16) == 32
    assert hip.factor_gram_rows_per_part(1000, 64) == 32
    big = hip.factor_gram_rows_per_part(10_000_000, 64)
    assert big % 32 == 0 and big * 1024 >= 10_000_000
    with pytest.raises(RuntimeError):
        hip.factor_gram_rows_per_part(0, 16)
