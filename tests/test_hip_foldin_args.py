"""Argument validation of the row-list Gram binding (``factor_gram_rows``).

Same pattern as test_hip_implicit_args.py: metadata checks run first and the
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

K = 16
TAB = torch.zeros(10, K, dtype=torch.bfloat16)
ROWS = torch.tensor([3, 1, 3], dtype=torch.int32)

BAD = [
    ("rows-int64", "rows must be", dict(rows=ROWS.long())),
    ("rows-float", "rows must be", dict(rows=ROWS.float())),
    ("rows-2d", "rows must be 1-D", dict(rows=ROWS.reshape(3, 1))),
    ("rows-empty", "rows must have at least one entry", dict(rows=ROWS[:0])),
    ("rows-noncontig", "rows must be contiguous",
     dict(rows=torch.zeros(6, dtype=torch.int32)[::2])),
    ("rank-144", "at most 128",
     dict(factors=torch.zeros(10, 144, dtype=torch.bfloat16))),
    ("rank-10", "need a multiple of 16",
     dict(factors=torch.zeros(10, 10, dtype=torch.bfloat16))),
    ("factors-dtype", "factors must be", dict(factors=TAB.float())),
    ("factors-empty", "factors must have 1..2\\^31-1 rows",
     dict(factors=TAB[:0])),
    ("rows-per-part", "rows_per_part must be >= 0", dict(rows_per_part=-1)),
]


def _call(**change):
    a = dict(factors=TAB, rows=ROWS, rows_per_part=0)
    a.update(change)
    return hip.factor_gram_rows(a["factors"], a["rows"], a["rows_per_part"], 0)


@pytest.mark.parametrize("name,match,change", BAD, ids=[b[0] for b in BAD])
def test_factor_gram_rows_rejects_bad_metadata(name, match, change):
    with pytest.raises(RuntimeError, match=f"factor_gram_rows: .*{match}"):
        _call(**change)


@pytest.mark.parametrize("fp8", [False, True])
def test_factor_gram_rows_device_check_is_last(fp8):
    tab = torch.zeros(10, K, dtype=torch.uint8) if fp8 else TAB
    with pytest.raises(RuntimeError,
                       match="factor_gram_rows: .* must be on the GPU"):
        _call(factors=tab)


def test_wrapper_checks_the_row_list():
    # the Python entry range-checks on any device: the kernel does not
    with pytest.raises(ValueError, match="rows entries must be rows"):
        ops.factor_gram(TAB, rows=torch.tensor([0, 10]))
    with pytest.raises(ValueError, match="rows entries must be rows"):
        ops.factor_gram(TAB, rows=torch.tensor([-1]))
    with pytest.raises(ValueError, match="1-D int64 or int32"):
        ops.factor_gram(TAB, rows=torch.tensor([[1]]))
    with pytest.raises(ValueError, match="1-D int64 or int32"):
        ops.factor_gram(TAB, rows=torch.tensor([1.0]))
