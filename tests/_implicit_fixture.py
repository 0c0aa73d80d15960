"""Shared data builders for the implicit-feedback (weighted ALS) tests.

Hard conditions every builder keeps (docs/KERNELS.md "Implicit feedback"):
|scale * factor| <= 64 and |ext| <= 64 -- far inside e4m3's +-448, so
saturation never enters -- and the tests use reg > 0.
"""

import torch

from flink_ms_amd import ops
from flink_ms_amd.data.blocked import CSR, csr_from_coo

# Worst measured ratio of the EXPLICIT e4m3 kernel's distance from the
# float64 oracle to the fp32 reference's, per fused path (the measurements
# are in test_gpu_implicit.py's docstring).  e4m3 solves are allowed twice
# this in place of the bf16 factor 4; shared with test_gpu_trainer_parity.py.
FP8_EXPLICIT_RATIO = {"wave": 154.2, "block": 38.3}

# chunk (32) and dual-chunk (64) edges of the staging loops
ROW_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 97, 129)


def csr_with_row_lengths(lengths, num_cols, seed, device="cpu") -> CSR:
    """CSR whose row i has lengths[i] stored entries: random columns (with
    repeats across rows) and values in {-2, ..., 5}, so r < 0 and r = 0 both
    occur; every third entry is +-4 (alpha = 100 makes alpha*|r| = 400)."""
    g = torch.Generator().manual_seed(seed)
    lengths = torch.tensor(list(lengths), dtype=torch.int64)
    nnz = int(lengths.sum())
    indptr = torch.zeros(lengths.numel() + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=indptr[1:])
    indices = torch.randint(0, num_cols, (nnz,), generator=g).to(torch.int32)
    values = torch.randint(-2, 6, (nnz,), generator=g).to(torch.float32)
    values[::3] = torch.where(values[::3] < 0, -4.0, 4.0)
    if nnz > 4:
        values[1] = 0.0
        values[2] = -1.0
    return CSR(indptr.to(device), indices.to(device), values.to(device),
               lengths.numel(), num_cols)


def factor_table(n, k, seed, gather, device="cpu"):
    """Random factors in (-1.5, 1.5) stored as the gather dtype: uint8 e4m3
    bytes for 'fp8', bf16 for 'bf16'.  With scale <= 20 (alpha*|r| <= 400),
    |scale * f| <= 30."""
    g = torch.Generator().manual_seed(seed)
    f = (torch.rand(n, k, generator=g) - 0.5) * 3.0
    t = ops.quantize_fp8(f) if gather == "fp8" else f.to(torch.bfloat16)
    return t.to(device)


def random_base(k, seed, device="cpu"):
    """Gram matrix of a random 200-row table (symmetric, PSD), fp32."""
    g = torch.Generator().manual_seed(seed)
    f = torch.rand(200, k, generator=g, dtype=torch.float64) - 0.5
    return (f.T @ f).to(torch.float32).to(device)


def planted_implicit(num_users, num_items, per_user, blocks, seed):
    """Planted block preferences: user u belongs to block u % blocks and
    interacts (strength 1..5) mostly with items of its block, plus a few
    strength-1 interactions anywhere.  Returns int64 users, items and fp32
    strengths, one entry per (user, item) pair."""
    g = torch.Generator().manual_seed(seed)
    users = torch.arange(num_users).repeat_interleave(per_user)
    ublock = users % blocks
    in_block = torch.rand(users.numel(), generator=g) < 0.85
    per_block = num_items // blocks
    within = torch.randint(0, per_block, (users.numel(),), generator=g)
    anywhere = torch.randint(0, num_items, (users.numel(),), generator=g)
    items = torch.where(in_block, within * blocks + ublock, anywhere)
    strength = torch.where(
        in_block,
        torch.randint(1, 6, (users.numel(),), generator=g).float(),
        torch.ones(users.numel()))
    key = users * num_items + items
    # keep the first occurrence of each pair
    order = torch.argsort(key, stable=True)
    keep = torch.ones_like(key, dtype=torch.bool)
    ks = key[order]
    keep[order[1:]] = ks[1:] != ks[:-1]
    return users[keep], items[keep], strength[keep]


def user_item_csr(users, items, values, num_users, num_items) -> CSR:
    return csr_from_coo(users.long(), items.to(torch.int32), values,
                        num_users, num_items)
