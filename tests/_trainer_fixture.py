"""Shared harness of the dispatch / trainer parity tests (CPU-only code).

Three pieces (docs/KERNELS.md "Dispatch and trainer parity"):

- ``small_ratings``: one tiny rating set whose sizes divide by nothing the
  code cares about and whose row lengths sit on the staging edges;
- ``replay``: the reference chain -- one flat ``ops.als_solve_side`` call per
  half-iteration, fed the previous low-precision image, built from the
  triples and the config alone;
- ``run_trainer``: an ``ALSTrainer`` stepped with its state recorded after
  every ``step()``.

Every fused kernel solves one entity from that entity's own stored row, in
stored order, so chunking, launch order and the replica layout change where
a row lives and when it is solved, never an operand: trainer and replay are
compared with ``torch.equal`` on bit patterns (``assert_same_bits``).
"""

from typing import List, NamedTuple, Tuple

import torch

from flink_ms_amd import ops
from flink_ms_amd.data.blocked import csr_from_coo
from flink_ms_amd.models.als import ALSConfig, ALSTrainer
from flink_ms_amd.parallel.dist import DistContext

NUM_USERS, NUM_ITEMS = 157, 71
# entities without a single entry (user 0, the last user, the last item)
EMPTY_USERS = (0, 77, NUM_USERS - 1)
EMPTY_ITEMS = (13, NUM_ITEMS - 1)
# users with exactly this many entries: the 32-entry staging chunk and the
# 64-entry dual chunk, and one past each
EDGE_USERS = {5: 32, 6: 33, 7: 64, 8: 65}
# the row that reaches a third staging chunk.  With unique cells a user has
# at most NUM_ITEMS entries, so this is an ITEM row (solved from the users)
HEAVY_ITEM, HEAVY_ITEM_MIN = 3, 129
ALPHA = 10.0          # implicit: alpha * r <= 50, scale <= 7.1, ext <= 7.3
REG = 0.1
STEPS = 3
# exchange chunk counts: one, two that divide neither side, one larger than
# both sides (one row per slab)
MODES = (("off", 4), ("force", 1), ("force", 3), ("force", 7),
         ("force", 200))
# ... and one whose rounded-up slabs cover the shard early (71 rows / 50 ->
# 36 slabs of 2, 157 / 50 -> 40 of 4): the CPU path only
MODES_CPU = MODES + (("force", 50),)


class Cfg(NamedTuple):
    gather: str               # 'bf16' or 'fp8' (e4m3 images)
    implicit: bool
    k: int
    mode: str = "off"         # ALSConfig.overlap_exchange
    chunks: int = 4           # ALSConfig.exchange_chunks


class Record(NamedTuple):
    """State after one ``step()`` (clones)."""
    user_f32: torch.Tensor
    item_f32: torch.Tensor
    user_image: torch.Tensor
    item_image: torch.Tensor


def small_ratings(seed: int, empty_rows: bool = True
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """COO triples (int64 users, int64 items, fp32 values in 1..5) over
    NUM_USERS x NUM_ITEMS, about 2,700 unique cells (2,698 for seed 11) in
    shuffled order, with
    the properties listed at the top of this module; all of them are
    asserted here.  ``empty_rows=False`` gives every entity of EMPTY_USERS /
    EMPTY_ITEMS one entry."""
    g = torch.Generator().manual_seed(seed)
    live_items = torch.tensor([i for i in range(NUM_ITEMS)
                               if i not in EMPTY_ITEMS])
    cell = torch.zeros(NUM_USERS, NUM_ITEMS, dtype=torch.bool)
    for u in range(NUM_USERS):
        if u in EMPTY_USERS:
            continue
        n = EDGE_USERS.get(u) or int(torch.randint(6, 26, (1,), generator=g))
        pick = live_items[torch.randperm(live_items.numel(), generator=g)[:n]]
        cell[u, pick] = True
    ordinary = torch.tensor([u for u in range(NUM_USERS)
                             if u not in EMPTY_USERS and u not in EDGE_USERS])
    heavy = ordinary[torch.randperm(ordinary.numel(), generator=g)[:135]]
    cell[heavy, HEAVY_ITEM] = True
    if not empty_rows:
        for n, u in enumerate(EMPTY_USERS):
            cell[u, 20 + n] = True
        for n, i in enumerate(EMPTY_ITEMS):
            cell[40 + n, i] = True
    users, items = cell.nonzero(as_tuple=True)
    shuffle = torch.randperm(users.numel(), generator=g)
    users, items = users[shuffle], items[shuffle]
    vals = torch.randint(1, 6, (users.numel(),), generator=g).float()
    check_small_ratings(users, items, vals, empty_rows)
    return users, items, vals


def check_small_ratings(users, items, vals, empty_rows: bool = True) -> None:
    """The properties the parity tests rely on."""
    for n in (NUM_USERS, NUM_ITEMS):
        assert all(n % d for d in (3, 4, 7, 16)), n
    assert 2000 <= users.numel() <= 3000
    assert int(users.min()) >= 0 and int(users.max()) < NUM_USERS
    assert int(items.min()) >= 0 and int(items.max()) < NUM_ITEMS
    key = users * NUM_ITEMS + items
    assert torch.unique(key).numel() == key.numel(), "cells must be unique"
    assert bool(((vals >= 1) & (vals <= 5) & (vals == vals.round())).all())
    ucount = torch.bincount(users, minlength=NUM_USERS)
    icount = torch.bincount(items, minlength=NUM_ITEMS)
    if empty_rows:
        assert len(EMPTY_USERS) >= 2 and len(EMPTY_ITEMS) >= 2
        assert {0, NUM_USERS - 1} <= set(EMPTY_USERS)
        assert NUM_ITEMS - 1 in EMPTY_ITEMS
        assert (ucount == 0).nonzero().flatten().tolist() == list(EMPTY_USERS)
        assert (icount == 0).nonzero().flatten().tolist() == list(EMPTY_ITEMS)
    else:
        assert int(ucount.min()) >= 1 and int(icount.min()) >= 1
    for u, n in EDGE_USERS.items():
        assert int(ucount[u]) == n, (u, int(ucount[u]))
    assert int(icount[HEAVY_ITEM]) >= HEAVY_ITEM_MIN
    # the stored order inside a row is not sorted by column: the kernels
    # must take each row as stored
    assert bool((key[1:] < key[:-1]).any())


def als_config(cfg: Cfg) -> ALSConfig:
    return ALSConfig(iterations=STEPS, num_factors=cfg.k, lambda_=REG,
                     seed=42, dtype=torch.bfloat16,
                     factor_dtype="fp8" if cfg.gather == "fp8" else "bf16",
                     overlap_exchange=cfg.mode, exchange_chunks=cfg.chunks,
                     implicit_prefs=cfg.implicit, alpha=ALPHA)


def run_trainer(device, cfg: Cfg, triples, steps: int = STEPS):
    """Step a single-process trainer on ``device``.  Returns (trainer, the
    initial item image, one Record per step)."""
    users, items, vals = triples
    ctx = DistContext(rank=0, world_size=1, local_rank=0,
                      device=torch.device(device))
    tr = ALSTrainer(als_config(cfg), ctx)
    tr.setup(users, items, vals, NUM_USERS, NUM_ITEMS)
    image0 = tr.item_shard.clone()
    records = []
    for _ in range(steps):
        tr.step()
        records.append(Record(tr.user_f32.clone(), tr.item_f32.clone(),
                              tr.user_shard.clone(), tr.item_shard.clone()))
    return tr, image0, records


def _image(x: torch.Tensor, gather: str) -> torch.Tensor:
    return ops.quantize_fp8(x) if gather == "fp8" else x.to(torch.bfloat16)


def side_csrs(triples, device):
    """(user CSR, item CSR) with global column ids, rows as stored."""
    users, items, vals = triples
    ucsr = csr_from_coo(users, items.to(torch.int32), vals,
                        NUM_USERS, NUM_ITEMS).to(device)
    icsr = csr_from_coo(items, users.to(torch.int32), vals,
                        NUM_ITEMS, NUM_USERS).to(device)
    return ucsr, icsr


def replay(device, cfg: Cfg, triples, item_image0: torch.Tensor,
           steps: int = STEPS) -> List[Record]:
    """The reference chain.  Only the triples, the config and the initial
    item image go in: per half-iteration ONE flat ``als_solve_side`` call
    without a launch schedule, an output image or slabs; the next image is
    the host conversion of the fp32 result."""
    ucsr, icsr = side_csrs(triples, device)

    def half(csr, image_in):
        kw = {}
        if cfg.implicit:
            scale, ext = ops.implicit_weights(csr.values, ALPHA)
            kw = dict(scale=scale, ext=ext, base=ops.factor_gram(image_in))
        x = ops.als_solve_side(csr, image_in, REG, **kw)
        return x, _image(x, cfg.gather)

    out = []
    item_image = item_image0
    for _ in range(steps):
        ux, user_image = half(ucsr, item_image)
        ix, item_image = half(icsr, user_image)
        out.append(Record(ux, ix, user_image, item_image))
    return out


def bits(t: torch.Tensor) -> torch.Tensor:
    """Bit pattern: fp32 as int32 (NaN and the sign of a zero count),
    bf16 / e4m3 images as bytes."""
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 \
        else t.view(torch.uint8)


def assert_same_bits(got: torch.Tensor, want: torch.Tensor, what: str
                     ) -> None:
    """``torch.equal`` on bit patterns; the message names the first
    (row, column) that differs."""
    assert got.shape == want.shape and got.dtype == want.dtype, \
        (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = bits(got), bits(want)
    if torch.equal(g, w):
        return
    bad = (g != w).nonzero()
    r, c = (int(v) for v in bad[0][:2])
    per = g.shape[1] // got.shape[1]        # bytes per image element
    raise AssertionError(
        f"{what}: {bad.shape[0]} differing words, first at row {r} column "
        f"{c // per}: got {got[r, c // per].item()!r}, want "
        f"{want[r, c // per].item()!r}")


def assert_records_equal(got: List[Record], want: List[Record], what: str
                         ) -> None:
    assert len(got) == len(want)
    for step, (a, b) in enumerate(zip(got, want), 1):
        for name in Record._fields:
            assert_same_bits(getattr(a, name), getattr(b, name),
                             f"{what}, step {step}, {name}")


def assert_record_shape(rec: Record, cfg: Cfg, triples, what: str) -> None:
    """What must hold of every recorded state whatever the mode: padded
    columns are 0, entities without entries are all-zero bytes, and the
    images are the RNE images of the fp32 factors."""
    users, items, _ = triples
    k = cfg.k
    for side, x, img, ids, n in (
            ("user", rec.user_f32, rec.user_image, users, NUM_USERS),
            ("item", rec.item_f32, rec.item_image, items, NUM_ITEMS)):
        tag = f"{what}, {side}"
        assert x.dtype == torch.float32 and x.shape[0] == n, tag
        assert img.shape == x.shape, (tag, img.shape, x.shape)
        assert bool((x[:, k:] == 0).all()), f"{tag}: padded factor columns"
        assert bool((img[:, k:].float() == 0).all()), \
            f"{tag}: padded image columns"
        empty = (torch.bincount(ids, minlength=n) == 0).to(x.device)
        assert bool((bits(x)[empty] == 0).all()), f"{tag}: empty rows"
        assert bool((bits(img)[empty] == 0).all()), f"{tag}: empty rows"
        assert_same_bits(img, _image(x, cfg.gather), f"{tag}: image of x")
