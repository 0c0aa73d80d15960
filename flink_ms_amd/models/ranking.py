"""Ranking evaluation of a factor model (no reference analog; the reference
only has MSE.java).

For every held-out (user, item) pair ``ops.rank_counts`` gives the position
of the item among the user's unseen items as two counts -- ``g`` items score
strictly higher, ``e`` score the same -- without ever writing the [users,
items] score matrix.  Every metric below is float64 host arithmetic on those
counts.  Ties are taken in expectation: the target sits uniformly at the
0-based positions ``g .. g + e``.

``c`` is the number of items that compete with the target: all items, less
the user's training items, less the target itself.  Pairs with ``c == 0``
have no rank to speak of: they are counted in ``n_degenerate`` and left out
of the percentile means (mean percentile rank, AUC); the other metrics see
them at position 0.

  mean_percentile_rank  100 * mean((g + e/2) / c): Hu, Koren, Volinsky
                        2008; 0 % = always first, 50 % = random
  auc                   1 - mean((g + e/2) / c)
  hit_rate[n]           mean(clamp((n - g) / (e + 1), 0, 1))
  mrr                   mean((H[g+e+1] - H[g]) / (e + 1)), H the harmonic
                        numbers: the tie-averaged 1 / (position + 1)
  ndcg[n]               per user DCG / IDCG, averaged over the users with a
                        scored pair; DCG sums the tie-averaged
                        1 / log2(position + 2) over positions below n, IDCG
                        is that discount over min(m_u, n) positions, m_u the
                        user's number of scored pairs
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence

import torch

from .. import ops

# Pairs per ops.rank_counts call.  The kernel's own workspace is pairs x
# chunks x 16 bytes and a batch this size scans the catalogue in one chunk
# per 16-pair tile (4096 tiles > the launcher's 2048-wave target), so it is
# 1 MiB: the bound is the gathered bf16 target block (16 MiB at rank 128)
# and, on the CPU path, the reference's score blocks.  Larger batches buy
# nothing -- 4096 waves already fill the GPU sixteen deep.
PAIR_BATCH = 65536


@dataclass
class RankingResult:
    mean_percentile_rank: float
    auc: float
    mrr: float
    hit_rate: Dict[int, float] = field(default_factory=dict)
    ndcg: Dict[int, float] = field(default_factory=dict)
    n_scored: int = 0
    n_skipped: int = 0      # pairs whose user or item is missing
    n_degenerate: int = 0   # scored pairs with no competing item


def _rows(ids: torch.Tensor, index: Optional[torch.Tensor], n: int
          ) -> torch.Tensor:
    """Global ids -> factor rows, -1 where the model has none."""
    ids = ids.long().cpu()
    if index is None:
        return torch.where((ids >= 0) & (ids < n), ids,
                           torch.full_like(ids, -1))
    index = index.long().cpu()
    inside = (ids >= 0) & (ids < index.numel())
    out = torch.full_like(ids, -1)
    out[inside] = index[ids[inside]]
    return out


def evaluate_ranking(
    user_factors: torch.Tensor,   # [U, k]
    item_factors: torch.Tensor,   # [I, k]
    train_users: torch.Tensor,
    train_items: torch.Tensor,
    test_users: torch.Tensor,
    test_items: torch.Tensor,
    ns: Sequence[int] = (10,),
    user_index: Optional[torch.Tensor] = None,  # global id -> row (-1 missing)
    item_index: Optional[torch.Tensor] = None,
) -> RankingResult:
    dev = user_factors.device
    nu, ni = user_factors.shape[0], item_factors.shape[0]
    ns = [int(n) for n in ns]
    if any(n < 1 for n in ns):
        raise ValueError("every n must be >= 1")

    # exclusion CSR = the training pairs, per user sorted and deduplicated
    tu = _rows(train_users, user_index, nu)
    ti = _rows(train_items, item_index, ni)
    ok = (tu >= 0) & (ti >= 0)
    seen = torch.unique(tu[ok] * ni + ti[ok])             # sorted keys
    excl_ptr = torch.zeros(nu + 1, dtype=torch.int64)
    excl_ptr[1:] = torch.cumsum(
        torch.bincount(seen // ni, minlength=nu), 0)
    excl_rows = seen % ni

    u = _rows(test_users, user_index, nu)
    t = _rows(test_items, item_index, ni)
    ok = (u >= 0) & (t >= 0)
    n_skipped = int((~ok).sum())
    u, t = u[ok], t[ok]
    P = int(u.numel())
    nan = float("nan")
    if P == 0:
        return RankingResult(nan, nan, nan, {n: nan for n in ns},
                             {n: nan for n in ns}, 0, n_skipped, 0)

    exclude = (excl_ptr.to(dev), excl_rows.to(dev))
    greater = torch.empty(P, dtype=torch.int64)
    equal = torch.empty(P, dtype=torch.int64)
    for s in range(0, P, PAIR_BATCH):
        g, e, _ = ops.rank_counts(user_factors, item_factors,
                                  u[s:s + PAIR_BATCH].to(dev),
                                  t[s:s + PAIR_BATCH].to(dev),
                                  exclude=exclude)
        greater[s:s + PAIR_BATCH] = g.cpu()
        equal[s:s + PAIR_BATCH] = e.cpu()

    g, e = greater.double(), equal.double()
    n_seen = (excl_ptr[1:] - excl_ptr[:-1])[u]
    target_seen = torch.isin(u * ni + t, seen)
    c = (ni - n_seen - (~target_seen).long()).double()
    live = c > 0
    n_degenerate = int((~live).sum())
    if bool(live.any()):
        pct = float(((g[live] + e[live] / 2) / c[live]).mean())
    else:
        pct = nan

    top = int((greater + equal).max()) + 2
    H = torch.zeros(top, dtype=torch.float64)             # harmonic numbers
    H[1:] = torch.cumsum(1.0 / torch.arange(1, top, dtype=torch.float64), 0)
    mrr = float(((H[greater + equal + 1] - H[greater]) / (e + 1)).mean())

    hit_rate, ndcg = {}, {}
    users, inverse = torch.unique(u, return_inverse=True)
    m_u = torch.bincount(inverse, minlength=users.numel())
    for n in ns:
        hit_rate[n] = float(((n - g) / (e + 1)).clamp(0, 1).mean())
        # D[m] = sum of the discount over positions 0 .. m-1
        D = torch.zeros(n + 1, dtype=torch.float64)
        D[1:] = torch.cumsum(
            1.0 / torch.log2(torch.arange(n, dtype=torch.float64) + 2), 0)
        gain = (D[(greater + equal + 1).clamp(max=n)]
                - D[greater.clamp(max=n)]) / (e + 1)
        dcg = torch.zeros(users.numel(), dtype=torch.float64)
        dcg.index_add_(0, inverse, gain)
        ndcg[n] = float((dcg / D[m_u.clamp(max=n)]).mean())

    return RankingResult(100.0 * pct, 1.0 - pct, mrr, hit_rate, ndcg,
                         P, n_skipped, n_degenerate)
