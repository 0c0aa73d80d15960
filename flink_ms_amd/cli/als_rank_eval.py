"""Ranking evaluation job for ALS models (no reference analog; the
reference's only evaluator is evaluation/MSE.java).

Flags: --userFactors, --itemFactors (model text files, or directories of
part files, as written by als_train), --train (the ratings the model was
trained on: a user's training items do not compete with the held-out ones),
--input (the held-out ratings), --n (cut-offs of HR@n / NDCG@n, comma
separated, default 10), --fieldDelimiter (comma|tab or a literal character,
default comma), --ignoreFirstLine (true), --output (file for the JSON line).

Prints ONE JSON line: mean_percentile_rank, auc, mrr, hit_rate, ndcg,
scored, skipped (pairs whose user or item the model does not have) and
degenerate (pairs with no competing item).  The rating column is not used:
every row of --input is a held-out interaction.  Runs on the GPU when one is
present (fused score + rank-count kernel) and on the CPU otherwise.
"""

from __future__ import annotations

import json
import os
import sys
from typing import List, Tuple

import torch

from ..data.ratings import load_ratings_csv
from ..models.ranking import evaluate_ranking
from ..utils.params import Params
from ..utils.textio import MEAN_ID, parse_als_row


def _load_factors(path: str, kind: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """Model rows of ``kind`` -> (ids int64 [n], factors fp32 [n, k]); MEAN
    rows are cold-start defaults, not entities, and are left out."""
    paths = ([os.path.join(path, p) for p in sorted(os.listdir(path))]
             if os.path.isdir(path) else [path])
    ids: List[int] = []
    rows: List[List[float]] = []
    for p in paths:
        with open(p) as f:
            for line in f:
                if not line.strip():
                    continue
                eid, k, fac = parse_als_row(line)
                if k != kind or eid == MEAN_ID:
                    continue
                ids.append(int(eid))
                rows.append(fac)
    if not rows:
        raise ValueError(f"no {kind} rows in {path}")
    return (torch.tensor(ids, dtype=torch.int64),
            torch.tensor(rows, dtype=torch.float32))


def _index(ids: torch.Tensor, *others: torch.Tensor) -> torch.Tensor:
    """Global id -> factor row, -1 for ids the model does not have; long
    enough for every id of ``others``."""
    top = max(int(t.max()) for t in (ids, *others) if t.numel()) + 1
    index = torch.full((top,), -1, dtype=torch.int64)
    index[ids] = torch.arange(ids.numel())
    return index


def main(argv=None) -> int:
    params = Params.from_args(sys.argv[1:] if argv is None else argv)
    delim = params.get("fieldDelimiter", "comma")
    skip_header = params.get_bool("ignoreFirstLine", True)
    ns = [int(tok) for tok in str(params.get("n", "10")).split(",") if tok]
    uids, U = _load_factors(params.get_required("userFactors"), "U")
    iids, V = _load_factors(params.get_required("itemFactors"), "I")
    tu, ti, _ = load_ratings_csv(params.get_required("train"), delim,
                                 skip_header)
    hu, hi, _ = load_ratings_csv(params.get_required("input"), delim,
                                 skip_header)
    dev = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    if dev.type == "cuda":
        U, V = U.to(dev, torch.bfloat16), V.to(dev, torch.bfloat16)
    res = evaluate_ranking(
        U, V, tu.long(), ti.long(), hu.long(), hi.long(), ns=ns,
        user_index=_index(uids, tu.long(), hu.long()),
        item_index=_index(iids, ti.long(), hi.long()))
    line = json.dumps({
        "mean_percentile_rank": res.mean_percentile_rank,
        "auc": res.auc,
        "mrr": res.mrr,
        "hit_rate": {str(n): v for n, v in res.hit_rate.items()},
        "ndcg": {str(n): v for n, v in res.ndcg.items()},
        "scored": res.n_scored,
        "skipped": res.n_skipped,
        "degenerate": res.n_degenerate,
        "device": dev.type,
    })
    if params.has("output"):
        with open(params.get("output"), "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
