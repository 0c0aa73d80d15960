"""Quality of the re-rounded operand in implicit-feedback ALS.

Planted block preferences (users of block b interact mostly with items of
block b), one interaction per user held out.  Trains 10 iterations three
ways from one init -- CPU fp32 (no rounding anywhere), GPU bf16, GPU fp8 --
and reports the float64 full-grid objective and the held-out mean
percentile rank (0 % = the held-out item is ranked first, 50 % = random;
Hu, Koren, Volinsky 2008).  Prints one JSON line.

    python benchmarks/implicit_quality.py [--users 6000 --items 2000]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from flink_ms_amd.data.blocked import csr_from_coo
from flink_ms_amd.models.als import ALSConfig, ALSTrainer
from flink_ms_amd.ops import reference


def planted(num_users, num_items, per_user, blocks, seed):
    g = torch.Generator().manual_seed(seed)
    users = torch.arange(num_users).repeat_interleave(per_user)
    in_block = torch.rand(users.numel(), generator=g) < 0.85
    within = torch.randint(0, num_items // blocks, (users.numel(),),
                           generator=g)
    anywhere = torch.randint(0, num_items, (users.numel(),), generator=g)
    items = torch.where(in_block, within * blocks + users % blocks, anywhere)
    r = torch.where(in_block,
                    torch.randint(1, 6, (users.numel(),), generator=g).float(),
                    torch.ones(users.numel()))
    key = users * num_items + items
    order = torch.argsort(key, stable=True)
    keep = torch.ones_like(key, dtype=torch.bool)
    keep[order[1:]] = key[order][1:] != key[order][:-1]
    return users[keep], items[keep], r[keep]


def mean_percentile_rank(U, V, hu, hi, seen):
    """Mean over held-out (user, item) pairs of the item's rank percentile
    among the items the user has not seen in training."""
    S = U[hu].double() @ V.double().T
    S[seen[hu]] = -float("inf")
    target = S.gather(1, hi.unsqueeze(1))
    better = (S > target).sum(dim=1).double()
    cand = (~seen[hu]).sum(dim=1).double()
    return float((better / (cand - 1).clamp_min(1)).mean() * 100.0)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--users", type=int, default=6000)
    p.add_argument("--items", type=int, default=2000)
    p.add_argument("--per-user", type=int, default=24)
    p.add_argument("--blocks", type=int, default=20)
    p.add_argument("--rank", type=int, default=32)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--alpha", type=float, default=10.0)
    p.add_argument("--lambda", dest="lambda_", type=float, default=0.1)
    args = p.parse_args(argv)

    u, i, r = planted(args.users, args.items, args.per_user, args.blocks, 5)
    # hold out each user's LAST in-block interaction
    last = torch.zeros(args.users, dtype=torch.int64)
    last[u] = torch.arange(u.numel())
    held = torch.zeros(u.numel(), dtype=torch.bool)
    held[last] = True
    held &= (i % args.blocks) == (u % args.blocks)
    tu, ti, trn = u[~held], i[~held], r[~held]
    hu, hi = u[held], i[held]
    seen = torch.zeros(args.users, args.items, dtype=torch.bool)
    seen[tu, ti] = True
    csr = csr_from_coo(tu, ti.to(torch.int32), trn, args.users, args.items)

    runs = [("cpu-fp32", torch.device("cpu"), dict(dtype=torch.float32))]
    if torch.cuda.is_available():
        gpu = torch.device("cuda:0")
        runs += [("gpu-bf16", gpu, dict(dtype=torch.bfloat16)),
                 ("gpu-fp8", gpu, dict(factor_dtype="fp8"))]
    out = {"users": args.users, "items": args.items, "train": int(tu.numel()),
           "held_out": int(hu.numel()), "rank": args.rank,
           "alpha": args.alpha, "lambda": args.lambda_, "iters": args.iters}
    for name, dev, kw in runs:
        tr = ALSTrainer(ALSConfig(iterations=args.iters,
                                  num_factors=args.rank,
                                  lambda_=args.lambda_, implicit_prefs=True,
                                  alpha=args.alpha, **kw))
        tr.ctx.device = dev
        tr.setup(tu.long(), ti.long(), trn, args.users, args.items)
        m = tr.fit()
        U, V = m.user_factors.float().cpu(), m.item_factors.float().cpu()
        out[name] = {
            "objective": reference.implicit_objective(
                csr, U, V, args.alpha, args.lambda_),
            "mean_percentile_rank": mean_percentile_rank(U, V, hu, hi, seen),
        }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
