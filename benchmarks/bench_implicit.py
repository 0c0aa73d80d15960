"""ms/iteration of implicit-feedback ALS against explicit ALS.

ML-25M shape, rank 64 by default, fp8 and bf16 factor storage.  The explicit
and the implicit trainer live in ONE process and alternate: three
interleaved rounds of ``--iters`` iterations each, timed with device events,
so clock and thermal drift hit both alike.  The factor Gram kernel
(``ops.factor_gram``, two launches per implicit iteration plus the reduce)
is timed on its own.  Prints one JSON line.

    python benchmarks/bench_implicit.py [--iters 50] [--rounds 3]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from flink_ms_amd import ops
from flink_ms_amd.data.ratings import ML25M_SHAPE, RatingsShape, synthetic_ratings
from flink_ms_amd.models.als import ALSConfig, ALSTrainer


def _timed(fn, n):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / n


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--rank", type=int, default=64)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--alpha", type=float, default=1.0)
    p.add_argument("--lambda", dest="lambda_", type=float, default=0.9)
    p.add_argument("--ratings", type=int, default=ML25M_SHAPE.num_ratings)
    p.add_argument("--users", type=int, default=ML25M_SHAPE.num_users)
    p.add_argument("--items", type=int, default=ML25M_SHAPE.num_items)
    args = p.parse_args(argv)
    assert torch.cuda.is_available(), "bench_implicit needs a GPU"
    dev = torch.device("cuda:0")

    shape = RatingsShape(args.users, args.items, args.ratings)
    u, i, r = synthetic_ratings(shape, seed=42)
    out = {"shape": [args.users, args.items, args.ratings],
           "rank": args.rank, "alpha": args.alpha}
    for fd in ("fp8", "bf16"):
        trainers = {}
        for name, implicit in (("explicit", False), ("implicit", True)):
            tr = ALSTrainer(ALSConfig(
                num_factors=args.rank, lambda_=args.lambda_,
                factor_dtype=fd, implicit_prefs=implicit, alpha=args.alpha))
            tr.ctx.device = dev
            tr.setup(u.long(), i.long(), r, args.users, args.items)
            for _ in range(args.warmup):
                tr.step()
            trainers[name] = tr
        ms = {"explicit": [], "implicit": []}
        for _ in range(args.rounds):
            for name, tr in trainers.items():
                ms[name].append(_timed(tr.step, args.iters))
        tr = trainers["implicit"]
        gram = {side: _timed(lambda s=shard: ops.factor_gram(s), 200)
                for side, shard in (("items", tr.item_shard),
                                    ("users", tr.user_shard))}
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        out[fd] = {
            "ms_per_iteration": ms, "mean": mean,
            "implicit_over_explicit": mean["implicit"] / mean["explicit"],
            "factor_gram_ms_per_call": gram,
            "finite": bool(torch.isfinite(tr.model().user_factors).all()),
        }
        del trainers
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
