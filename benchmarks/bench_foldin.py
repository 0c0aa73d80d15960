"""ALS fold-in: the live-item Gram refresh and the store's fold-in calls.

Part (a), the ``G0`` refresh.  Three ways to get ``sum v v^T`` over a row
list of a bf16 item table [items][64], alternating inside one process after
a warm-up of every shape, each call timed with device events:

  rows     ops.factor_gram(V, rows=rows)            (k_factor_gram<ROWS>:
                                                     reads the table in place)
  compact  ops.factor_gram(V.index_select(0, rows)) (a second table, the
                                                     compaction timed)
  torch    V[rows].float().T @ V[rows].float()      (fp32 copy + matmul)

Items 59,047 (the MovieLens-25M item count) and 2,000,000 (the bulk-ingest
benchmark size); row lists: every row, and every second row.  The ``rows``
call includes the wrapper's range check of the list (a min and a max over
it, as ``topk_scores`` does for ``cand``).  Printed per shape: the bytes the
row-list kernel must read (the listed rows and the int32 list) and the HBM
floor of reading them once.

Part (b), ``ALSModelStore.fold_in`` / ``fold_in_recommend`` end to end on a
59,047-item rank-64 store: 1, 64 and 1,024 baskets of 20 and 200 entries,
explicit and implicit, timed with a host clock around the call (which ends
in a device-to-host copy of the result, so in a synchronise).  The item Gram
is cached by the warm-up call; its refresh is part (a).

One JSON line per shape, then markdown tables.

    PYTHONPATH=. python benchmarks/bench_foldin.py [--quick] [--reps N]
"""

import argparse
import json
import sys
import time

import torch

from flink_ms_amd import ops
from flink_ms_amd.serving import ALSModelStore

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec
K = 64


def _event_ms(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _median(t):
    return sorted(t)[len(t) // 2]


def gram_refresh(dev, g, sizes, reps_arg):
    results = []
    for items in sizes:
        V = (torch.randn(items, K, generator=g) * 0.3).to(torch.bfloat16
                                                          ).to(dev)
        for name, step in (("all", 1), ("every-2nd", 2)):
            rows64 = torch.arange(0, items, step, device=dev)
            rows = rows64.to(torch.int32)
            variants = {
                "rows": lambda: ops.factor_gram(V, rows=rows),
                "compact": lambda: ops.factor_gram(
                    V.index_select(0, rows64)),
                "torch": lambda: V[rows64].float().T @ V[rows64].float(),
            }
            reps = reps_arg or (20 if items < 1_000_000 else 7)
            for fn in variants.values():          # warm-up, every variant
                fn()
                fn()
            torch.cuda.synchronize()
            samples = {n: [] for n in variants}
            for _ in range(reps):                 # alternate the variants
                for n, fn in variants.items():
                    samples[n].append(_event_ms(fn))
            med = {n: _median(t) for n, t in samples.items()}
            G = variants["rows"]()
            same = torch.equal(G, variants["compact"]())
            ref = variants["torch"]()
            rel = float((G - ref).abs().max() / ref.abs().max())
            nlist = int(rows.numel())
            need = nlist * (K * 2 + 4)
            rec = {
                "part": "gram", "items": items, "k": K, "list": name,
                "nlist": nlist,
                "rows_ms": round(med["rows"], 4),
                "compact_ms": round(med["compact"], 4),
                "torch_ms": round(med["torch"], 4),
                "rows_min_ms": round(min(samples["rows"]), 4),
                "compact_min_ms": round(min(samples["compact"]), 4),
                "torch_min_ms": round(min(samples["torch"]), 4),
                "fastest": min(med, key=med.get),
                "bit_equal_to_compact": same,
                "rel_diff_vs_torch": rel,
                "bytes_needed": need,
                "rows_gbps": round(need / (med["rows"] * 1e-3) / 1e9, 1),
                "hbm_floor_ms": round(need / HBM_PEAK * 1e3, 5),
                "reps": reps,
            }
            print(json.dumps(rec), flush=True)
            results.append(rec)
    return results


def store_fold_in(dev, g, items, reps_arg):
    store = ALSModelStore(device=dev)
    store.attach_factors(torch.randn(4, K, generator=g) * 0.3,
                         torch.randn(items, K, generator=g) * 0.3)
    results = []
    for nb in (1, 64, 1024):
        for per in (20, 200):
            picks = torch.stack([torch.randperm(items, generator=g)[:per]
                                 for _ in range(nb)]).tolist()
            vals = torch.randint(1, 6, (nb, per), generator=g).tolist()
            baskets = [[(str(i), float(v)) for i, v in zip(p, vv)]
                       for p, vv in zip(picks, vals)]
            for mode, kw in (("explicit", {}),
                             ("implicit", dict(implicit=True, alpha=10.0))):
                calls = {
                    "fold_in": lambda: store.fold_in(baskets, 0.1, **kw),
                    "fold_in_recommend": lambda: store.fold_in_recommend(
                        baskets, 10, 0.1, **kw),
                }
                reps = reps_arg or (7 if nb * per < 100_000 else 3)
                for fn in calls.values():
                    fn()
                torch.cuda.synchronize()
                samples = {n: [] for n in calls}
                for _ in range(reps):
                    for n, fn in calls.items():
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        samples[n].append((time.perf_counter() - t0) * 1e3)
                rec = {"part": "store", "items": items, "k": K,
                       "baskets": nb, "entries": per, "mode": mode,
                       "fold_in_ms": round(_median(samples["fold_in"]), 3),
                       "fold_in_recommend_ms": round(
                           _median(samples["fold_in_recommend"]), 3),
                       "reps": reps}
                print(json.dumps(rec), flush=True)
                results.append(rec)
    return results


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true",
                    help="59,047 items only")
    ap.add_argument("--reps", type=int, default=0,
                    help="timed calls per variant (default: by shape)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_foldin needs a GPU: nothing measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    sizes = (59_047,) if args.quick else (59_047, 2_000_000)
    gram = gram_refresh(dev, g, sizes, args.reps)
    fold = store_fold_in(dev, g, 59_047, args.reps)
    print("\n| items | list | rows ms | compact ms | torch ms | fastest | "
          "needed MB | rows GB/s | HBM floor ms | = compact |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in gram:
        print(f"| {r['items']:,} | {r['list']} | {r['rows_ms']:.3f} | "
              f"{r['compact_ms']:.3f} | {r['torch_ms']:.3f} | {r['fastest']} "
              f"| {r['bytes_needed'] / 1e6:.1f} | {r['rows_gbps']:.0f} | "
              f"{r['hbm_floor_ms']:.4f} | "
              f"{'yes' if r['bit_equal_to_compact'] else 'NO'} |")
    print("\n| baskets | entries | mode | fold_in ms | fold_in_recommend ms |")
    print("|---|---|---|---|---|")
    for r in fold:
        print(f"| {r['baskets']} | {r['entries']} | {r['mode']} | "
              f"{r['fold_in_ms']:.2f} | {r['fold_in_recommend_ms']:.2f} |")
    return 0 if all(r["bit_equal_to_compact"] for r in gram) else 2


if __name__ == "__main__":
    sys.exit(main())
