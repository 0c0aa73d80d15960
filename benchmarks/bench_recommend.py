"""Top-N recommendation kernel vs the unfused torch baseline.

Times ``ops.topk_scores`` (fused score + top-k, topk_kernels.hip) against

  f32   torch.topk(Q.float() @ V.float().T, n)      ([nq, items] fp32 in HBM)
  bf16  torch.topk(Q @ V.T, n)                      (bf16 matmul and scores)

on the same device and inputs: the three alternate inside one process after
a warm-up of every shape, each call timed with device events.  Shapes:
items 59,047 (the MovieLens-25M item count) and 2,000,000 (the bulk-ingest
benchmark size) x rank 64; batches 1, 64, 1024; n 10 and 100.

The fused result is checked against the f32 baseline's set: every returned
row must score (in the baseline's own matrix) within the two kernels' fp32
accumulation bounds of the baseline's n-th score.  Also printed per shape:
the bytes the fused kernel reads from V (once per 16-query tile) and the
HBM floor of reading V once.  One JSON line per shape, then a markdown table.

    PYTHONPATH=. python benchmarks/bench_recommend.py [--quick] [--reps N]
"""

import argparse
import json
import sys

import torch

from flink_ms_amd import ops

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec
K = 64


def _time_ms(fn, reps):
    """Per-call device time of ``fn``: median and minimum over ``reps``."""
    times = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0]


def _check(Q, V32, n, rows):
    """Fused rows vs the f32 baseline's set, per query, under the sum of the
    two fp32 accumulation bounds 2 k 2^-24 sum|q v| (max over the items)."""
    S = Q.float() @ V32.T
    base = torch.topk(S, n).values[:, -1]
    tol = 4 * K * 2.0 ** -24 * (Q.float().abs() @ V32.abs().T).max(dim=1).values
    ours = S.gather(1, rows)
    distinct = all(len(set(r)) == n for r in rows[:64].tolist())
    return bool((ours.min(dim=1).values >= base - tol).all()) and distinct


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true",
                    help="59,047 items only")
    ap.add_argument("--reps", type=int, default=0,
                    help="timed calls per variant (default 20, 7 at 2M)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_recommend needs a GPU: nothing measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    results = []
    for items in (59_047,) if args.quick else (59_047, 2_000_000):
        V = (torch.randn(items, K, generator=g) * 0.3).to(torch.bfloat16
                                                          ).to(dev)
        V32 = V.float()
        for nq in (1, 64, 1024):
            Q = (torch.randn(nq, K, generator=g) * 0.3).to(torch.bfloat16
                                                           ).to(dev)
            for n in (10, 100):
                variants = {
                    "fused": lambda: ops.topk_scores(Q, V, n),
                    "f32": lambda: torch.topk(Q.float() @ V32.T, n),
                    "bf16": lambda: torch.topk(Q @ V.T, n),
                }
                reps = args.reps or (20 if items < 1_000_000 else 7)
                for fn in variants.values():      # warm-up, every variant
                    fn()
                    fn()
                torch.cuda.synchronize()
                # alternate the variants: one timed call each per round
                samples = {name: [] for name in variants}
                for _ in range(reps):
                    for name, fn in variants.items():
                        samples[name].append(_time_ms(fn, 1)[0])
                med = {name: sorted(t)[len(t) // 2]
                       for name, t in samples.items()}
                best = {name: min(t) for name, t in samples.items()}
                _, rows = ops.topk_scores(Q, V, n)
                ok = _check(Q, V32, n, rows)
                v_bytes = items * K * 2
                tiles = (nq + 15) // 16
                rec = {
                    "items": items, "k": K, "batch": nq, "n": n,
                    "fused_ms": round(med["fused"], 4),
                    "f32_ms": round(med["f32"], 4),
                    "bf16_ms": round(med["bf16"], 4),
                    "fused_min_ms": round(best["fused"], 4),
                    "f32_min_ms": round(best["f32"], 4),
                    "bf16_min_ms": round(best["bf16"], 4),
                    "speedup_vs_f32": round(med["f32"] / med["fused"], 3),
                    "speedup_vs_bf16": round(med["bf16"] / med["fused"], 3),
                    "matches_f32_set": ok,
                    "chunk_items": ops.topk_chunk_items(nq, items, n),
                    "v_bytes_read": v_bytes * tiles,
                    "v_read_gbps": round(v_bytes * tiles
                                         / (med["fused"] * 1e-3) / 1e9, 1),
                    "hbm_floor_ms": round(v_bytes / HBM_PEAK * 1e3, 5),
                    "reps": reps,
                }
                print(json.dumps(rec), flush=True)
                results.append(rec)
    print("\n| items | batch | n | fused ms | f32 ms | bf16 ms | vs f32 | "
          "vs bf16 | V read MB | HBM floor ms | set ok |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        print(f"| {r['items']:,} | {r['batch']} | {r['n']} | "
              f"{r['fused_ms']:.3f} | {r['f32_ms']:.3f} | {r['bf16_ms']:.3f} "
              f"| {r['speedup_vs_f32']:.2f}x | {r['speedup_vs_bf16']:.2f}x | "
              f"{r['v_bytes_read'] / 1e6:.1f} | {r['hbm_floor_ms']:.4f} | "
              f"{'yes' if r['matches_f32_set'] else 'NO'} |")
    return 0 if all(r["matches_f32_set"] for r in results) else 2


if __name__ == "__main__":
    sys.exit(main())
