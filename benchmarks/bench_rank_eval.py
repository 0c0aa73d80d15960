"""Rank-count kernel (K9) vs the unfused torch baseline.

Times, per shape, on the same device and inputs:

  fused  T = V[t_idx], then the rank_counts binding (k_rank_scan +
         k_rank_finish): what ops.rank_counts launches, without the
         wrapper's host-side checks
  ops    ops.rank_counts as a user calls it: the same plus the range,
         repeat and sort checks of q_idx / t_idx / the exclusion CSR (each
         a device reduction and a host sync)
  torch  bf16 S = Q[q_idx] @ V.T in blocks of pairs whose score block stays
         under 1 GiB; the exclusion scatter to -inf (flat indices built
         outside the timed window); compare with the gathered target; sum

alternating inside one process after a warm-up of every variant, each call
timed with device events; medians and minima.  Shapes: rank 64; 59,047
items (the MovieLens-25M item count) x 8,192 and 162,541 pairs (one per
ML-25M user); 2,000,000 items x 8,192 pairs; every user has about 150
excluded items.

Counts are compared where scores are exact: on factors in {-1, 0, 1} every
dot is an integer of at most 64, exact in the baseline's bf16 scores too,
and the two must agree on every pair.  Printed next to the times: the bytes
of V (HBM floor of reading it once) and the MFMA flops of the 16-pair tiles
(floor at the dense bf16 peak).  One JSON line per shape, then a markdown
table.

    PYTHONPATH=. python benchmarks/bench_rank_eval.py [--quick] [--reps N]
"""

import argparse
import json
import sys

import torch

from flink_ms_amd import ops

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E spec
MFMA_PEAK = 2.5e15         # flop/s, dense bf16 spec
K = 64
EXCL = 150
SCORE_BLOCK_BYTES = 1 << 30


def _event_ms(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _problem(items, pairs, dev, seed, exact):
    g = torch.Generator().manual_seed(seed)
    if exact:
        Q = torch.randint(-1, 2, (pairs, K), generator=g).float()
        V = torch.randint(-1, 2, (items, K), generator=g).float()
    else:
        Q = torch.randn(pairs, K, generator=g) * 0.3
        V = torch.randn(items, K, generator=g) * 0.3
    q_idx = torch.randperm(pairs, generator=g)        # one pair per user
    t_idx = torch.randint(0, items, (pairs,), generator=g)
    # per user about EXCL distinct ascending rows: a random start plus
    # strictly positive steps
    steps = torch.randint(1, items // (EXCL + 1), (pairs, EXCL), generator=g)
    rows = torch.cumsum(steps, 1) - 1
    ptr = torch.arange(pairs + 1, dtype=torch.int64) * EXCL
    return (Q.to(torch.bfloat16).to(dev), V.to(torch.bfloat16).to(dev),
            q_idx.to(dev), t_idx.to(dev), ptr.to(dev),
            rows.reshape(-1).contiguous().to(dev))


def _torch_plan(q_idx, ptr, ex, items):
    """Pair blocks and, per block, the flat (pair-in-block, row) scatter
    indices of its exclusions."""
    block = max(1, SCORE_BLOCK_BYTES // (2 * items))
    plan = []
    counts = ptr[1:] - ptr[:-1]
    for s in range(0, q_idx.numel(), block):
        q = q_idx[s:s + block]
        n = counts[q]
        local = torch.repeat_interleave(
            torch.arange(q.numel(), device=q.device), n)
        start = torch.repeat_interleave(ptr[q] - (torch.cumsum(n, 0) - n), n)
        src = start + torch.arange(local.numel(), device=q.device)
        plan.append((s, q, local * items + ex[src]))
    return plan


def _torch_counts(Q, V, t_idx, plan, items):
    greater = torch.empty(t_idx.numel(), dtype=torch.int64, device=Q.device)
    equal = torch.empty_like(greater)
    for s, q, flat in plan:
        S = Q[q] @ V.T                                  # [b, items] bf16
        t = t_idx[s:s + q.numel()].unsqueeze(1)
        ts = S.gather(1, t)
        S.view(-1)[flat] = -float("inf")
        S.scatter_(1, t, -float("inf"))                 # the target itself
        greater[s:s + q.numel()] = (S > ts).sum(1)
        equal[s:s + q.numel()] = (S == ts).sum(1)
    return greater, equal


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true",
                    help="59,047 items x 8,192 pairs only")
    ap.add_argument("--reps", type=int, default=10,
                    help="timed calls per variant")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_rank_eval needs a GPU: nothing measured",
              file=sys.stderr)
        return 1
    import flink_ms_amd._hip_ops as hip
    dev = torch.device("cuda:0")
    none = torch.empty(0, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

    # ---- same counts where scores are exact
    Q, V, q_idx, t_idx, ptr, ex = _problem(59_047, 8_192, dev, 1, exact=True)
    g, e, _ = ops.rank_counts(Q, V, q_idx, t_idx, exclude=(ptr, ex))
    bg, be = _torch_counts(Q, V, t_idx, _torch_plan(q_idx, ptr, ex, 59_047),
                           59_047)
    same = bool(torch.equal(g, bg) and torch.equal(e, be))
    print(json.dumps({"exact_case_counts_equal": same,
                      "pairs_with_ties": int((e > 0).sum())}), flush=True)

    shapes = [(59_047, 8_192)]
    if not args.quick:
        shapes += [(59_047, 162_541), (2_000_000, 8_192)]
    results = []
    for items, pairs in shapes:
        Q, V, q_idx, t_idx, ptr, ex = _problem(items, pairs, dev, 2,
                                               exact=False)
        plan = _torch_plan(q_idx, ptr, ex, items)
        variants = {
            "fused": lambda: hip.rank_counts(Q, V, V[t_idx], q_idx, t_idx,
                                             none, ptr, ex, 0, stream()),
            "ops": lambda: ops.rank_counts(Q, V, q_idx, t_idx,
                                           exclude=(ptr, ex)),
            "torch": lambda: _torch_counts(Q, V, t_idx, plan, items),
        }
        out = {}
        for name, fn in variants.items():              # warm-up
            fn()
            out[name] = fn()
        torch.cuda.synchronize()
        samples = {name: [] for name in variants}
        for _ in range(args.reps):                     # alternate
            for name, fn in variants.items():
                samples[name].append(_event_ms(fn)[0])
        med = {n: sorted(t)[len(t) // 2] for n, t in samples.items()}
        best = {n: min(t) for n, t in samples.items()}
        # real-valued scores: the bf16-rounded baseline may order close
        # scores differently; report how far apart the positions are
        fg, fe = out["fused"][0], out["fused"][1]
        tg, te = out["torch"]
        gap = ((fg + fe / 2) - (tg + te / 2)).abs()
        v_bytes = items * K * 2
        tiles = (pairs + 15) // 16
        flops = 2.0 * tiles * 16 * (items + EXCL * 16) * K
        rec = {
            "items": items, "pairs": pairs, "k": K, "excl_per_user": EXCL,
            "fused_ms": round(med["fused"], 4),
            "ops_ms": round(med["ops"], 4),
            "torch_ms": round(med["torch"], 4),
            "fused_min_ms": round(best["fused"], 4),
            "ops_min_ms": round(best["ops"], 4),
            "torch_min_ms": round(best["torch"], 4),
            "speedup_fused": round(med["torch"] / med["fused"], 3),
            "speedup_ops": round(med["torch"] / med["ops"], 3),
            "ops_equals_fused": bool(torch.equal(out["ops"][0], fg)
                                     and torch.equal(out["ops"][1], fe)),
            "mean_position_gap_vs_bf16_baseline": round(float(gap.mean()), 3),
            "chunk_items": ops.rank_chunk_items(pairs, items),
            "v_bytes": v_bytes,
            "hbm_floor_ms": round(v_bytes / HBM_PEAK * 1e3, 5),
            "mfma_flops": flops,
            "mfma_floor_ms": round(flops / MFMA_PEAK * 1e3, 5),
            "torch_pair_block": max(1, SCORE_BLOCK_BYTES // (2 * items)),
            "reps": args.reps,
        }
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del plan, variants, out
    print("\n| items | pairs | fused ms (min) | ops ms (min) | torch ms (min) "
          "| torch / fused | torch / ops | V MB | HBM floor ms | "
          "MFMA floor ms |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in results:
        print(f"| {r['items']:,} | {r['pairs']:,} | {r['fused_ms']:.3f} "
              f"({r['fused_min_ms']:.3f}) | {r['ops_ms']:.3f} "
              f"({r['ops_min_ms']:.3f}) | {r['torch_ms']:.3f} "
              f"({r['torch_min_ms']:.3f}) | {r['speedup_fused']:.2f}x | "
              f"{r['speedup_ops']:.2f}x | {r['v_bytes'] / 1e6:.1f} | "
              f"{r['hbm_floor_ms']:.4f} | {r['mfma_floor_ms']:.4f} |")
    ok = same and all(r["ops_equals_fused"] for r in results)
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
