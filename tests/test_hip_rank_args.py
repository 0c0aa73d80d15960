"""Argument validation of the ``rank_counts`` binding (bindings.cpp).

Same pattern as test_hip_topk_args.py: the CPU part runs wherever the
extension is built (metadata checks first, the device check last); the GPU
part passes arguments that are wrong in a way that could not read or write
out of bounds even without the check.  ``rank_counts`` allocates its own
outputs and workspace, so "nothing was written" is checked on what the
caller does own: every tensor handed in keeps its sentinel fill.
"""

import pytest
import torch

from flink_ms_amd import ops

if not ops.hip_available():
    pytest.skip("HIP extension not built", allow_module_level=True)

import flink_ms_amd._hip_ops as hip  # noqa: E402

NQ, NV, K, P = 5, 40, 16, 7


def _args(device, k=K):
    return dict(
        Q=torch.full((NQ, k), 2.0, dtype=torch.bfloat16, device=device),
        V=torch.full((NV, k), 3.0, dtype=torch.bfloat16, device=device),
        T=torch.full((P, k), 3.0, dtype=torch.bfloat16, device=device),
        q_idx=torch.arange(P, dtype=torch.int64, device=device) % NQ,
        skip=torch.arange(P, dtype=torch.int64, device=device) * 2,
        cand=torch.arange(0, NV, 2, dtype=torch.int64, device=device),
        excl_ptr=torch.arange(NQ + 1, dtype=torch.int64, device=device),
        excl_rows=torch.arange(NQ, dtype=torch.int64, device=device) * 2,
        chunk_items=0)


def _call(a, st=0):
    return hip.rank_counts(a["Q"], a["V"], a["T"], a["q_idx"], a["skip"],
                           a["cand"], a["excl_ptr"], a["excl_rows"],
                           a["chunk_items"], st)


def _wider(t):
    return t.float() if t.dtype == torch.bfloat16 else t.double()


def _bad_cases(device):
    """(name, argument dict, expected message) for every rejected shape."""
    cases = []

    def case(name, match, **change):
        a = _args(device)
        a.update(change)
        cases.append((name, a, match))

    good = _args(device)
    for name in ("Q", "V", "T", "q_idx", "skip", "cand", "excl_ptr",
                 "excl_rows"):
        case(f"dtype-{name}", f"{name} must be", **{name: _wider(good[name])})
    for name in ("Q", "V", "T"):
        wide = torch.full((good[name].shape[0], 2 * K), 1.0,
                          dtype=torch.bfloat16, device=device)
        case(f"noncontig-{name}", f"{name} must be contiguous",
             **{name: wide[:, ::2]})
    for name in ("q_idx", "skip"):
        case(f"noncontig-{name}", f"{name} must be contiguous",
             **{name: torch.zeros(2 * P, dtype=torch.int64,
                                  device=device)[::2]})
        for n in (P - 1, P + 1):
            case(f"{name}-len-{n}", f"{name} must be 1-D with P",
                 **{name: torch.zeros(n, dtype=torch.int64, device=device)})
    case("T-rows", "q_idx must be 1-D with P",
         T=torch.full((P + 1, K), 3.0, dtype=torch.bfloat16, device=device))
    case("noncontig-cand", "cand must be contiguous",
         cand=torch.arange(NV, dtype=torch.int64, device=device)[::2])
    case("rank-mismatch", "rank mismatch",
         V=torch.full((NV, 2 * K), 3.0, dtype=torch.bfloat16, device=device))
    case("T-rank-mismatch", "rank mismatch",
         T=torch.full((P, 2 * K), 3.0, dtype=torch.bfloat16, device=device))
    case("Q-1d", "must be 2-D", Q=good["Q"].reshape(-1))
    case("cand-2d", "cand must be 1-D", cand=good["cand"].reshape(2, -1))
    case("chunk-negative", "chunk_items must be", chunk_items=-16)
    wide = {n: torch.full((r, 129), 2.0, dtype=torch.bfloat16, device=device)
            for n, r in (("Q", NQ), ("V", NV), ("T", P))}
    case("k-129", "rank k = 129 must be in 1..128", **wide)
    for n in (NQ, NQ + 2):
        case(f"excl_ptr-len-{n}", "excl_ptr must be 1-D with nq",
             excl_ptr=torch.zeros(n, dtype=torch.int64, device=device))
    case("excl_rows-alone", "excl_rows given without excl_ptr",
         excl_ptr=torch.empty(0, device=device))
    return cases


# ------------------------------------------------------------- CPU part

def test_cpu_tensors_are_rejected_last():
    with pytest.raises(RuntimeError, match="rank_counts: Q must be on the GPU"):
        _call(_args("cpu"))


@pytest.mark.parametrize("name", [c[0] for c in _bad_cases("cpu")])
def test_cpu_bad_arguments_raise(name):
    """Metadata checks run before the device check."""
    (a, match), = [(a, m) for n, a, m in _bad_cases("cpu") if n == name]
    with pytest.raises(RuntimeError) as ei:
        _call(a)
    assert "rank_counts" in str(ei.value) and match in str(ei.value)


def test_chunk_items_helper():
    assert hip.rank_chunk_items(1, 100) == 512              # the floor
    c = hip.rank_chunk_items(16, 2_000_000)
    assert c % 16 == 0 and 1024 < -(-2_000_000 // c) <= 2048
    assert hip.rank_chunk_items(8192, 2_000_000) >= c
    # more pair tiles than waves wanted: one chunk, whole 16-row tiles
    assert hip.rank_chunk_items(162_541, 59_047) == 59_056
    assert ops.rank_chunk_items(16, 2_000_000) == c
    for bad in ((0, 10), (1, 0), (-1, 10), (1, 1 << 31)):
        assert hip.rank_chunk_items(*bad) == -1
        with pytest.raises(ValueError):
            ops.rank_chunk_items(*bad)


# ------------------------------------------------------------- GPU part

@pytest.mark.gpu
def test_gpu_bad_arguments_raise_and_write_nothing():
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for name, a, match in _bad_cases(dev):
        before = {n: t.clone() for n, t in a.items()
                  if isinstance(t, torch.Tensor)}
        with pytest.raises(RuntimeError) as ei:
            _call(a, st)
        assert match in str(ei.value), name
        torch.cuda.synchronize()
        for n, t in before.items():
            assert torch.equal(a[n], t), (name, n)


@pytest.mark.gpu
def test_gpu_good_arguments_run_and_keep_inputs():
    dev = torch.device("cuda:0")
    a = _args(dev)
    before = {n: t.clone() for n, t in a.items()
              if isinstance(t, torch.Tensor)}
    greater, equal, score = _call(a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert greater.shape == equal.shape == score.shape == (P,)
    assert greater.dtype == equal.dtype == torch.int64
    assert score.dtype == torch.float32
    # every score is 2 * 3 * K: all 20 candidates tie, less the skip row
    # 2 p and, for query q = p % NQ, the excluded row 2 q
    assert torch.equal(score.cpu(), torch.full((P,), 6.0 * K))
    assert greater.cpu().tolist() == [0] * P
    want = [20 - len({2 * p, 2 * (p % NQ)}) for p in range(P)]
    assert equal.cpu().tolist() == want
    for n, t in before.items():
        assert torch.equal(a[n], t), n
