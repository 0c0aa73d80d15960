"""Implicit-feedback ALS over gloo (world_size = 2), same harness style as
test_distributed_cpu.py: the base matrix ``Y^T Y`` is each rank's own shard
Gram matrix summed over ranks, so it must equal the Gram matrix of the whole
table in every exchange mode (routed all-to-all-v, chunked overlap)."""

import multiprocessing as mp
import os

import pytest
import torch

WORLD = 2
NU, NI, K = 120, 60, 8
ALPHA, REG, ITERS = 10.0, 0.2, 3

_PORT_SALT = [0]


def _data():
    from _implicit_fixture import planted_implicit
    return planted_implicit(NU, NI, 10, 4, seed=21)


def _run_workers(target, extra=()):
    ctx = mp.get_context("spawn")
    _PORT_SALT[0] += 1
    port = 20000 + ((os.getpid() * 17 + _PORT_SALT[0] * 103) % 20000)
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(rank, WORLD, port, q, *extra))
             for rank in range(WORLD)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(WORLD):
        rank, payload = q.get(timeout=180)
        results[rank] = payload
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0, f"worker exit {p.exitcode}"
    return results


def _worker(rank, world, port, q, mode):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    torch.manual_seed(0)
    os.environ.update({
        "RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
        "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
    })
    import flink_ms_amd.parallel.dist as D
    D._CTX = None
    ctx = D.init_from_env(backend="gloo")
    from flink_ms_amd.models.als import ALSConfig, ALSTrainer
    u, i, r = _data()
    mask = torch.arange(u.numel()) % world == rank
    kw = (dict(routed_exchange="on") if mode == "routed"
          else dict(routed_exchange="off", overlap_exchange="auto",
                    exchange_chunks=3))
    cfg = ALSConfig(iterations=ITERS, num_factors=K, lambda_=REG,
                    dtype=torch.float32, implicit_prefs=True, alpha=ALPHA,
                    **kw)
    tr = ALSTrainer(cfg, ctx)
    tr.setup(u[mask].long(), i[mask].long(), r[mask], NU, NI)
    assert tr._overlap == (mode == "overlap")
    assert (tr.item_route is not None) == (mode == "routed")
    tr.fit()
    m = tr.model()
    # the base the NEXT user half-step would use: all ranks' item shards
    base = tr._weighted_kw(tr.user_w, tr.item_shard)["base"]
    q.put((rank, {
        "user_ids": m.user_ids.tolist(),
        "user_factors": m.user_factors.tolist(),
        "item_ids": m.item_ids.tolist(),
        "item_factors": m.item_factors.tolist(),
        "base": base.tolist(),
    }))
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode", ["routed", "overlap"])
def test_distributed_implicit_als(mode):
    from flink_ms_amd.models.als import ALSConfig, ALSTrainer
    from flink_ms_amd.ops import reference
    from _implicit_fixture import user_item_csr
    results = _run_workers(_worker, extra=(mode,))
    U = torch.zeros(NU, K)
    V = torch.zeros(NI, K)
    for rank in results:
        U[torch.tensor(results[rank]["user_ids"])] = torch.tensor(
            results[rank]["user_factors"])
        V[torch.tensor(results[rank]["item_ids"])] = torch.tensor(
            results[rank]["item_factors"])

    # every rank's base = Gram matrix of the concatenated item table
    g64 = reference.factor_gram_f64(V)
    v64 = V.double().abs()
    bound = 2 * NI * 2.0 ** -24 * (v64.T @ v64)
    for rank in results:
        base = torch.tensor(results[rank]["base"]).double()
        err = (base - g64).abs()
        print(f"rank {rank}: max base error {float(err.max()):.3e}, "
              f"min bound {float(bound.min()):.3e}")
        assert bool((err <= bound).all())
    assert torch.equal(torch.tensor(results[0]["base"]),
                       torch.tensor(results[1]["base"]))

    # quality: per-rank seeds differ, so the project's distributed
    # convention -- within 1.25x of the single-process objective
    u, i, r = _data()
    csr = user_item_csr(u, i, r, NU, NI)
    obj = reference.implicit_objective(csr, U, V, ALPHA, REG)
    import flink_ms_amd.parallel.dist as D
    D._CTX = None
    tr = ALSTrainer(ALSConfig(iterations=ITERS, num_factors=K, lambda_=REG,
                              dtype=torch.float32, implicit_prefs=True,
                              alpha=ALPHA))
    tr.ctx.device = torch.device("cpu")
    tr.setup(u.long(), i.long(), r, NU, NI)
    m = tr.fit()
    obj_sp = reference.implicit_objective(csr, m.user_factors,
                                          m.item_factors, ALPHA, REG)
    print(f"{mode}: distributed objective {obj:.6g}, single {obj_sp:.6g}")
    assert obj <= 1.25 * obj_sp
