"""Checks shared by the fold-in tests (test_gpu_foldin.py on the GPU,
test_foldin_cpu.py through the references): the store's cached live-item
Gram, fold-in against the solve it is built on and against float64 oracles,
and fold-in recommendations against a brute-force ranking.  All on the
integer-factor store of _topk_store_fixture (imported, not edited).
"""

import pytest
import torch

import _topk_store_fixture as fx
from flink_ms_amd import ops
from flink_ms_amd.data.blocked import CSR
from flink_ms_amd.ops import reference as R

ULP32 = 2.0 ** -23
REG, ALPHA = 0.1, 4.0      # alpha*|r| is a power of 4: exact scaling in bf16

BASKETS = [
    # two sources, a shadowed id (11: the mirror value counts) and an
    # unknown id
    [("12", 1.0), ("31", 4.0), ("20", 1.0), ("11", 16.0), ("999", 1.0)],
    [("13", 4.0)],
    [("777", 1.0)],                          # nothing resolves
    [(item, 1.0) for item in fx.LIVE],       # every live item
]
USED = [4, 1, 0, 22]
MODES = ("explicit", "implicit")


def _kw(mode):
    return dict(implicit=True, alpha=ALPHA) if mode == "implicit" else {}


# ---------------------------------------------------------------- G0

def live_gram_exact(store, items):
    """fp32 Gram of the bf16 images of the store's current vectors of
    ``items``, with a float64 check that every sum is exact in fp32 -- so
    the expected matrix does not depend on the order of the additions."""
    V = torch.tensor([store.get_vector(f"{i}-I") for i in items],
                     dtype=torch.float32).to(torch.bfloat16).double()
    G = V.T @ V
    assert torch.equal(G.float().double(), G)
    # every entry is a multiple of 2^-7, so every product and partial sum is
    # a multiple of 2^-14, and below 2^-14 * 2^24 in magnitude: exact
    absum = V.abs().T @ V.abs()
    assert torch.equal((V * 128).round(), V * 128)
    assert float(absum.max()) < 2.0 ** 10
    return G.float()


def check_store_gram(device):
    store = fx.build_store(device)
    live = dict(fx.LIVE)
    want = torch.zeros(4, 4)
    for m in live.values():
        d = torch.tensor(fx.digits(m))
        want += d.unsqueeze(1) * d.unsqueeze(0)
    assert len(live) == 22
    G = store._item_gram()
    assert G.dtype == torch.float32 and G.shape == (4, 4)
    assert torch.equal(G.cpu(), want), G
    assert torch.equal(G.cpu(), live_gram_exact(store, live))
    assert store._item_gram() is G                  # cached
    # every writer of an item row's device values invalidates the cache
    store.ingest_row("30,I," + ";".join(str(x) for x in fx.digits(5)))
    assert store._item_gram() is not G
    assert torch.equal(store._item_gram().cpu(), live_gram_exact(store, live))
    assert not torch.equal(store._item_gram().cpu(), want)
    # user 5 (mirror) x item 12 (bulk block): err = 76 - 75 = 1, so the new
    # item row is v + u / 8, exact in bf16
    before = store._item_gram()
    batched, scalar, _ = store.sgd_update_batch(["5"], ["12"], [76.0],
                                                learning_rate=0.125)
    assert (batched, scalar) == (1, 0)
    assert store.get_vector("12-I") != fx.digits(fx.LIVE["12"])
    assert not torch.equal(store._item_gram(), before)
    assert torch.equal(store._item_gram().cpu(), live_gram_exact(store, live))
    # scalar SGD reaches ingest: item 33 lives in the mirror (err = 1 again)
    before = store._item_gram()
    dot = sum(a * b for a, b in zip(store.get_vector("5-U"),
                                    store.get_vector("33-I")))
    store.sgd_update("5", "33", dot + 1.0, learning_rate=0.125)
    assert not torch.equal(store._item_gram(), before)
    assert torch.equal(store._item_gram().cpu(), live_gram_exact(store, live))
    before = store._item_gram()
    store.attach_factors(torch.tensor([fx.USERS["3"]], dtype=torch.float32),
                         torch.tensor([fx.digits(77)]),
                         user_ids=torch.tensor([3]),
                         item_ids=torch.tensor([40]))
    live["40"] = 77
    assert not torch.equal(store._item_gram(), before)
    assert torch.equal(store._item_gram().cpu(), live_gram_exact(store, live))
    before = store._item_gram()
    store.ingest_bulk("41,I,1.0;0.0;2.0;0.0\n")
    live["41"] = 72
    assert not torch.equal(store._item_gram(), before)
    assert torch.equal(store._item_gram().cpu(), live_gram_exact(store, live))
    # the blocks' own in-place writer
    before = store._item_gram()
    assert store._blocks.update_row_("I", 40, [0.0, 3.0, 0.0, 1.0])
    assert not torch.equal(store._item_gram(), before)
    assert torch.equal(store._item_gram().cpu(), live_gram_exact(store, live))
    # a user row does not touch it
    before = store._item_gram()
    store.ingest_row("6,U,1.0;1.0;1.0;1.0")
    assert store._item_gram() is before


# ----------------------------------------------------------- fold-in

def compact_problem(store, baskets, device):
    """The compact problem fold_in must build, assembled from get_vector:
    (csr with indices = arange(nnz), table [nnz][k] bf16, used)."""
    rows, vals, used = [], [], []
    for basket in baskets:
        cnt = 0
        for item, value in basket:
            v = store.get_vector(f"{item}-I")
            if v is None:
                continue
            rows.append(v)
            vals.append(value)
            cnt += 1
        used.append(cnt)
    nnz = len(rows)
    indptr = torch.zeros(len(baskets) + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.tensor(used), 0)
    csr = CSR(indptr.to(device),
              torch.arange(nnz, dtype=torch.int32, device=device),
              torch.tensor(vals, dtype=torch.float32, device=device),
              len(baskets), nnz)
    table = torch.tensor(rows, dtype=torch.float32).to(torch.bfloat16)
    return csr, table.to(device), used


def direct_solve(store, csr, table, mode):
    if mode == "implicit":
        s, e = ops.implicit_weights(csr.values, ALPHA)
        return ops.als_solve_side(csr, table, REG, scale=s, ext=e,
                                  base=store._item_gram())
    return ops.als_solve_side(csr, table, REG)


def oracle_f64(store, baskets, mode):
    """Float64 over the live vectors: the dense Hu-Koren-Volinsky update
    (implicit) or the ridge solve (explicit)."""
    live = list(fx.LIVE)
    col = {item: j for j, item in enumerate(live)}
    Y = torch.tensor([store.get_vector(f"{i}-I") for i in live],
                     dtype=torch.float64)
    ptr, idx, val = [0], [], []
    for basket in baskets:
        for item, value in basket:
            if item in col:
                idx.append(col[item])
                val.append(value)
        ptr.append(len(idx))
    csr = CSR(torch.tensor(ptr, dtype=torch.int64),
              torch.tensor(idx, dtype=torch.int32),
              torch.tensor(val, dtype=torch.float32), len(baskets), len(live))
    if mode == "implicit":
        return R.implicit_dense_f64(csr, Y, ALPHA, REG)
    out = torch.zeros(len(baskets), Y.shape[1], dtype=torch.float64)
    for u in range(len(baskets)):
        s, e = ptr[u], ptr[u + 1]
        if s == e:
            continue
        y = Y[torch.tensor(idx[s:e])]
        r = torch.tensor(val[s:e], dtype=torch.float64)
        A = y.T @ y + REG * (e - s) * torch.eye(Y.shape[1],
                                                dtype=torch.float64)
        out[u] = torch.linalg.solve(A, y.T @ r)
    return out


def check_fold_in(device, mode):
    store = fx.build_store(device)
    used, X, rows = store.fold_in(BASKETS, REG, **_kw(mode))
    assert used == USED and rows == []
    assert X.shape == (4, 4) and X.dtype == torch.float32
    assert X.device.type == "cpu"
    assert not bool(X[2].any())
    assert bool(X[0].any()) and bool(X[1].any()) and bool(X[3].any())
    # exactly the solve it is built on
    csr, table, used2 = compact_problem(store, BASKETS, device)
    assert used2 == USED
    assert torch.equal(X, direct_solve(store, csr, table, mode).cpu())
    # and the float64 oracles over the live vectors, under the bf16
    # convention with the fp32 torch reference as the yardstick
    x64 = oracle_f64(store, BASKETS, mode)
    cpu = torch.device("cpu")
    cstore = store if device.type == "cpu" else fx.build_store(cpu)
    ccsr, ctable, _ = compact_problem(cstore, BASKETS, cpu)
    x32 = direct_solve(cstore, ccsr, ctable, mode)
    ref_err = float((x32.double() - x64).abs().max())
    tol = 4.0 * ref_err + 4.0 * ULP32 * float(x64.abs().max())
    err = float((X.double() - x64).abs().max())
    print(f"fold_in {mode} on {device}: err {err:.3e} reference {ref_err:.3e} "
          f"tol {tol:.3e}")
    assert err <= tol, (mode, err, tol)
    with pytest.raises(ValueError, match="twice"):
        store.fold_in([[("12", 1.0), ("13", 1.0), ("12", 2.0)]], REG,
                      **_kw(mode))
    with pytest.raises(ValueError, match="reserved"):
        store.fold_in([[("12", 1.0)]], REG, user_ids=["MEAN"], **_kw(mode))
    assert store.get_vector("MEAN-U") == [9.0] * 4


# ------------------------------------------------- recommend + persist

def brute_force(store, q, n, exclude=()):
    """fp64 ranking of query q over the live items: score descending, then
    numeric id.  Returns (items, scores, every candidate's score sorted)."""
    ranked = []
    for item in fx.LIVE:
        if item in exclude:
            continue
        v = store.get_vector(f"{item}-I")
        ranked.append((-sum(a * b for a, b in zip(q, v)), int(item)))
    ranked.sort()
    return ([str(i) for _, i in ranked[:n]], [-s for s, _ in ranked[:n]],
            [-s for s, _ in ranked])


def check_recommend_and_persist(device, mode):
    store = fx.build_store(device)
    n, k = 5, 4
    kw = _kw(mode)
    for exclude_seen in (True, False):
        used, X, items, scores, rows = store.fold_in_recommend(
            BASKETS, n, REG, exclude_seen=exclude_seen, **kw)
        assert used == USED and rows == []
        assert items[2] == [] and scores[2] == []
        for i, basket in enumerate(BASKETS):
            if not used[i]:
                continue
            seen = {item for item, _ in basket}
            q = X[i].to(torch.bfloat16).double().tolist()
            want_i, want_s, every = brute_force(
                store, q, n, seen if exclude_seen else ())
            bound = 4 * k * 2.0 ** -24 * max(
                sum(abs(a * b) for a, b in
                    zip(q, store.get_vector(f"{item}-I")))
                for item in fx.LIVE)
            # the oracle's own numbers: distinct scores are further apart
            # than the bound, so the ranking is decided
            gaps = [a - b for a, b in zip(every, every[1:]) if a != b]
            assert all(g > 2 * bound for g in gaps), (i, min(gaps), bound)
            assert items[i] == want_i, (mode, exclude_seen, i)
            assert len(scores[i]) == len(want_s)
            for got, want in zip(scores[i], want_s):
                assert abs(got - want) <= bound, (got, want, bound)
            if exclude_seen:
                assert not seen & set(items[i])
        if exclude_seen:
            assert items[3] == []                # every live item was seen
        else:
            assert len(items[3]) == n
            assert any(set(items[i]) & {it for it, _ in BASKETS[i]}
                       for i in (0, 1))
    # an explicit exclusion list on top
    _, _, items_x, _, _ = store.fold_in_recommend(
        BASKETS[:2], n, REG, exclude=[[items[0][0]], []],
        exclude_seen=False, **kw)
    assert items[0][0] not in items_x[0] and items_x[1] == items[1]
    # persist: the stored user is served exactly what the fold-in returned
    ids = ["900", "901", "902", "903"]
    used, X, items, scores, rows = store.fold_in_recommend(
        BASKETS, n, REG, user_ids=ids, **kw)
    assert [r.split(",")[0] for r in rows] == ["900", "901", "903"]
    assert all(r.split(",")[1] == "U" for r in rows)
    assert store.get_vector("902-U") is None
    for i in (0, 1, 3):
        seen = [item for item, _ in BASKETS[i]]
        found, r_items, r_scores = store.recommend([ids[i]], n,
                                                   exclude=[seen])
        assert found == [True]
        assert r_items[0] == items[i] and r_scores[0] == scores[i]
        assert [float(x) for x in rows[[0, 1, 3].index(i)]
                .split(",")[2].split(";")] == X[i].tolist()
    assert store.predict("900", "12") is not None
    assert store.predict("902", "12") is None
