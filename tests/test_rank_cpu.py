"""CPU tests of rank counts and the ranking metrics: the float64 oracle
against a literal double loop, the fp32 reference and the wrapper's
validation, consistency with the top-N reference, hand-checked metrics, the
``als_rank_eval`` CLI and ``POST /als/rank``.
"""

import importlib.util
import json
import math
import os

import pytest
import torch
from fastapi.testclient import TestClient

from flink_ms_amd import ops
from flink_ms_amd.models.ranking import RankingResult, evaluate_ranking
from flink_ms_amd.ops import reference
from flink_ms_amd.serving import SVMModelStore, create_app
from flink_ms_amd.serving.client import QueryClientHelper

import _topk_store_fixture as fx

CPU = torch.device("cpu")


def _ints(shape, seed, lo=-3, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.bfloat16)


def _csr(lists):
    ptr = torch.zeros(len(lists) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.tensor([len(x) for x in lists]), 0)
    flat = [r for rows in lists for r in sorted(rows)]
    return ptr, torch.tensor(flat, dtype=torch.int64)


def _loop(Q, V, q_idx, t_idx, cand, lists):
    """The contract, literally."""
    def key(x):            # NaN below -inf; -0 == +0 is float comparison
        return (0, 0.0) if math.isnan(x) else (1, x)
    rows = range(V.shape[0]) if cand is None else cand.tolist()
    out = []
    for q, t in zip(q_idx.tolist(), t_idx.tolist()):
        ts = float(sum(a * b for a, b in zip(Q[q].tolist(), V[t].tolist())))
        g = e = 0
        for r in rows:
            if r == t or r in lists[q]:
                continue
            s = float(sum(a * b for a, b in zip(Q[q].tolist(),
                                                V[r].tolist())))
            g += key(s) > key(ts)
            e += key(s) == key(ts)
        out.append((g, e, ts))
    return out


# ------------------------------------------------------------------ oracle

def test_oracle_equals_the_double_loop():
    Q = torch.tensor([[1, 0, 2], [0, 1, 1], [2, 2, 0], [1, 1, 1],
                      [0, 0, 0]], dtype=torch.float64)
    V = torch.tensor([[1, 1, 1], [2, 0, 1], [0, 2, 1], [1, 1, 1], [3, 0, 0],
                      [0, 0, 3], [1, 2, 0], [2, 1, 0], [1, 1, 1]],
                     dtype=torch.float64)
    lists = [[0, 4], [], [3, 6, 7], [8], [1]]
    q_idx = torch.tensor([0, 0, 1, 2, 2, 3, 4, 3, 1])
    t_idx = torch.tensor([3, 4, 2, 6, 0, 0, 5, 8, 7])   # 4, 6, 8: excluded
    for cand in (None, torch.tensor([8, 0, 2, 3, 5, 6])):
        g, e, s = reference.rank_counts_f64(Q, V, q_idx, t_idx, cand,
                                            _csr(lists))
        want = _loop(Q, V, q_idx, t_idx, cand, lists)
        assert g.tolist() == [w[0] for w in want]
        assert e.tolist() == [w[1] for w in want]
        assert s.tolist() == [w[2] for w in want]
        assert s.dtype == torch.float64
    assert int(e.sum()) > 0 and int(g.sum()) > 0        # ties and losses


def test_oracle_nan_order():
    Q = torch.ones(1, 2, dtype=torch.float64)
    V = torch.tensor([[1.0, 1.0], [float("nan"), 0.0], [float("nan"), 1.0],
                      [-float("inf"), 0.0], [0.0, -0.0]], dtype=torch.float64)
    q_idx, t_idx = torch.zeros(5, dtype=torch.int64), torch.arange(5)
    g, e, _ = reference.rank_counts_f64(Q, V, q_idx, t_idx)
    assert g.tolist() == [0, 3, 3, 2, 1] and e.tolist() == [0, 1, 1, 0, 0]
    want = _loop(Q, V, q_idx, t_idx, None, [[]])
    assert [(w[0], w[1]) for w in want] == list(zip(g.tolist(), e.tolist()))


# ------------------------------------------------- reference and validation

@pytest.fixture(scope="module")
def problem():
    nq, nv, k, P = 9, 120, 24, 60
    Q, V = _ints((nq, k), 1), _ints((nv, k), 2)
    g = torch.Generator().manual_seed(3)
    q_idx = torch.randint(0, nq, (P,), generator=g)
    t_idx = torch.randint(0, nv, (P,), generator=g)
    lists = [torch.randperm(nv, generator=g)[:7 * q].tolist()
             for q in range(nq)]
    cand = torch.randperm(nv, generator=g)[:100]
    return Q, V, q_idx, t_idx, cand, lists


def test_reference_equals_oracle_and_cpu_dispatch(problem):
    Q, V, q_idx, t_idx, cand, lists = problem
    for c in (None, cand):
        for ex in (None, _csr(lists)):
            want = reference.rank_counts_f64(Q, V, q_idx, t_idx, c, ex)
            ref = reference.rank_counts_reference(Q, V, q_idx, t_idx, c, ex)
            got = ops.rank_counts(Q, V, q_idx, t_idx, cand=c, exclude=ex)
            for out in (ref, got):
                assert torch.equal(out[0], want[0])
                assert torch.equal(out[1], want[1])
                assert out[2].dtype == torch.float32
                assert torch.equal(out[2].double(), want[2])
            vec = ops.rank_counts_vectors(Q, V, V[t_idx], q_idx, t_idx,
                                          cand=c, exclude=ex)
            assert torch.equal(vec[0], want[0])
            assert torch.equal(vec[1], want[1])


def test_no_pairs_on_cpu(problem):
    Q, V = problem[0], problem[1]
    none = torch.zeros(0, dtype=torch.int64)
    g, e, s = ops.rank_counts(Q, V, none, none)
    assert g.numel() == e.numel() == s.numel() == 0


def test_wrapper_validation(problem):
    Q, V, q_idx, t_idx, cand, lists = problem
    nq, nv = Q.shape[0], V.shape[0]
    ptr, ex = _csr(lists)

    def bad(**kw):
        args = dict(q_idx=q_idx, t_idx=t_idx, cand=None, exclude=None)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.rank_counts(Q, V, args["q_idx"], args["t_idx"],
                            cand=args["cand"], exclude=args["exclude"])

    for wrong in (-1, nq):
        q = q_idx.clone()
        q[5] = wrong
        bad(q_idx=q)
    for wrong in (-1, nv):
        t = t_idx.clone()
        t[5] = wrong
        bad(t_idx=t)
    bad(t_idx=t_idx[:-1])
    bad(cand=torch.tensor([3, 4, 3]))                   # repeated
    bad(cand=torch.tensor([3, nv]))
    bad(exclude=(ptr[:-1], ex))                         # wrong length
    bad(exclude=(torch.cat([ptr, ptr[-1:]]), ex))
    down = ex.clone()
    down[[0, 1]] = down[[1, 0]]                         # slice 1 descends
    assert int(ptr[1]) == 0 and int(ptr[2]) == 7
    bad(exclude=(ptr, down))
    twice = ex.clone()
    twice[1] = twice[0]                                 # ... or repeats
    bad(exclude=(ptr, twice))
    out = ex.clone()
    out[-1] = nv
    bad(exclude=(ptr, out))
    # a step down where the next slice starts is fine
    ops.rank_counts(Q, V, q_idx, t_idx,
                    exclude=_csr([[5, 9], [], [1, 2]] + [[]] * (nq - 3)))


# ------------------------------------------------- consistency with top-N

def test_position_in_the_top_n_list(problem):
    Q, V, _, _, cand, lists = problem
    nq, nv = Q.shape[0], V.shape[0]
    cand = cand[:100]
    ex = _csr(lists)
    scores, rows = reference.topk_scores_reference(Q, V, 128, cand, ex)
    q_idx = torch.arange(nq).repeat_interleave(cand.numel())
    t_idx = cand.repeat(nq)
    g, e, s = ops.rank_counts(Q, V, q_idx, t_idx, cand=cand, exclude=ex)
    seen = 0
    for p in range(q_idx.numel()):
        q, t = int(q_idx[p]), int(t_idx[p])
        if t in lists[q]:
            assert t not in rows[q].tolist()
            continue
        pos = rows[q].tolist().index(t)          # every live row is listed
        assert int(g[p]) <= pos <= int(g[p]) + int(e[p])
        live = rows[q] >= 0
        assert int(g[p]) == int((scores[q][live] > scores[q, pos]).sum())
        assert float(scores[q, pos]) == float(s[p])
        seen += 1
    assert seen > 500


# ----------------------------------------------------------------- metrics

def _one_user():
    """k = 1, user factor 1: an item's score is its factor.  Items 5 and 6
    are training items (they would top the list)."""
    U = torch.tensor([[1.0]])
    V = torch.tensor([[5.0], [3.0], [3.0], [3.0], [1.0], [10.0], [10.0]])
    train = (torch.tensor([0, 0, 0]), torch.tensor([5, 6, 5]))   # one repeat
    return U, V, train


def test_metrics_by_hand_one_held_out_item():
    U, V, (tu, ti) = _one_user()
    r = evaluate_ranking(U, V, tu, ti, torch.tensor([0]), torch.tensor([1]),
                         ns=(2, 10))
    assert isinstance(r, RankingResult)
    # g = 1 (item 0), e = 2 (items 2, 3), c = 7 - 2 - 1 = 4
    assert r.mean_percentile_rank == pytest.approx(100 * (1 + 1) / 4, abs=1e-12)
    assert r.auc == pytest.approx(1 - 2 / 4, abs=1e-12)
    assert r.hit_rate[2] == pytest.approx(1 / 3, abs=1e-12)
    assert r.hit_rate[10] == 1.0
    assert r.mrr == pytest.approx((1 / 2 + 1 / 3 + 1 / 4) / 3, abs=1e-12)
    dcg = (1 / math.log2(3) + 1 / math.log2(4) + 1 / math.log2(5)) / 3
    assert r.ndcg[10] == pytest.approx(dcg / 1.0, abs=1e-12)
    # positions 1, 2, 3 with cut-off 2: only position 1 is inside
    assert r.ndcg[2] == pytest.approx(1 / math.log2(3) / 3, abs=1e-12)
    assert (r.n_scored, r.n_skipped, r.n_degenerate) == (1, 0, 0)


def test_metrics_by_hand_two_held_out_items():
    U, V, (tu, ti) = _one_user()
    r = evaluate_ranking(U, V, tu, ti, torch.tensor([0, 0]),
                         torch.tensor([1, 4]), ns=(10, 1))
    # item 4: g = 4, e = 0 (the other held-out item competes), c = 4
    first = (1 / math.log2(3) + 1 / math.log2(4) + 1 / math.log2(5)) / 3
    dcg = first + 1 / math.log2(6)
    idcg = 1 / math.log2(2) + 1 / math.log2(3)
    assert r.ndcg[10] == pytest.approx(dcg / idcg, abs=1e-12)
    assert r.ndcg[1] == 0.0
    assert r.mean_percentile_rank == pytest.approx(
        100 * ((1 + 1) / 4 + 4 / 4) / 2, abs=1e-12)
    assert r.mrr == pytest.approx(((1 / 2 + 1 / 3 + 1 / 4) / 3 + 1 / 5) / 2,
                                  abs=1e-12)
    assert r.hit_rate[1] == 0.0 and r.hit_rate[10] == 1.0


def test_skipped_and_degenerate_pairs():
    U = torch.tensor([[1.0], [2.0]])
    V = torch.tensor([[5.0], [3.0], [1.0]])
    # user 1 has trained on every item
    tu, ti = torch.tensor([1, 1, 1, 0]), torch.tensor([0, 1, 2, 0])
    hu, hi = torch.tensor([0, 7, 0, 1]), torch.tensor([1, 1, 99, 2])
    r = evaluate_ranking(U, V, tu, ti, hu, hi)
    assert (r.n_scored, r.n_skipped, r.n_degenerate) == (2, 2, 1)
    # only (0, 1) has a percentile: item 2 below it, item 0 excluded
    assert r.mean_percentile_rank == 0.0 and r.auc == 1.0
    # id maps: user id 7 -> row 0, item id 99 -> row 1
    uidx = torch.full((8,), -1, dtype=torch.int64)
    uidx[7] = 0
    iidx = torch.full((100,), -1, dtype=torch.int64)
    iidx[99], iidx[3] = 1, 2
    r = evaluate_ranking(U, V, torch.tensor([7]), torch.tensor([50]),
                         torch.tensor([7, 7, 6, 500]),
                         torch.tensor([99, 3, 99, 99]), user_index=uidx,
                         item_index=iidx)
    assert (r.n_scored, r.n_skipped, r.n_degenerate) == (2, 2, 0)
    none = evaluate_ranking(U, V, tu, ti, torch.tensor([9]),
                            torch.tensor([0]))
    assert none.n_scored == 0 and math.isnan(none.mean_percentile_rank)


def test_agrees_with_the_benchmark_number():
    path = os.path.join(os.path.dirname(__file__), "..", "benchmarks",
                        "implicit_quality.py")
    spec = importlib.util.spec_from_file_location("implicit_quality", path)
    iq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(iq)
    nu, ni, blocks = 60, 40, 4
    u, i, _ = iq.planted(nu, ni, 8, blocks, 5)
    last = torch.zeros(nu, dtype=torch.int64)
    last[u] = torch.arange(u.numel())
    held = torch.zeros(u.numel(), dtype=torch.bool)
    held[last] = True
    held &= (i % blocks) == (u % blocks)
    tu, ti, hu, hi = u[~held], i[~held], u[held], i[held]
    assert hu.numel() > 30
    seen = torch.zeros(nu, ni, dtype=torch.bool)
    seen[tu, ti] = True
    # wide integers: every dot is exact in fp32 (|sum| <= 8e6 < 2^24), and
    # no two items of a user tie
    g = torch.Generator().manual_seed(6)
    U = torch.randint(-1000, 1001, (nu, 8), generator=g).float()
    V = torch.randint(-1000, 1001, (ni, 8), generator=g).float()
    S = U.double() @ V.double().T
    assert all(S[q].unique().numel() == ni for q in range(nu))
    want = iq.mean_percentile_rank(U, V, hu, hi, seen)
    got = evaluate_ranking(U, V, tu, ti, hu, hi)
    assert got.n_scored == hu.numel() and got.n_degenerate == 0
    assert abs(got.mean_percentile_rank - want) <= 1e-12


# ---------------------------------------------------------------------- CLI

def test_cli_round_trip(tmp_path, capsys):
    from flink_ms_amd.cli import als_rank_eval, als_train
    from flink_ms_amd.data.ratings import RatingsShape, synthetic_ratings
    u, i, r = synthetic_ratings(RatingsShape(40, 30, 600), seed=5)
    rows = sorted(set(zip(u.tolist(), i.tolist())))
    test, train = rows[::10], [p for n, p in enumerate(rows) if n % 10]
    for name, part in (("train.csv", train),
                       ("test.csv", test + [(999, 0), (0, 999)])):
        with open(tmp_path / name, "w") as f:
            f.write("userId,movieId,rating\n")
            for a, b in part:
                f.write(f"{a},{b},1.0\n")
    ufile, ifile = tmp_path / "uf.model", tmp_path / "if.model"
    assert als_train.main([
        "--input", str(tmp_path / "train.csv"), "--iterations", "2",
        "--numFactors", "8", "--lambda", "0.1", "--implicitPrefs",
        "--userFactors", str(ufile), "--itemFactors", str(ifile)]) == 0
    capsys.readouterr()
    out_file = tmp_path / "rank.json"
    assert als_rank_eval.main([
        "--userFactors", str(ufile), "--itemFactors", str(ifile),
        "--train", str(tmp_path / "train.csv"),
        "--input", str(tmp_path / "test.csv"), "--n", "5,20",
        "--fieldDelimiter", ",", "--output", str(out_file)]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    res = json.loads(line)
    assert json.loads(open(out_file).read()) == res
    assert res["skipped"] >= 2
    assert res["scored"] + res["skipped"] == len(test) + 2
    assert res["degenerate"] == 0
    assert 0.0 <= res["mean_percentile_rank"] <= 100.0
    assert res["auc"] == pytest.approx(
        1 - res["mean_percentile_rank"] / 100, abs=1e-12)
    assert set(res["hit_rate"]) == set(res["ndcg"]) == {"5", "20"}
    assert 0.0 <= res["hit_rate"]["5"] <= res["hit_rate"]["20"] <= 1.0
    assert 0.0 < res["mrr"] <= 1.0
    # the same numbers as the library call on the parsed files
    uids, U = als_rank_eval._load_factors(str(ufile), "U")
    iids, V = als_rank_eval._load_factors(str(ifile), "I")
    if res["device"] == "cpu":
        tr, te = torch.tensor(train), torch.tensor(test)
        direct = evaluate_ranking(
            U, V, tr[:, 0], tr[:, 1], te[:, 0], te[:, 1], ns=(5, 20),
            user_index=als_rank_eval._index(uids, tr[:, 0], te[:, 0]),
            item_index=als_rank_eval._index(iids, tr[:, 1], te[:, 1]))
        assert direct.mean_percentile_rank == res["mean_percentile_rank"]
        assert direct.n_scored == res["scored"]


# --------------------------------------------------------------------- REST

@pytest.fixture(scope="module")
def store():
    return fx.build_store(CPU)


@pytest.fixture(scope="module")
def http(store):
    return TestClient(create_app(store, SVMModelStore()))


def _oracle(store, user, item, exclude=()):
    """Counts over the concatenated catalogue, from get_vector in float64."""
    items = sorted(fx.LIVE, key=int)
    V = torch.tensor([store.get_vector(f"{i}-I") for i in items],
                     dtype=torch.float64)
    Q = torch.tensor([store.get_vector(f"{user}-U")], dtype=torch.float64)
    gone = sorted(items.index(x) for x in exclude if x in items)
    g, e, s = reference.rank_counts_f64(
        Q, V, torch.tensor([0]), torch.tensor([items.index(item)]),
        exclude=_csr([gone]))
    c = len(items) - len(gone) - (item not in exclude)
    return int(g), int(e), c, float(s)


def test_store_rank_counts_both_sources(store):
    assert set(fx.BULK) | set(fx.ATTACH) | set(fx.ROWS)   # both sources live
    users = ["1", "2", "3", "4", "5", "1", "2"]
    items = ["12", "31", "20", "11", "30", "26", "13"]    # blocks and mirror
    exclude = [["20", "13"], [], ["777", "20"], ["30", "31", "12"], [],
               ["26"], ["10", "33"]]
    for ex in (None, exclude):
        found, g, e, c, s = store.rank(users, items, ex)
        assert found == [True] * len(users)
        for j, (u, i) in enumerate(zip(users, items)):
            assert (g[j], e[j], c[j], s[j]) == _oracle(
                store, u, i, ex[j] if ex else ()), (u, i)
    # items 12 (blocks) and 31 (mirror) share a vector: one tie, across
    # the two sources
    assert store.rank(["1"], ["12"])[2] == [1]
    assert store.rank(["999", "1"], ["12", "888"]) == (
        [False, False], [0, 0], [0, 0], [0, 0], [0.0, 0.0])
    with pytest.raises(ValueError):
        store.rank(["1", "2"], ["12"])
    with pytest.raises(ValueError):
        store.rank(["1", "2"], ["12", "13"], [[]])


def test_rest_rank(store, http):
    body = {"users": [" 1 ", "999", "3"], "items": ["12", "12", " 20"],
            "exclude": [["13"], [], ["21", "nope"]]}
    r = http.post("/als/rank", json=body)
    assert r.status_code == 200
    a = _oracle(store, "1", "12", ["13"])
    b = _oracle(store, "3", "20", ["21"])
    assert r.json() == {"found": [True, False, True],
                        "greater": [a[0], 0, b[0]], "equal": [a[1], 0, b[1]],
                        "candidates": [a[2], 0, b[2]],
                        "score": [a[3], 0.0, b[3]]}
    helper = QueryClientHelper("testserver", 80)
    helper._client.close()
    helper._client = http
    helper.base = "http://testserver"
    assert helper.als_rank(["3"], ["20"], [["21"]])["greater"] == [b[0]]
    for bad in ({"users": ["1"], "items": []},
                {"users": ["1"], "items": ["12"], "exclude": [[], []]}):
        assert http.post("/als/rank", json=bad).status_code == 400
