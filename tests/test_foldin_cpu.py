"""ALS fold-in on the CPU, through the references: the row-list Gram
reference, the store's cached live-item Gram, ``fold_in`` /
``fold_in_recommend`` (the same checks test_gpu_foldin.py runs on the GPU),
the REST endpoint with its journal, the client, the CLI, and one
trainer-level test showing fold-in is the trainer's user half-iteration.
"""

import io

import pytest
import torch
from fastapi.testclient import TestClient

import _foldin_fixture as ff
import _implicit_fixture as ifx
import _topk_store_fixture as fx
from flink_ms_amd import ops
from flink_ms_amd.models.als import ALSConfig, ALSTrainer
from flink_ms_amd.ops import reference as R
from flink_ms_amd.serving import ALSModelStore, SVMModelStore, create_app
from flink_ms_amd.serving.client import QueryClientHelper

CPU = torch.device("cpu")


# ------------------------------------------------------ row-list reference

@pytest.mark.parametrize("gather", ["fp8", "bf16"])
def test_factor_gram_rows_reference(gather):
    tab = ifx.factor_table(200, 16, seed=9, gather=gather)
    g = torch.Generator().manual_seed(4)
    rows = torch.randperm(200, generator=g)[:45]
    rows[7] = rows[3]                               # a repeated row
    g64 = R.factor_gram_f64(tab[rows])
    assert torch.equal(R.factor_gram_f64(tab, rows), g64)
    assert torch.equal(R.factor_gram_f64(tab, rows.to(torch.int32)), g64)
    G = ops.factor_gram(tab, rows=rows)
    assert torch.equal(G, R.factor_gram_reference(tab[rows]))
    assert torch.equal(G, ops.factor_gram(tab[rows]))
    a = R._table_f32(tab[rows]).double().abs()
    assert bool(((G.double() - g64).abs()
                 <= 2 * 45 * 2.0 ** -24 * (a.T @ a)).all())
    assert not torch.equal(G, ops.factor_gram(tab))
    Z = ops.factor_gram(tab, rows=torch.zeros(0, dtype=torch.int64))
    assert Z.shape == (16, 16) and not bool(Z.any())
    with pytest.raises(ValueError, match="rows entries must be rows"):
        ops.factor_gram(tab, rows=torch.tensor([200]))


# ------------------------------------------------------------------ store

def test_store_item_gram_exact():
    ff.check_store_gram(CPU)


def test_store_item_gram_of_an_empty_store():
    store = ALSModelStore(device=CPU)
    assert store._item_gram().numel() == 0
    used, X, rows = store.fold_in([[("1", 1.0)]], 0.1, implicit=True)
    assert used == [0] and X.shape[0] == 1 and rows == []
    store.ingest_row("1,U,1.0;2.0")                 # users only: zeros
    assert torch.equal(store._item_gram(), torch.zeros(2, 2))
    store.ingest_row("MEAN,I,5.0;5.0")              # not a live item
    assert torch.equal(store._item_gram(), torch.zeros(2, 2))
    store.ingest_row("7,I,1.0;2.0")
    assert store._item_gram().tolist() == [[1.0, 2.0], [2.0, 4.0]]


@pytest.mark.parametrize("mode", ff.MODES)
def test_fold_in_equals_its_solve(mode):
    ff.check_fold_in(CPU, mode)


@pytest.mark.parametrize("mode", ff.MODES)
def test_fold_in_recommend_and_persist(mode):
    ff.check_recommend_and_persist(CPU, mode)


def test_fold_in_bad_arguments():
    store = fx.build_store(CPU)
    with pytest.raises(ValueError):
        store.fold_in([[("12", 1.0)]], 0.1, user_ids=["1", "2"])
    for n in (0, 129):
        with pytest.raises(ValueError):
            store.fold_in_recommend([[("12", 1.0)]], n, 0.1)
    with pytest.raises(ValueError):
        store.fold_in_recommend([[("12", 1.0)]], 3, 0.1, exclude=[[], []])
    wide = ALSModelStore(device=CPU)
    wide.ingest_row("1,I," + ";".join(["1.0"] * 144))
    with pytest.raises(ValueError, match="rank <= 128"):
        wide.fold_in([[("1", 1.0)]], 0.1)


# ---------------------------------------------------- REST, client and CLI

@pytest.fixture()
def http():
    return TestClient(create_app(fx.build_store(CPU), SVMModelStore()))


def _helper(http):
    helper = QueryClientHelper("testserver", 80)
    helper._client.close()
    helper._client = http
    helper.base = "http://testserver"
    return helper


def _body(**kw):
    body = {"items": [[i for i, _ in b] for b in ff.BASKETS],
            "values": [[v for _, v in b] for b in ff.BASKETS],
            "regularization": ff.REG, "implicit": True, "alpha": ff.ALPHA}
    body.update(kw)
    return body


def test_rest_foldin(http):
    store = http.app.state.als
    want_used, want_X, _ = fx.build_store(CPU).fold_in(
        ff.BASKETS, ff.REG, implicit=True, alpha=ff.ALPHA)
    r = http.post("/als/foldin", json=_body())
    assert r.status_code == 200, r.text
    out = r.json()
    assert set(out) == {"used", "factors", "items", "scores", "rows"}
    assert out["used"] == ff.USED and out["rows"] == []
    assert out["items"] == [[]] * 4 and out["scores"] == [[]] * 4
    X = torch.tensor([[float(x) for x in f.split(";")]
                      for f in out["factors"]], dtype=torch.float32)
    assert torch.equal(X, want_X)
    # ids are normalised; values default to 1; n asks for recommendations
    out = http.post("/als/foldin", json={
        "items": [[" 13 "]], "regularization": ff.REG, "n": 3}).json()
    _, _, want_i, want_s, _ = store.fold_in_recommend(
        [[("13", 1.0)]], 3, ff.REG)
    assert out["used"] == [1]
    assert out["items"] == want_i and out["scores"] == want_s
    assert len(want_i[0]) == 3 and "13" not in want_i[0]
    out = http.post("/als/foldin", json={
        "items": [["13"]], "regularization": ff.REG, "n": 3,
        "exclude_seen": False, "exclude": [[want_i[0][0]]]}).json()
    assert want_i[0][0] not in out["items"][0]


def test_rest_foldin_rejects(http):
    bad = [
        _body(values=[[1.0]]),                                # baskets
        _body(values=[[1.0]] + [[v for _, v in b]
                                for b in ff.BASKETS[1:]]),    # entries
        _body(exclude=[[]]), _body(users=["1"]),
        _body(n=-1), _body(n=129), _body(regularization=-0.5),
        _body(items=[["12", " 12"]], values=None),            # duplicate
        _body(items=[["12"]], values=None, users=["mean"]),
        {"items": [["12"]]},                                  # no lambda
        _body(items=[["1"]] * 1025, values=None),
        _body(items=[["1"] * 32769] * 2, values=None),
    ]
    for body in bad:
        r = http.post("/als/foldin", json=body)
        assert r.status_code in (400, 422), (body.get("n"), r.status_code)
        if "regularization" in body:
            assert r.status_code == 400
    assert http.post("/als/foldin", json=_body(
        items=[["1"]] * 1024, values=None)).status_code == 200


def test_rest_foldin_persists(http):
    out = http.post("/als/foldin", json=_body(
        users=["900", "901", "902", "903"], n=5)).json()
    assert [r.split(",")[0] for r in out["rows"]] == ["900", "901", "903"]
    assert out["rows"][0] == "900,U," + out["factors"][0]
    p = http.get("/als/predict", params={"user": "900", "item": "12"}).json()
    assert p["found"] is True
    x = [float(v) for v in out["factors"][0].split(";")]
    assert p["prediction"] == sum(
        a * b for a, b in zip(x, fx.digits(fx.LIVE["12"])))
    assert http.get("/als/predict", params={"user": "902", "item": "12"}
                    ).json()["found"] is False
    seen = [i for i, _ in ff.BASKETS[0]]
    rec = http.post("/als/recommend", json={"users": ["900"], "n": 5,
                                            "exclude": [seen]}).json()
    assert rec["items"][0] == out["items"][0]
    assert rec["scores"][0] == out["scores"][0]


def test_rest_foldin_fs_backend_keeps_the_user(tmp_path):
    uri = str(tmp_path / "ckpt")

    def app():
        return create_app(ALSModelStore(device=CPU), SVMModelStore(),
                          checkpoint_data_uri=uri, checkpoint_interval_ms=0,
                          state_backend="fs")

    with TestClient(app()) as c:
        c.post("/model/als/rows", json={"rows": [
            "1,I,1.0;2.0", "2,I,0.5;0.5", "3,I,2.0;0.0"]})
        assert c.post("/checkpoint").json()["written"] > 0
        out = c.post("/als/foldin", json={
            "items": [["1", "3"]], "values": [[4.0, 2.0]],
            "regularization": 0.1, "users": ["77"]}).json()
        assert out["used"] == [2] and len(out["rows"]) == 1
        # simulate crash: NO further checkpoint
    with TestClient(app()) as c:
        hit = c.get("/state/ALS_MODEL/77-U")
        assert hit.status_code == 200
        assert hit.json()["value"][1] == out["factors"][0]
        assert c.get("/als/predict", params={"user": "77", "item": "2"}
                     ).json()["found"] is True


def test_client_fold_in(http):
    res = _helper(http).als_fold_in([["13"], ["777"]], [[4.0], [1.0]],
                                    regularization=ff.REG, n=2)
    used, X, items, scores, _ = http.app.state.als.fold_in_recommend(
        [[("13", 4.0)], [("777", 1.0)]], 2, ff.REG)
    assert res["used"] == used == [1, 0]
    assert res["items"] == items and res["scores"] == scores
    assert res["items"][1] == [] and len(res["items"][0]) == 2
    assert [float(x) for x in res["factors"][0].split(";")] == X[0].tolist()
    # values default to 1.0, keywords pass through
    res = _helper(http).als_fold_in([["13"]], regularization=ff.REG,
                                    implicit=True, alpha=ff.ALPHA)
    _, X, _ = http.app.state.als.fold_in([[("13", 1.0)]], ff.REG,
                                         implicit=True, alpha=ff.ALPHA)
    assert [float(x) for x in res["factors"][0].split(";")] == X[0].tolist()


def test_cli_foldin(http, monkeypatch, capsys):
    from flink_ms_amd.cli import als_foldin
    monkeypatch.setattr(als_foldin, "QueryClientHelper",
                        lambda host, port: _helper(http))
    monkeypatch.setattr(http, "close", lambda: None)
    monkeypatch.setattr("sys.stdin",
                        io.StringIO("12:1,31:4, 20 ,11:16,999\n\n777\n"))
    assert als_foldin.main(["job0", "testserver", "80", "--lambda",
                            str(ff.REG), "--implicitPrefs", "true",
                            "--alpha", str(ff.ALPHA), "--n", "3"]) == 0
    out = capsys.readouterr().out
    _, _, items, scores, _ = http.app.state.als.fold_in_recommend(
        ff.BASKETS[:1], 3, ff.REG, implicit=True, alpha=ff.ALPHA)
    assert len(items[0]) == 3
    for item, score in zip(items[0], scores[0]):
        assert f"{item}\t{score:f}\n" in out
    assert out.count("\t") == 3
    assert "do not exist in the model for the query: 777" in out
    assert als_foldin.main([]) == 1
    assert als_foldin.main(["job0"]) == 1                   # no --lambda
    assert als_foldin.main(["job0", "--lambda"]) == 1
    assert als_foldin.main(["job0", "--lambda", "1", "--bogus", "1"]) == 1


# ------------------------------------------------------------- trainer

def test_fold_in_is_the_trainers_user_half_iteration():
    nu, ni, rank, alpha, reg = 30, 40, 8, 10.0, 0.1
    u, i, r = ifx.planted_implicit(nu, ni, 6, 4, seed=21)
    cfg = ALSConfig(iterations=2, num_factors=rank, lambda_=reg,
                    implicit_prefs=True, alpha=alpha, dtype=torch.float32)
    tr = ALSTrainer(cfg)
    tr.ctx.device = CPU
    tr.setup(u.long(), i.long(), r, nu, ni)
    for _ in range(2):
        tr.step()
    m = tr.model()
    store = ALSModelStore(device=CPU)
    store.attach_factors(m.user_factors, m.item_factors,
                         user_ids=m.user_ids, item_ids=m.item_ids)
    csr = ifx.user_item_csr(u, i, r, nu, ni)
    ptr = csr.indptr.tolist()
    baskets = [[(str(int(csr.indices[j])), float(csr.values[j]))
                for j in range(ptr[row], ptr[row + 1])]
               for row in range(nu)]
    used, X, _ = store.fold_in(baskets, reg, implicit=True, alpha=alpha)
    assert used == csr.row_counts().tolist() and min(used) > 0
    # the trainer's user solve against the bf16 item table the store serves
    order = torch.argsort(m.item_ids)
    Y = m.item_factors[order].to(torch.bfloat16)
    s, e = ops.implicit_weights(csr.values, alpha)
    x64 = R.als_solve_weighted_f64(csr, Y, reg, s, e, R.factor_gram_f64(Y))
    x32 = R.als_solve_weighted_reference(csr, Y, reg, s, e,
                                         R.factor_gram_reference(Y))
    ref_err = float((x32.double() - x64).abs().max())
    tol = 4.0 * ref_err + 4.0 * ff.ULP32 * float(x64.abs().max())
    err = float((X.double() - x64).abs().max())
    print(f"fold-in vs trainer half-iteration: err {err:.3e} "
          f"reference {ref_err:.3e} tol {tol:.3e}")
    assert err <= tol
