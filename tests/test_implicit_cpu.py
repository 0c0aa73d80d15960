"""Implicit-feedback (confidence-weighted) ALS on the CPU: the weighted
normal-equation contract, its float64 oracles, the trainer and the CLI.

The formulation under test: per stored entry ``scale = sqrt(alpha*|r|)`` and
``ext = (1 + alpha*|r|)/scale`` for ``r > 0`` (else 0), base matrix
``G0 = Y^T Y`` over all rows of the opposite side; then
``A = G0 + sum (s q)(s q)^T + reg*n*I``, ``b = sum ext * (s q)`` is the
Hu-Koren-Volinsky update with this project's weighted lambda.
"""

import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.models.als import ALSConfig, ALSTrainer
from flink_ms_amd.ops import reference

from _implicit_fixture import planted_implicit, user_item_csr

ALPHA, REG = 40.0, 0.1


def _toy(seed=3, users=60, items=40, density=0.25):
    """60 x 40 at ~25 % density, values in {-2..3} (zero and negative stored
    values included), user 7 left without any entry."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(users, items, generator=g) < density
    mask[7] = False
    u, i = mask.nonzero(as_tuple=True)
    r = torch.randint(-2, 4, (u.numel(),), generator=g).float()
    assert (r == 0).any() and (r < 0).any()
    return u, i, r, users, items


def test_implicit_weights_formula():
    r = torch.tensor([2.0, -3.0, 0.0, 0.5, 10.0])
    s, e = ops.implicit_weights(r, 40.0)
    w = 40.0 * r.abs()
    assert s.dtype == torch.float32 and e.dtype == torch.float32
    assert torch.equal(s, torch.sqrt(w))
    assert e[1] == 0 and e[2] == 0 and s[2] == 0       # r < 0, r = 0
    pos = r > 0
    assert torch.equal(e[pos], (1 + w[pos]) / torch.sqrt(w[pos]))


def test_weighted_oracle_equals_dense_closed_form():
    u, i, r, nu, ni = _toy()
    csr = user_item_csr(u, i, r, nu, ni)
    assert int(csr.row_counts()[7]) == 0
    Y = torch.randn(ni, 8, generator=torch.Generator().manual_seed(1))
    s, e = ops.implicit_weights(csr.values, ALPHA)
    x = reference.als_solve_weighted_f64(
        csr, Y, REG, s, e, reference.factor_gram_f64(Y), gather=None)
    dense = reference.implicit_dense_f64(csr, Y, ALPHA, REG)
    # both float64; the gap is s and e being formed in fp32 (~1e-7)
    gap = float((x - dense).abs().max() / dense.abs().max())
    print(f"weighted oracle vs dense closed form: {gap:.3e} of max|x|")
    assert gap <= 1e-6
    assert torch.equal(x[7], torch.zeros(8, dtype=torch.float64))

    # the fp32 reference (the GPU tests' yardstick): distance only reported
    x32 = reference.als_solve_weighted_reference(
        csr, Y, REG, s, e, reference.factor_gram_reference(Y), gather=None)
    print("fp32 reference vs oracle: "
          f"{float((x32.double() - x).abs().max() / x.abs().max()):.3e}")
    assert torch.equal(x32[7], torch.zeros(8))


@pytest.mark.parametrize("gather", ["fp8", "bf16"])
def test_weighted_reference_rounds_like_the_contract(gather):
    """round_D sits after ONE fp32 multiply; pair_D is the hi/lo pair."""
    u, i, r, nu, ni = _toy(seed=5)
    csr = user_item_csr(u, i, r, nu, ni)
    g = torch.Generator().manual_seed(2)
    f = torch.rand(ni, 16, generator=g) - 0.5
    tab = ops.quantize_fp8(f) if gather == "fp8" else f.to(torch.bfloat16)
    s, e = ops.implicit_weights(csr.values, ALPHA)
    rows, pair = reference.effective_rows(csr, tab, s, e)
    deq = ops.dequantize_fp8(tab) if gather == "fp8" else tab.float()
    want = s.unsqueeze(1) * deq[csr.indices.long()]
    if gather == "fp8":
        want = ops.dequantize_fp8(ops.quantize_fp8(want))
        assert torch.equal(pair, ops.fp8_rating_pair(e))
    else:
        want = want.to(torch.bfloat16).float()
        assert torch.equal(pair, ops.bf16_rating_pair(e))
        # bf16 hi/lo keeps 16 mantissa bits
        assert float(((pair - e).abs() / e.abs().clamp_min(1e-30)).max()) \
            < 2.0 ** -15
    assert torch.equal(rows, want)
    # the solve through ops (CPU path) is the reference on those rows
    base = ops.factor_gram(tab)
    assert torch.equal(base, deq.T @ deq)
    x = ops.als_solve_side(csr, tab, REG, scale=s, ext=e, base=base)
    x64 = reference.als_solve_weighted_f64(csr, tab, REG, s, e, base)
    assert torch.isfinite(x).all()
    assert float((x.double() - x64).abs().max()) <= 1e-3 * float(
        x64.abs().max())


def test_ops_weight_triple_all_or_none():
    u, i, r, nu, ni = _toy()
    csr = user_item_csr(u, i, r, nu, ni)
    Y = torch.randn(ni, 8)
    s, e = ops.implicit_weights(csr.values, ALPHA)
    base = ops.factor_gram(Y)
    for kw in ({"scale": s}, {"ext": e}, {"base": base},
               {"scale": s, "ext": e}, {"scale": s, "base": base},
               {"ext": e, "base": base}):
        with pytest.raises(ValueError, match="all three"):
            ops.als_solve_side(csr, Y, REG, **kw)
        with pytest.raises(ValueError, match="all three"):
            ops.gramian(csr, Y, REG, **kw)
        with pytest.raises(ValueError, match="all three"):
            ops.als_solve_chunk(csr, Y, REG, torch.zeros(nu, 8), None, None,
                                torch.arange(4), **kw)
    with pytest.raises(ValueError, match="one element per stored entry"):
        ops.als_solve_side(csr, Y, REG, scale=s[:-1], ext=e, base=base)
    with pytest.raises(ValueError, match="base must be"):
        ops.als_solve_side(csr, Y, REG, scale=s, ext=e, base=base[:4])


def _objective_trace(cfg, u, i, r, nu, ni, iters):
    """implicit_objective after every half-step of the single-process
    trainer: (X_t, Y_{t-1}) after the user half, (X_t, Y_t) after the item
    half."""
    csr = user_item_csr(u, i, r, nu, ni)
    tr = ALSTrainer(cfg)
    tr.ctx.device = torch.device("cpu")
    tr.setup(u.long(), i.long(), r, nu, ni)
    k = cfg.num_factors

    def items_now():
        sh = tr.item_shard[:ni, :k]
        return (ops.dequantize_fp8(sh) if sh.dtype == torch.uint8
                else sh.float())

    y_prev = items_now().clone()
    trace = []
    for _ in range(iters):
        tr.step()
        m = tr.model()
        x, y = m.user_factors.float(), m.item_factors.float()
        trace.append(reference.implicit_objective(csr, x, y_prev, cfg.alpha,
                                                  cfg.lambda_))
        trace.append(reference.implicit_objective(csr, x, y, cfg.alpha,
                                                  cfg.lambda_))
        y_prev = y.clone()
    return trace, tr


def test_fp32_trainer_objective_falls_monotonically():
    u, i, r, nu, ni = _toy(seed=11)
    cfg = ALSConfig(iterations=6, num_factors=8, lambda_=REG,
                    dtype=torch.float32, implicit_prefs=True, alpha=ALPHA)
    trace, _ = _objective_trace(cfg, u, i, r, nu, ni, 6)
    print("objective per half-step:", [f"{v:.6g}" for v in trace])
    # each half-step minimises its side exactly; an fp32 solve error enters
    # the objective to second order only
    for prev, cur in zip(trace, trace[1:]):
        assert cur <= prev * (1 + 1e-6), trace
    assert trace[-1] < 0.9 * trace[0]


@pytest.mark.parametrize("kw", [{"factor_dtype": "fp8"},
                                {"dtype": torch.bfloat16}])
def test_factor_dtype_emulation_runs_and_stays_finite(kw):
    u, i, r = planted_implicit(90, 40, 8, 4, seed=2)
    base = dict(iterations=3, num_factors=8, lambda_=REG,
                dtype=torch.float32, implicit_prefs=True, alpha=10.0)
    base.update(kw)
    trace, tr = _objective_trace(ALSConfig(**base), u, i, r, 90, 40, 3)
    m = tr.model()
    assert torch.isfinite(m.user_factors).all()
    assert torch.isfinite(m.item_factors).all()
    assert all(v == v and v < float("inf") for v in trace)
    assert trace[-1] < trace[0]


def test_implicit_differs_from_explicit_and_default_is_off():
    assert ALSConfig().implicit_prefs is False and ALSConfig().alpha == 1.0
    u, i, r, nu, ni = _toy(seed=4)
    out = []
    for implicit in (False, True):
        tr = ALSTrainer(ALSConfig(iterations=2, num_factors=8, lambda_=REG,
                                  dtype=torch.float32,
                                  implicit_prefs=implicit, alpha=ALPHA))
        tr.ctx.device = torch.device("cpu")
        tr.setup(u.long(), i.long(), r, nu, ni)
        out.append(tr.fit().user_factors.clone())
    assert not torch.allclose(out[0], out[1])


def test_cli_implicit_prefs(tmp_path):
    from flink_ms_amd.cli import als_train
    from flink_ms_amd.utils.textio import parse_als_row
    u, i, r = planted_implicit(40, 24, 6, 4, seed=9)
    csv = tmp_path / "clicks.csv"
    with open(csv, "w") as f:
        f.write("userId,itemId,strength\n")
        for a, b, c in zip(u.tolist(), i.tolist(), r.tolist()):
            f.write(f"{a},{b},{c}\n")
    texts = {}
    for name, extra in (("explicit", []),
                        ("implicit", ["--implicitPrefs", "true",
                                      "--alpha", "10"])):
        uf, itf = tmp_path / f"{name}.U", tmp_path / f"{name}.I"
        assert als_train.main(["--input", str(csv), "--iterations", "3",
                               "--numFactors", "8", "--lambda", "0.1",
                               "--userFactors", str(uf),
                               "--itemFactors", str(itf), *extra]) == 0
        texts[name] = (open(uf).read(), open(itf).read())
    assert texts["implicit"][0] != texts["explicit"][0]
    assert texts["implicit"][1] != texts["explicit"][1]
    for text, kind in zip(texts["implicit"], "UI"):
        rows = [parse_als_row(line) for line in text.splitlines()]
        assert rows and all(k == kind and len(f) == 8 for _, k, f in rows)
        assert all(x == x for _, _, f in rows for x in f)
