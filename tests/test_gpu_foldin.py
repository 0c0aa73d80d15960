"""GPU tests of ALS fold-in: the row-list Gram kernel (``k_factor_gram``
with ``ROWS``), the store's cached live-item Gram, ``fold_in`` and
``fold_in_recommend``.

1. Row-list Gram: bit-equal to ``factor_gram`` of the compacted table (the
   same MFMA sequence), every unlisted row poisoned with NaN so a load
   outside the list shows, exactly symmetric, bit-reproducible, and inside
   the fp32 dot bound of test_gpu_implicit.py's ``test_factor_gram``
   against the float64 oracle.
2. The store's ``G0`` is exact on the integer-factor store, before and
   after every writer of an item row.
3. ``fold_in`` is bit-equal to ``ops.als_solve_side`` on the compact problem
   and agrees with the float64 oracles under the bf16 convention.
4. ``fold_in_recommend`` ranks as the brute-force fp64 ranking does, and a
   persisted user is then served the same lists by ``recommend``.
"""

import pytest
import torch

import _foldin_fixture as ff
import _implicit_fixture as fx
from flink_ms_amd import ops
from flink_ms_amd.ops import reference as R

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
NTAB = 200
NAN_BYTE = 0x7F                                   # the e4m3 NaN


def _poisoned(k, gather, rows, seed):
    """(table with every row outside ``rows`` NaN, the clean table)."""
    tab = fx.factor_table(NTAB, k, seed=seed, gather=gather)
    keep = torch.zeros(NTAB, dtype=torch.bool)
    keep[rows] = True
    bad = tab.clone()
    if gather == "fp8":
        bad[~keep] = NAN_BYTE
    else:
        bad[~keep] = float("nan")
    assert bool(torch.isnan(R._table_f32(bad)[~keep]).all())
    return bad, tab


def _row_list(length, seed):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randperm(NTAB, generator=g)[:length]
    if length > 2:                 # neither ascending nor a prefix
        assert bool((rows[1:] < rows[:-1]).any())
        assert sorted(rows.tolist()) != list(range(length))
    return rows


@pytest.mark.parametrize("gather", ["fp8", "bf16"])
@pytest.mark.parametrize("k", [16, 64, 128])
@pytest.mark.parametrize("length", [1, 31, 32, 33, 97])
def test_factor_gram_rows(gpu, length, k, gather):
    rows = _row_list(length, seed=7 * length + k)
    bad, tab = _poisoned(k, gather, rows, seed=400 + length + k)
    g64 = R.factor_gram_f64(tab[rows])
    assert torch.equal(g64, R.factor_gram_f64(tab, rows))
    a = R._table_f32(tab[rows]).double().abs()
    absum = a.T @ a
    dbad, dcompact = bad.to(gpu), tab[rows].to(gpu)
    for rows_dev in (rows.to(gpu), rows.to(torch.int32)):
        for rpp in (None, 32, 96):
            per = rpp or ops.factor_gram_rows_per_part(length, k)
            parts = -(-length // per)
            G = ops.factor_gram(dbad, rows=rows_dev, rows_per_part=rpp)
            assert G.shape == (k, k) and G.dtype == torch.float32
            assert not bool(torch.isnan(G).any())
            assert torch.equal(G, ops.factor_gram(dcompact,
                                                  rows_per_part=rpp))
            assert torch.equal(G, G.T)
            assert torch.equal(
                ops.factor_gram(dbad, rows=rows_dev, rows_per_part=rpp), G)
            err = (G.cpu().double() - g64).abs()
            bound = 2 * (length + parts) * U32 * absum
            assert bool((err <= bound).all()), (length, k, gather, rpp,
                                                float((err / bound).max()))


@pytest.mark.parametrize("gather", ["fp8", "bf16"])
def test_factor_gram_rows_repeats(gpu, gather):
    rows = torch.tensor([5, 5, 7, 199, 5, 0] * 7)       # 42 entries, 2 chunks
    bad, tab = _poisoned(64, gather, rows, seed=11)
    G = ops.factor_gram(bad.to(gpu), rows=rows.to(gpu))
    assert torch.equal(G, ops.factor_gram(tab[rows].to(gpu)))
    g64 = R.factor_gram_f64(tab, rows)
    a = R._table_f32(tab[rows]).double().abs()
    assert bool(((G.cpu().double() - g64).abs()
                 <= 2 * (42 + 2) * U32 * (a.T @ a)).all())
    # a repeated row counts once per occurrence
    once = ops.factor_gram(bad.to(gpu), rows=torch.tensor([5]).to(gpu))
    thrice = ops.factor_gram(bad.to(gpu), rows=torch.tensor([5, 5, 5]).to(gpu))
    assert bool(((thrice - 3 * once).abs() <= 8 * U32 * thrice.abs()).all())


def test_factor_gram_rows_pads_odd_ranks(gpu):
    rows = _row_list(45, seed=3)
    bad, tab = _poisoned(10, "bf16", rows, seed=5)
    G = ops.factor_gram(bad.to(gpu), rows=rows.to(gpu))
    assert G.shape == (10, 10) and not bool(torch.isnan(G).any())
    assert torch.equal(G, ops.factor_gram(tab[rows].to(gpu)))
    assert torch.equal(G, G.T)
    a = tab[rows].double().abs()
    assert bool(((G.cpu().double() - R.factor_gram_f64(tab, rows)).abs()
                 <= 2 * (45 + 2) * U32 * (a.T @ a)).all())


def test_factor_gram_rows_edges(gpu):
    tab = fx.factor_table(NTAB, 16, seed=1, gather="bf16").to(gpu)
    Z = ops.factor_gram(tab, rows=torch.zeros(0, dtype=torch.int64))
    assert Z.shape == (16, 16) and Z.device == tab.device
    assert not bool(Z.any())
    with pytest.raises(ValueError, match="rows entries must be rows"):
        ops.factor_gram(tab, rows=torch.tensor([0, NTAB]))
    with pytest.raises(ValueError, match="rows entries must be rows"):
        ops.factor_gram(tab, rows=torch.tensor([-1]).to(gpu))
    # rows=None is the whole-table path: the full list in order matches it
    every = torch.arange(NTAB)
    assert torch.equal(ops.factor_gram(tab, rows=every, rows_per_part=64),
                       ops.factor_gram(tab, rows_per_part=64))


def test_store_item_gram_exact(gpu):
    ff.check_store_gram(gpu)


@pytest.mark.parametrize("mode", ff.MODES)
def test_fold_in_equals_its_solve(gpu, mode):
    ff.check_fold_in(gpu, mode)


@pytest.mark.parametrize("mode", ff.MODES)
def test_fold_in_recommend_and_persist(gpu, mode):
    ff.check_recommend_and_persist(gpu, mode)
