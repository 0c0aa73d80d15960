"""Bit parity of the host code that composes the ALS kernels into a
half-iteration and a training step: ``ops.als_solve_side`` (fused and slab
paths), ``ops.als_solve_chunk`` and the exchange modes of ``ALSTrainer``
(docs/KERNELS.md "Dispatch and trainer parity").

Every fused kernel solves one entity from that entity's own row, in stored
order, so chunking, launch order, slab size and the replica layout change
where a row lives and when it is solved, never an operand.  The assertions
are therefore ``torch.equal`` on bit patterns; the one tolerance is in
``test_replay_is_anchored``, which ties the common answer to float64.

dispatch path                         gather   ratings   rank        test
------------------------------------  -------  --------  ----------  ----
trainer off / force x {1,3,7,200}     both     both      10, 64, 80  modes_equal_replay
als_solve_chunk, partial id lists     both     both      16, 64      solve_chunk_scatter (wave)
                                      both     both      80, 128     solve_chunk_scatter (block)
  ... rank 10 padded to 16            both     both      10          modes_equal_replay (force)
als_solve_side slab path + images     both     both      16, 64      slab_sizes (gramian[_w] + ldl_solve_wave_reg)
als_solve_side slab_rows at k > 64    both     both      80          slab_sizes (block-fused kernel: the
                                                                     wrapper ignores slab_rows above 64)
"""

import functools

import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.data.blocked import CSR
from flink_ms_amd.ops import reference as R

import _implicit_fixture as fx
import _trainer_fixture as tf

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -23
GATHERS = ["bf16", "fp8"]
RATINGS = [pytest.param(False, id="explicit"), pytest.param(True, id="implicit")]


@functools.lru_cache(maxsize=None)
def _triples():
    return tf.small_ratings(seed=11)


# ------------------------------------------------- 1. trainer vs the replay

@pytest.mark.parametrize("implicit", RATINGS)
@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", [10, 64, 80])
def test_trainer_modes_equal_replay(gpu, k, gather, implicit):
    """Padded wave (10 -> 16), full wave (64) and block-fused (80) ranks.
    Step 1 consumes the replica filled at setup, steps 2-3 what the comm
    stream gathered during the previous solve."""
    triples = _triples()
    kp = (k + 15) // 16 * 16
    want = None
    for mode, chunks in tf.MODES:
        cfg = tf.Cfg(gather, implicit, k, mode, chunks)
        tr, image0, recs = tf.run_trainer(gpu, cfg, triples)
        assert tr._overlap == (mode == "force")
        what = f"k={k} {gather} implicit={implicit} {mode}/{chunks}"
        if want is None:
            first_image = image0
            want = tf.replay(gpu, cfg, triples, image0)
        assert torch.equal(image0.view(torch.uint8),
                           first_image.view(torch.uint8)), what
        for rec in recs:
            assert rec.user_f32.shape == (tf.NUM_USERS, kp)
            assert rec.item_f32.shape == (tf.NUM_ITEMS, kp)
        tf.assert_records_equal(recs, want, what)
        for step, rec in enumerate(recs, 1):
            tf.assert_record_shape(rec, cfg, triples, f"{what}, step {step}")


# ------------------------------------------------------ 2. als_solve_chunk

CHUNK_REG = 0.25
CHUNK_ALPHA = 100.0      # _implicit_fixture: |scale * f| <= 30, |ext| <= 21
# the staging edges of _implicit_fixture four times over, and one more row
CHUNK_LENGTHS = fx.ROW_LENGTHS * 4 + (5,)
TABLE_ROWS = 50


@functools.lru_cache(maxsize=None)
def _chunk_case(k, gather, weighted):
    """CPU-side problem, built once and never modified."""
    csr = fx.csr_with_row_lengths(CHUNK_LENGTHS, TABLE_ROWS, seed=400 + k)
    assert csr.num_rows == 45 and int(csr.indices.max()) < TABLE_ROWS
    tab = fx.factor_table(TABLE_ROWS, k, seed=500 + k, gather=gather)
    kw = {}
    if weighted:
        s, e = ops.implicit_weights(csr.values, CHUNK_ALPHA)
        rows, _ = R.effective_rows(csr, tab, s, e)
        assert float(rows.abs().max()) <= 64 and float(e.abs().max()) <= 64
        kw = dict(scale=s, ext=e, base=fx.random_base(k, seed=k))
    return csr, tab, kw


def _on(gpu, csr, tab, kw):
    return csr.to(gpu), tab.to(gpu), {n: t.to(gpu) for n, t in kw.items()}


def _prefilled(nrows, k, gather, gpu):
    """fp32 buffer of NaN and an image of 0xA5 bytes."""
    x = torch.full((nrows, k), float("nan"), device=gpu)
    width = k if gather == "fp8" else 2 * k
    img = torch.full((nrows, width), 0xA5, dtype=torch.uint8, device=gpu)
    return x, (img if gather == "fp8" else img.view(torch.bfloat16))


def _flat(csr, tab, kw, gather, gpu, **more):
    """One flat als_solve_side call with the gather dtype's image."""
    _, img = _prefilled(csr.num_rows, tab.shape[1], gather, gpu)
    x = ops.als_solve_side(csr, tab, CHUNK_REG,
                           out_bf16=img if gather == "bf16" else None,
                           out_fp8=img if gather == "fp8" else None,
                           **more, **kw)
    torch.cuda.synchronize()
    return x, img


def _id_lists(nrows):
    """A contiguous range in permuted order, one row, a strided subset of
    the rest, and the remainder (a size that is no multiple of 4)."""
    g = torch.Generator().manual_seed(nrows)
    contiguous = 8 + torch.randperm(12, generator=g)
    single = torch.tensor([nrows - 1])
    taken = set(contiguous.tolist()) | set(single.tolist())
    rest = torch.tensor([r for r in range(nrows) if r not in taken])
    strided = rest[::3][torch.randperm(len(rest[::3]), generator=g)]
    taken |= set(strided.tolist())
    remainder = torch.tensor([r for r in range(nrows) if r not in taken])
    assert remainder.numel() % 4 != 0 and strided.numel() % 4 != 0
    lists = [contiguous, single, strided, remainder]
    assert sorted(torch.cat(lists).tolist()) == list(range(nrows))
    return lists


@pytest.mark.parametrize("weighted", [False, True], ids=["explicit", "weighted"])
@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", [16, 64, 80, 128])
def test_solve_chunk_scatter(gpu, k, gather, weighted):
    csr, tab, kw = _on(gpu, *_chunk_case(k, gather, weighted))
    n = csr.num_rows
    x_flat, img_flat = _flat(csr, tab, kw, gather, gpu)
    x, img = _prefilled(n, k, gather, gpu)
    x0, img0 = x.clone(), img.clone()

    def chunk(ids):
        ops.als_solve_chunk(csr, tab, CHUNK_REG, x,
                            img if gather == "fp8" else None,
                            img if gather == "bf16" else None,
                            ids.to(torch.int32).to(gpu), **kw)
        torch.cuda.synchronize()

    def check(done, what):
        solved = torch.zeros(n, dtype=torch.bool)
        solved[torch.tensor(done, dtype=torch.int64)] = True
        solved = solved.to(gpu)
        tf.assert_same_bits(x[~solved], x0[~solved], f"{what}: stray x")
        tf.assert_same_bits(img[~solved], img0[~solved], f"{what}: stray image")
        tf.assert_same_bits(x[solved], x_flat[solved], f"{what}: x")
        tf.assert_same_bits(img[solved], img_flat[solved], f"{what}: image")

    chunk(torch.empty(0, dtype=torch.int64))
    check([], "empty id list")
    done = []
    for ids in _id_lists(n):
        chunk(ids)
        done += ids.tolist()
        check(done, f"after {len(done)} of {n} rows")
    assert len(done) == n


def test_solve_chunk_empty_ids_never_reach_the_extension(gpu, monkeypatch):
    """An empty id list returns before the launcher could see nrows = 0."""
    csr, tab, kw = _on(gpu, *_chunk_case(16, "fp8", False))
    monkeypatch.setattr(ops, "_require_hip", lambda: pytest.fail("launched"))
    x, img = _prefilled(csr.num_rows, 16, "fp8", gpu)
    ops.als_solve_chunk(csr, tab, CHUNK_REG, x, img, None,
                        torch.empty(0, dtype=torch.int32, device=gpu))


# ------------------------------------------------------------ 3. slab path

@pytest.mark.parametrize("weighted", [False, True], ids=["explicit", "weighted"])
@pytest.mark.parametrize("gather", GATHERS)
@pytest.mark.parametrize("k", [16, 64, 80])
def test_slab_sizes_do_not_change_bits(gpu, k, gather, weighted):
    """k <= 64: gramian[_w] over a sliced indptr + ldl_solve_wave_reg with
    sliced images; one slab keeps the launch schedule, several drop it.
    k = 80: als_solve_side takes the block-fused kernel whatever slab_rows
    says, so there the slab sizes must trivially agree."""
    cpu_csr, _, _ = _chunk_case(k, gather, weighted)
    csr, tab, kw = _on(gpu, *_chunk_case(k, gather, weighted))
    n = csr.num_rows
    order = torch.randperm(n, generator=torch.Generator().manual_seed(k)
                           ).to(torch.int32).to(gpu)
    first = None
    for slab in (1, 4, 33, n, n + 5):
        for ro in (None, order):
            x, img = _flat(csr, tab, kw, gather, gpu, slab_rows=slab,
                           row_order=ro)
            what = f"slab_rows={slab}" + (" row_order" if ro is not None else "")
            if first is None:
                first = (x, img)
                empty = (cpu_csr.row_counts() == 0).to(gpu)
                assert int(empty.sum()) == 4
                assert bool((tf.bits(x)[empty] == 0).all())
                assert bool((tf.bits(img)[empty] == 0).all())
                tf.assert_same_bits(img, tf._image(x, gather), "image of x")
            tf.assert_same_bits(x, first[0], f"{what}: x")
            tf.assert_same_bits(img, first[1], f"{what}: image")


# ------------------------------------------------- 4. the float64 anchor

def _criterion(x, x64, x32, factor):
    err = float((x - x64).abs().max())
    cpu = float((x32.double() - x64).abs().max())
    tol = factor * cpu + 4.0 * ULP32 * float(x64.abs().max())
    return err, cpu, tol


def _explicit_kernel_ratio(gpu, csr, tab, s, e, gather):
    """The explicit kernel on the expanded table of the base = 0 problem
    (one table row per stored entry, already scaled and rounded; ratings =
    ext) against the same criterion: the yardstick of the e4m3 factor.
    Only computed where the fixed e4m3 factor is missed (``_hold``); the
    figures in docs/KERNELS.md were measured once with it."""
    zero = torch.zeros(tab.shape[1], tab.shape[1])
    rows, _ = R.effective_rows(csr, tab, s, e)
    z64 = R.als_solve_weighted_f64(csr, tab, tf.REG, s, e, zero)
    z32 = R.als_solve_weighted_reference(csr, tab, tf.REG, s, e, zero)
    xtab = tf._image(rows, gather)
    nnz = csr.indices.numel()
    xcsr = CSR(csr.indptr, torch.arange(nnz, dtype=torch.int32), e.clone(),
               csr.num_rows, nnz)
    xe = ops.als_solve_side(xcsr.to(gpu), xtab.to(gpu), tf.REG)
    err, cpu, _ = _criterion(xe.cpu().double(), z64, z32, 1.0)
    return err / max(cpu, 1e-300)


def _hold(what, gpu, gather, x, x64, x32, csr, tab, s, e):
    """The criterion with F = 4 (bf16) or 2 * FP8_EXPLICIT_RATIO (e4m3, wave
    kernel at k = 64).  Where the e4m3 factor is missed, the constant is not
    widened: the explicit kernel's own ratio on the same inputs is printed
    and x is held to twice that."""
    factor = 2.0 * fx.FP8_EXPLICIT_RATIO["wave"] if gather == "fp8" else 4.0
    err, cpu, tol = _criterion(x, x64, x32, factor)
    print(f"{what}: err {err:.3e} cpu-fp32 {cpu:.3e} ratio "
          f"{err / max(cpu, 1e-300):.2f} tol {tol:.3e}")
    if err > tol and gather == "fp8":
        own = _explicit_kernel_ratio(gpu, csr, tab, s, e, gather)
        _, _, tol = _criterion(x, x64, x32, 2.0 * own)
        print(f"{what}: above {factor:.1f}x; the explicit kernel's own "
              f"ratio on these inputs is {own:.1f}, tol {tol:.3e}")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("implicit", RATINGS)
@pytest.mark.parametrize("gather", GATHERS)
def test_replay_is_anchored(gpu, gather, implicit):
    """"Same bits" must not mean "same wrong answer": the two half-
    iterations of the last step, inputs read back from the trainer's own
    images, against a float64 solve of those inputs with the criterion of
    test_gpu_implicit.py: max|x - x64| <= F max|x32 - x64| + 4 ulp max|x64|
    (``_hold``).  Explicit: the contract's oracle with scale = 1, ext = r,
    base = 0.  Implicit: the dense Hu-Koren-Volinsky update, which shares
    nothing with the scale / ext / base path -- but it does not round
    scale * f to the gather dtype either, so x32 (which does) is itself
    2e-3 (bf16) to 4e-2 (e4m3) away from it and this assertion alone would
    pass many wrong kernels: it only rules out a grossly wrong update.  The
    one that bites is the second, the contract's own oracle on exactly the
    scale, ext and base the kernel was given; it is not independent of
    implicit_weights and factor_gram, which test_gpu_implicit.py holds to
    their own oracles."""
    k = 64
    triples = _triples()
    cfg = tf.Cfg(gather, implicit, k, "force", 3)
    tr, _, recs = tf.run_trainer(gpu, cfg, triples)
    ucsr, icsr = tf.side_csrs(triples, "cpu")
    last, prev = recs[-1], recs[-2]
    for side, csr, image, x, w in (
            ("user", ucsr, prev.item_image, last.user_f32, tr.user_w),
            ("item", icsr, last.user_image, last.item_f32, tr.item_w)):
        tab = image.cpu()
        x = x.cpu().double()
        what = f"{side} {gather} implicit={implicit}"
        if implicit:
            s, e = ops.implicit_weights(csr.values, tf.ALPHA)
            base = R.factor_gram_reference(tab)
            x64 = R.implicit_dense_f64(csr, R._table_f32(tab), tf.ALPHA,
                                       tf.REG)
        else:
            s, e = torch.ones_like(csr.values), csr.values
            base = torch.zeros(k, k)
            x64 = R.als_solve_weighted_f64(csr, tab, tf.REG, s, e, base)
        x32 = R.als_solve_weighted_reference(csr, tab, tf.REG, s, e, base)
        _hold(what, gpu, gather, x, x64, x32, csr, tab, s, e)
        if implicit:
            s, e = (t.cpu() for t in w)
            base = ops.factor_gram(image).cpu()
            c64 = R.als_solve_weighted_f64(csr, tab, tf.REG, s, e, base)
            c32 = R.als_solve_weighted_reference(csr, tab, tf.REG, s, e, base)
            _hold(what + ", contract oracle", gpu, gather, x, c64, c32, csr,
                  tab, s, e)
