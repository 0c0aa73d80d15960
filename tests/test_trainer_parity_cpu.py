"""The trainer parity harness on the CPU path: the fixture's own properties,
and every exchange mode of ``ALSTrainer`` bit-equal to the replay chain of
flat ``ops.als_solve_side`` calls (``tests/_trainer_fixture.py``).  The GPU
twin is ``test_gpu_trainer_parity.py``."""

import functools

import pytest
import torch

from flink_ms_amd import ops
from flink_ms_amd.parallel.shard import ChunkedAllgather, Partition

import _trainer_fixture as tf

CPU = torch.device("cpu")


@functools.lru_cache(maxsize=None)
def _triples(empty_rows=True):
    return tf.small_ratings(seed=11, empty_rows=empty_rows)


def test_fixture_properties():
    for empty_rows in (True, False):
        u, i, r = _triples(empty_rows)
        tf.check_small_ratings(u, i, r, empty_rows)
        assert u.numel() == (2698 if empty_rows else 2703)
        u2, i2, r2 = tf.small_ratings(seed=11, empty_rows=empty_rows)
        assert torch.equal(u, u2) and torch.equal(i, i2) \
            and torch.equal(r, r2)
    ucsr, icsr = tf.side_csrs(_triples(), CPU)
    assert int(icsr.row_counts().max()) >= tf.HEAVY_ITEM_MIN
    assert sorted(tf.EDGE_USERS.values()) == sorted(
        int(ucsr.row_counts()[u]) for u in tf.EDGE_USERS)
    # implicit weights stay far from e4m3 saturation (448)
    s, e = ops.implicit_weights(ucsr.values, tf.ALPHA)
    assert float(s.max()) < 8 and float(e.max()) < 8


def test_fixture_catches_a_wrong_bit():
    x = torch.zeros(3, 4)
    y = x.clone()
    y[2, 1] = -0.0
    assert torch.equal(x, y)
    with pytest.raises(AssertionError, match="row 2 column 1"):
        tf.assert_same_bits(y, x, "signed zero")
    img = torch.ones(3, 4, dtype=torch.bfloat16)
    bad = img.clone()
    bad[1, 3] = 1.0078125
    with pytest.raises(AssertionError, match="row 1 column 3"):
        tf.assert_same_bits(bad, img, "one bf16 ulp")


def _ctx(world=1):
    from flink_ms_amd.parallel.dist import DistContext
    return DistContext(rank=0, world_size=world, local_rank=0, device=CPU)


@pytest.mark.parametrize("world", [1, 3])
def test_chunk_slabs_tile_the_shard(world):
    """Every (shard size, chunk count): the slabs tile the shard without an
    empty or negative one, and the remap is a bijection onto the replica.
    Rounding the slab size up used to leave slabs that START past the end
    (5 rows in 4 chunks, 71 in 50): negative row counts, a replica smaller
    than the side and remapped ids outside it."""
    ctx = _ctx(world)
    for ss in range(1, 80):
        total = ss * world
        for chunks in list(range(1, 60)) + [200]:
            ch = ChunkedAllgather(ctx, Partition(total, world), chunks)
            what = (ss, world, chunks)
            assert 1 <= ch.chunks <= min(chunks, ss), what
            assert ch.chunks == len(ch.bounds) == len(ch.rows), what
            assert all(r >= 1 for r in ch.rows), what
            covered = [r for a, b in ch.bounds for r in range(a, b)]
            assert covered == list(range(ss)), what
            assert ch.replica_rows == total, what
            pos = ch.remap_indices(torch.arange(total)).long()
            assert sorted(pos.tolist()) == list(range(total)), what
            if world == 1:
                assert torch.equal(pos, torch.arange(total)), what
    for chunks, want in ((1, 1), (3, 3), (7, 7), (50, 36), (200, 71)):
        ch = ChunkedAllgather(_ctx(), Partition(tf.NUM_ITEMS, 1), chunks)
        assert ch.chunks == want


def test_overlap_setup_failure_restores_global_ids(monkeypatch):
    """The fall-back to the serial exchange must undo the column remap of
    the replica layout: the serial all-gather is in global id order."""
    from flink_ms_amd.models.als import ALSTrainer
    triples = _triples()
    cfg = tf.Cfg("bf16", False, 8, "force", 3)
    _, _, want = tf.run_trainer(CPU, cfg._replace(mode="off"), triples)

    def boom(self, dev, kp):
        raise RuntimeError("no replica today")
    monkeypatch.setattr(ALSTrainer, "_prep_overlap", boom)
    monkeypatch.setattr(ChunkedAllgather, "remap_indices",
                        lambda self, ids: torch.zeros_like(ids))
    tr, _, got = tf.run_trainer(CPU, cfg, triples)
    assert tr._overlap is False
    tf.assert_records_equal(got, want, "fallback")


@pytest.mark.parametrize("empty_rows", [True, False],
                         ids=["empty-rows", "no-empty-rows"])
@pytest.mark.parametrize("implicit", [False, True],
                         ids=["explicit", "implicit"])
@pytest.mark.parametrize("gather", ["bf16", "fp8"])
@pytest.mark.parametrize("k", [8, 10])
def test_trainer_modes_equal_replay_cpu(k, gather, implicit, empty_rows):
    triples = _triples(empty_rows)
    want = None
    for mode, chunks in tf.MODES_CPU:
        cfg = tf.Cfg(gather, implicit, k, mode, chunks)
        tr, image0, recs = tf.run_trainer(CPU, cfg, triples)
        assert tr._overlap == (mode == "force")
        what = f"k={k} {gather} implicit={implicit} {mode}/{chunks}"
        if want is None:
            first_image = image0
            want = tf.replay(CPU, cfg, triples, image0)
        assert torch.equal(image0.view(torch.uint8),
                           first_image.view(torch.uint8))
        tf.assert_records_equal(recs, want, what)
        for step, rec in enumerate(recs, 1):
            tf.assert_record_shape(rec, cfg, triples, f"{what}, step {step}")
