"""Every index class against the row-list model of index_lifecycle.py over deterministic pseudo-random operation sequences
and the hand-written ones: what an index holds and returns is a function of its training and of the rows that are live, in arrival order, and
of nothing else that happened to it.  Every checkpoint compares ntotal, the contents, reconstruct_n, search, range search and (flat, fp16-SQ)
the bounds with the yardsticks, bit for bit.  test_index_lifecycle_host.py asserts the generator's conditions for every sequence run here.
Sixteen families (the five flat / code classes with both 8-bit quantisers, the four inverted-file classes with IVFPQ coded with and without
residuals, two RefineFlatIndex pairings, PreTransformIndex, GraphFlatIndex, ImpactIndex), three seeds each, and the named sequences."""
import pytest
import torch

import index_lifecycle as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", L.SEEDS)
@pytest.mark.parametrize("family", L.FAMILIES)
def test_generated_sequence(family, seed, tmp_path):
    ops = L.sequence(family, seed)
    assert all(L.conditions(family, ops).values())
    L.Driver(L.make_model(family, seed), tmp_path).run(ops)


@pytest.mark.parametrize("name,family", [(n, f) for n, (fams, _, _) in L.NAMED.items() for f in fams])
def test_named_sequence(name, family, tmp_path):
    _, ops, ntotals = L.NAMED[name]
    drv = L.Driver(L.make_model(family), tmp_path)
    if name == "ivfpq_129_check_add1_check":
        drv.run(ops[:2])            # the first checkpoint's rebuild replaced the codes by a buffer of exactly ceil(129 / 128) = 2 blocks
        pq = drv.idx.pq
        assert pq._codes.numel() == 2 * 128 * pq.Mp and pq.capacity == 256
        drv.run(ops[2:])            # the next row is coded into that buffer, or one grown from it: either way after the 129 rows it holds
        assert pq.ntotal == 130 and pq.capacity >= 256
    else:
        drv.run(ops)
    assert drv.idx.ntotal == ntotals[-1]


@pytest.mark.parametrize("family", ["pq", "sq8", "sq8_uniform"])
def test_first_commit_trains_and_reset_keeps_the_training(family, tmp_path):
    """An untrained code index is trained by its first commit(); reset() drops the rows and keeps that training: the rows added afterwards are
    coded under it.  The model takes the training from the index (a k-means for PQ: not restated here) and the rest from the yardsticks."""
    m = L.Model(family)
    drv = L.Driver(m, tmp_path, trained=False)
    idx = drv.idx
    assert not idx.is_trained
    rows = m.draw(300)
    idx.append_slot(300).copy_(torch.from_numpy(rows))
    idx.commit(300)
    assert idx.is_trained and idx.ntotal == 300
    if family == "pq":
        m.C = idx.centroids.cpu().numpy().copy()
    else:
        m.trained = idx.trained.cpu().numpy().copy()
        import sq8_yardstick as S8
        L.same(m.trained, S8.train(rows, m.uniform), "the range the first commit() trained")
    m.append(rows)
    L.same(idx.codes(), m.codes(), "codes() after the first commit()")
    drv.apply(("reset",))
    assert idx.is_trained and idx.ntotal == 0
    drv.apply(("add", 130))
    L.same(idx.centroids if family == "pq" else idx.trained, m.C if family == "pq" else m.trained, "the training after reset() and add()")
    L.same(idx.codes(), m.codes(), "codes() after reset() and add()")
    if family == "pq":                      # (the trained 8-bit range is off the grid on which its score bits are order-independent)
        drv.check()
