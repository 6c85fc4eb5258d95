"""tests/seam_restatement.py without a GPU: hand-worked seams, and the algebra of ShardedTiler._ids_of (the torch form that
obia_tiler_import_seam replaced) on CPU tensors with a stub engine -- the restatement tests/test_gpu_seam_import.py holds the kernels to."""
import numpy as np
import pytest

from tests import seam_restatement as SR

I32 = np.int32


def test_a_hand_worked_seam():
    me, owner, third = 1, 2, 5
    fmap = np.zeros(10, I32)
    fmap[3] = 41                                                  # id 3 of the owner is local id 41 already
    code_of = np.full(60, 7, I32)
    codes = np.array([[0, -5, SR.code(me, 9), SR.code(owner, 3), SR.code(owner, 8)],
                      [SR.code(owner, 2), SR.code(owner, 8), SR.code(third, 2), SR.code(owner, 12), SR.code(owner, 0)]], I32)
    r = SR.import_seam(codes, me, owner, fmap, code_of, 50)
    # new ids of the owner: 2 and 8 (8 twice), ascending -> 50 and 51; 12 lies beyond the map, 0 is no id
    assert r["ids"].tolist() == [[0, 0, 9, 41, 51], [50, 51, 0, 0, 0]] and r["ids"].dtype == I32
    assert (r["first"], r["n_new"], r["t_max"]) == (50, 2, 12)
    want_f = np.zeros(10, I32)
    want_f[[2, 3, 8]] = [50, 41, 51]
    assert np.array_equal(r["fmap"], want_f)
    want_c = np.full(60, 7, I32)
    want_c[50], want_c[51] = (3 << 24) | 2, (3 << 24) | 8
    assert np.array_equal(r["code_of"], want_c)
    assert not fmap[2] and code_of[50] == 7                       # the inputs are left alone
    # the same seam again: nothing is new, the same ids
    again = SR.import_seam(codes, me, owner, r["fmap"], r["code_of"], 52)
    assert again["n_new"] == 0 and again["t_max"] == 12 and np.array_equal(again["ids"], r["ids"])
    assert np.array_equal(again["fmap"], r["fmap"]) and np.array_equal(again["code_of"], r["code_of"])
    # on a larger map id 12 is imported too
    grown = np.zeros(16, I32)
    grown[:10] = r["fmap"]
    more = SR.import_seam(codes, me, owner, grown, r["code_of"], 52)
    assert more["n_new"] == 1 and more["ids"].tolist() == [[0, 0, 9, 41, 51], [50, 51, 0, 52, 0]] and more["fmap"][12] == 52
    assert more["code_of"][52] == (3 << 24) | 12


def test_the_edges_of_the_code():
    me, owner = 0, 126
    fmap, code_of = np.zeros(1 << 12, I32), np.zeros(40, I32)
    top = SR.ID_MASK                                              # the largest id a code carries; the largest rank keeps the code positive
    codes = np.array([SR.code(owner, top), SR.code(owner, 1), SR.code(me, top), SR.code(owner, len(fmap) - 1), SR.code(owner, len(fmap)),
                      np.iinfo(I32).min, -1, SR.code(me, 0)], I32)
    assert (codes[:5] > 0).all()
    r = SR.import_seam(codes, me, owner, fmap, code_of, 30)
    assert r["ids"].tolist() == [0, 30, top, 31, 0, 0, 0, 0] and r["t_max"] == top and r["n_new"] == 2
    # an empty seam, and a seam without a code of the owner
    e = SR.import_seam(np.zeros((0,), I32), me, owner, fmap, code_of, 30)
    assert e["ids"].shape == (0,) and (e["n_new"], e["t_max"]) == (0, 0)
    o = SR.import_seam(SR.code(np.array([me, 5, 5]), np.array([4, 4, 9])), me, owner, fmap, code_of, 30)
    assert o["ids"].tolist() == [4, 0, 0] and (o["n_new"], o["t_max"]) == (0, 0) and not o["fmap"].any()
    # when I am the owner myself, my own rank decides
    s = SR.import_seam(SR.code(np.array([3, 3]), np.array([6, 7])), 3, 3, fmap, code_of, 30)
    assert s["ids"].tolist() == [6, 7] and s["n_new"] == 0 and s["t_max"] == 0


class StubEngine:
    """what the torch form asks of an engine: the id counter"""

    def __init__(self, next_id):
        self.n = int(next_id)

    def next_id(self):
        return self.n

    def set_segments(self, first, sizes):
        self.n = max(self.n, int(first) + int(sizes.numel()))


def test_the_torch_form_of_the_sharded_driver_is_this_algebra():
    torch = pytest.importorskip("torch")
    from obia_amd.distributed import ShardedTiler
    me, owner = 1, 2
    t = object.__new__(ShardedTiler)
    t.rank, t.engine, t.G = me, StubEngine(57), torch.zeros((1, 1), dtype=torch.int32)
    t.code_of = torch.zeros((1 << 16,), dtype=torch.int32)
    t.fmap, t.f_batches, t.stats = {}, [], {"imports": 0, "foreign_ids": 0}
    rs = np.random.RandomState(3)
    fmap, code_of, nxt = np.zeros(1 << 12, I32), np.zeros(1 << 16, I32), 57      # (the torch form starts its map at 4096 entries here)
    for step, hi in enumerate([300, 300, 3000, 9000, 9000]):      # 9000 lies beyond the first map: one growth
        tt = rs.randint(0, hi, size=(7, 150))
        oo = rs.choice([owner, owner, owner, me, 4], size=(7, 150))
        codes = np.where(rs.rand(7, 150) < 0.2, rs.randint(-3, 1, (7, 150)), SR.code(oo, tt)).astype(I32)
        want = t._ids_of(torch.as_tensor(codes), (owner,)).numpy()
        while True:                                               # as ShardedTiler._ids_of_kernel: again on a grown map
            r = SR.import_seam(codes, me, owner, fmap, code_of, nxt)
            fmap, code_of, nxt = r["fmap"], r["code_of"], nxt + r["n_new"]
            if r["t_max"] < len(fmap):
                break
            grown = np.zeros(1 << (2 * r["t_max"] + 2).bit_length(), I32)
            grown[:len(fmap)] = fmap
            fmap = grown
        assert np.array_equal(r["ids"].astype(np.int64), want), step
        assert nxt == t.engine.next_id()
        fm = t.fmap[owner].numpy()
        m = min(len(fm), len(fmap))
        assert np.array_equal(fm[:m], fmap[:m]) and not fm[m:].any() and not fmap[m:].any()
        assert np.array_equal(t.code_of.numpy()[:nxt], code_of[:nxt])
    assert len(fmap) > 1 << 12 and nxt > 57 + 1000               # the map grew; well over a thousand ids came in
