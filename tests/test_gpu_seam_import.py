"""obia_tiler_import_seam (tiling.hip) on a session of its own, against tests/seam_restatement.py: exact.

tests/test_gpu_distributed.py holds the import to the torch form over seams of 9 x 200 codes, which never reach the counting kernel
(more new ids than the LDS sort takes), the full width of the sort, the second trip of the stride loops, or a refusal.  Here the
entry point is called through ctypes on the handle of a HipTilerEngine over a 64 x 64 x 1 raster (no tile pass runs: the session is
there for its id counter and alive flags).  `ids_out` lies between poisoned guards; `fmap` and `code_of` are the caller's, pre-filled
with content the contract leaves alone, and compared whole; `next_id` and the alive flags are compared after every import."""
import ctypes

import numpy as np
import pytest

from tests import launch_grids as LG
from tests import seam_restatement as SR
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.test_gpu_launch_clamps import crossed, dev, judge

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = POISONS[0]
I32, U8 = np.int32, np.uint8
ME, OWNER, THIRD = 1, 2, 4


class Session:
    """a tiler session and the host's picture of it: next_id, alive flags, one owner's map, code_of"""

    def __init__(self, extra_ids, fmap_cap, own_ids=0):
        from obia_amd import _lib
        from obia_amd.distributed import HipTilerEngine
        self._lib, self.lib = _lib, _lib.load()
        self.ctx = _lib.Context(0)                                # (a session owns its context)
        img = torch.zeros((64, 64, 1), dtype=torch.float32, device="cuda")
        self.e = HipTilerEngine(img, None, 64, 0, 64, 8, 4, (1.0, 1.0), {}, extra_ids, ctx=self.ctx)
        self.id_cap = self._id_cap()
        self.next_id = 1
        self.alive = np.zeros(self.id_cap, U8)
        if own_ids:                                               # ids of my own, as a tile pass would have left them
            self.e.set_segments(1, torch.full((own_ids,), 9, dtype=torch.int64))
            self.alive[1:1 + own_ids] = 1
            self.next_id = 1 + own_ids
        self.fmap = np.zeros(fmap_cap, I32)
        self.code_of = -(np.arange(self.id_cap + 8, dtype=I32) + 1)        # known, non-zero: whatever is not a new id's entry keeps it
        self.upload()

    def _id_cap(self):
        """the largest count obia_tiler_get_alive takes (a host check, nothing is copied when it refuses)"""
        probe = torch.zeros((1 << 22,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        lo, hi = 0, probe.numel()                                 # lo is taken, hi is refused
        assert self.lib.obia_tiler_get_alive(self.e.h, probe.data_ptr(), hi) == self._lib.E_INVALID
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if self.lib.obia_tiler_get_alive(self.e.h, probe.data_ptr(), mid) == self._lib.OBIA_OK:
                lo = mid
            else:
                hi = mid
        return lo

    def upload(self):
        self.fmap_t, self.code_of_t = dev(self.fmap), dev(self.code_of)

    def grow_map(self, t_max):
        """as ShardedTiler._ids_of_kernel grows it"""
        grown = np.zeros(min(1 << SR.CODE_SHIFT, 1 << (2 * int(t_max) + 2).bit_length()), I32)
        grown[:len(self.fmap)] = self.fmap
        self.fmap = grown
        self.fmap_t = dev(grown)

    def call(self, codes, k=1):
        """the entry point itself: (rc, guarded ids, first, n_new, t_max)"""
        ct = dev(codes)
        snap = snapshot(ct)
        g = guarded(codes.shape, I32, POISON, "cuda", k)
        first, n_new, t_max = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
        rc = self.lib.obia_tiler_import_seam(self.e.h, ct.data_ptr(), int(codes.size), ME, OWNER, self.fmap_t.data_ptr(), len(self.fmap),
                                             self.code_of_t.data_ptr(), g.ptr, ctypes.byref(first), ctypes.byref(n_new), ctypes.byref(t_max))
        torch.cuda.synchronize()
        assert unchanged(ct, snap)
        return rc, g, first.value, n_new.value, t_max.value

    def state_is(self, name):
        """the device's maps, the id counter and the alive flags equal the host's picture, every element"""
        assert np.array_equal(self.fmap_t.cpu().numpy(), self.fmap), f"{name}: fmap"
        assert np.array_equal(self.code_of_t.cpu().numpy(), self.code_of), f"{name}: code_of"
        assert self.e.next_id() == self.next_id, (name, self.e.next_id(), self.next_id)
        g = guarded((self.id_cap,), U8, POISON, "cuda", 1)
        assert self.lib.obia_tiler_get_alive(self.e.h, g.ptr, self.id_cap) == self._lib.OBIA_OK, self._lib.last_error()
        torch.cuda.synchronize()
        judge(g, self.alive, f"{name}: alive")

    def imports(self, codes, name):
        """one good import against the restatement; returns the restatement's result"""
        r = SR.import_seam(codes, ME, OWNER, self.fmap, self.code_of, self.next_id)
        assert self.next_id + r["n_new"] <= self.id_cap, "the case needs more extra_ids"
        rc, g, first, n_new, t_max = self.call(codes)
        assert rc == self._lib.OBIA_OK, (name, rc, self._lib.last_error())
        assert (first, n_new, t_max) == (r["first"], r["n_new"], r["t_max"]), (name, (first, n_new, t_max), (r["first"], r["n_new"], r["t_max"]))
        judge(g, r["ids"], f"{name}: ids")
        self.fmap, self.code_of = r["fmap"], r["code_of"]
        self.alive[self.next_id:self.next_id + n_new] = 1
        self.next_id += n_new
        self.state_is(name)
        return r

    def close(self):
        self.e.close()
        self.ctx.close()


def map_some(s, rs, ids, fraction):
    """a share of `ids` of the owner is in the map already (imported earlier: local ids of mine below next_id), and fmap[0] -- the entry
    of no id -- holds a value that must never come out"""
    known = ids[rs.rand(len(ids)) < fraction]
    s.fmap[known] = rs.randint(1, s.next_id, len(known))
    s.fmap[0] = 4242
    s.upload()
    return known


def sort_limit():
    from obia_amd import _lib
    limit = int(_lib.load().obia_test_seam_sort_limit())
    assert limit >= 2048 and limit & (limit - 1) == 0             # the bitonic sort pads to a power of two: the limit itself is its full width
    return limit


N_NEW = {"1": lambda L: 1, "2": lambda L: 2, "1025": lambda L: 1025, "limit-1": lambda L: L - 1, "limit": lambda L: L,
         "limit+1": lambda L: L + 1, "2.5xlimit": lambda L: 5 * L // 2}


@pytest.mark.parametrize("which", list(N_NEW))
def test_new_ids_on_both_sides_of_the_sort_limit(which):
    """n_new new ids, shuffled, each two to five times on the seam, from a sparse range with gaps, among codes of every other kind:
    up to the limit one workgroup sorts them in LDS (at the limit: all 64 KiB of it), one more goes to the counting kernel"""
    n_new = N_NEW[which](sort_limit())
    rs = np.random.RandomState(n_new)
    cap = 4 * n_new + 200
    s = Session(n_new + 64, cap, own_ids=40)
    try:
        pool = rs.permutation(np.arange(1, cap))                  # distinct ids of the owner below the map's end
        new, old = np.sort(pool[:n_new]), pool[n_new:n_new + 50]
        assert n_new < 1025 or ((np.diff(new) > 1).sum() > n_new // 2 and new.max() > 3 * n_new)      # sparse, with gaps
        s.fmap[old] = rs.randint(1, s.next_id, len(old))
        s.fmap[0] = 4242
        s.fmap[pool[n_new + 50:n_new + 90]] = 7                   # mapped ids the seam does not carry: left alone
        s.upload()
        t = np.concatenate([np.repeat(new, rs.randint(2, 6, n_new)), old, old[:9]])
        codes = np.concatenate([SR.code(OWNER, t), SR.code(ME, rs.randint(0, 500, 30)), SR.code(THIRD, new[:20]), np.zeros(25, I32),
                                SR.code(OWNER, [0, cap, cap + 3]), [-1]]).astype(I32)
        rs.shuffle(codes)
        r = s.imports(codes, which)
        assert r["n_new"] == n_new and r["t_max"] == cap + 3
        again = s.imports(codes, which + " again")
        assert again["n_new"] == 0 and np.array_equal(again["ids"], r["ids"])
    finally:
        s.close()


def seam_of_two_trips(rs, n, first_trip, cap, known, new_first, new_both, new_second, beyond):
    """n codes of every kind; the codes from `first_trip` on are the second trip's: `new_second` occurs only there, `new_both` on
    both sides, `new_first` only in front"""
    kinds = rs.choice(7, n, p=[0.15, 0.15, 0.1, 0.2, 0.05, 0.3, 0.05])
    t = np.zeros(n, np.int64)
    o = np.full(n, OWNER)
    o[kinds == 1], t[kinds == 1] = ME, rs.randint(0, 5000, (kinds == 1).sum())
    o[kinds == 2], t[kinds == 2] = THIRD, rs.randint(1, cap, (kinds == 2).sum())
    t[kinds == 3] = rs.choice(known, (kinds == 3).sum())
    t[kinds == 4] = rs.choice(beyond, (kinds == 4).sum())
    front = np.arange(n) < first_trip
    for sel, pools in ((front, (new_first, new_both)), (~front, (new_second, new_both))):
        m = (kinds >= 5) & sel
        t[m] = rs.choice(np.concatenate(pools), m.sum())
    codes = SR.code(o, t)
    codes[kinds == 0] = 0
    codes[rs.randint(0, n, 40)] = -rs.randint(1, 1 << 30, 40)
    return codes.astype(I32)


def test_the_second_trip_then_the_same_seam_then_a_grown_map():
    n, = crossed("tiler_seam")
    first_trip = LG.crossing("tiler_seam", (1,), 0, "x") - 1     # codes one trip of the grid takes
    assert n - first_trip >= 256
    rs = np.random.RandomState(31)
    cap = 1 << 15
    s = Session(40000, cap, own_ids=300)
    try:
        pool = rs.permutation(np.arange(1, cap))
        known, new_first, new_both, new_second = pool[:6000], pool[6000:26000], pool[26000:26060], pool[26060:26120]
        beyond = np.arange(cap, cap + 5000)
        map_some(s, rs, known, 1.0)
        s.fmap[pool[27000:27500]] = 11                            # mapped, not on the seam
        s.upload()
        codes = seam_of_two_trips(rs, n, first_trip, cap, known, new_first, new_both, new_second, beyond)
        r = s.imports(codes, "two trips")
        front, back = codes[:first_trip].astype(np.int64), codes[first_trip:].astype(np.int64)

        def new_in(part):
            t = part[(part > 0) & ((part >> SR.CODE_SHIFT) - 1 == OWNER)] & SR.ID_MASK
            return set(t[(t > 0) & (t < cap)].tolist()) - set(known.tolist())
        only_second, both = new_in(back) - new_in(front), new_in(back) & new_in(front)
        assert len(only_second) >= 10 and len(both) >= 10 and r["n_new"] == len(new_in(back) | new_in(front)) > 10000
        assert r["t_max"] >= cap and (r["ids"][first_trip:] > 0).sum() > 100
        again = s.imports(codes, "the same seam")
        assert again["n_new"] == 0 and np.array_equal(again["ids"], r["ids"])
        s.grow_map(r["t_max"])                                    # ... and what ShardedTiler._ids_of_kernel does next: the ids beyond the map
        grown = s.imports(codes, "grown map")
        assert grown["t_max"] == r["t_max"] < len(s.fmap) and 0 < grown["n_new"] <= len(beyond)
        assert np.array_equal(grown["ids"][r["ids"] != 0], r["ids"][r["ids"] != 0]) and (grown["ids"] != 0).sum() > (r["ids"] != 0).sum()
    finally:
        s.close()


def test_an_import_without_room_is_refused_and_leaves_no_claim():
    """next_id + n_new > id_cap: OBIA_E_NOMEM, and the map, code_of, the id counter and the alive flags are what they were -- the map
    entries the first kernel had claimed (-1) included, so the same ids can be imported once there is room (here: a smaller seam
    first, which fills the session to its last id)."""
    rs = np.random.RandomState(32)
    cap = 1 << 13
    s = Session(0, cap, own_ids=10)
    try:
        room = s.id_cap - s.next_id
        assert 100 < room < cap // 4
        pool = rs.permutation(np.arange(1, cap))
        known = map_some(s, rs, pool[:200], 1.0)
        fits, one_more = pool[200:200 + room], pool[200:200 + room + 1]

        def seam(new):
            t = np.concatenate([np.repeat(new, rs.randint(1, 4, len(new))), known])
            codes = np.concatenate([SR.code(OWNER, t), SR.code(ME, [5, 6]), [0, 0]]).astype(I32)
            rs.shuffle(codes)
            return codes
        rc, g, first, n_new, t_max = s.call(seam(one_more))
        assert rc == s._lib.E_NOMEM and "capacity" in s._lib.last_error(), (rc, s._lib.last_error())
        assert g.stray().size == 0
        s.state_is("refused")
        r = s.imports(seam(fits), "fits exactly")
        assert r["n_new"] == room and s.next_id == s.id_cap
        rc, g, first, n_new, t_max = s.call(seam(pool[2000:2300]))       # a full session: 300 more are refused
        assert rc == s._lib.E_NOMEM and g.stray().size == 0
        s.state_is("refused when full")
        again = s.imports(seam(fits), "after the refusals")
        assert again["n_new"] == 0 and (again["ids"] > 0).sum() >= room + len(known)
    finally:
        s.close()
