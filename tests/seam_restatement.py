"""The seam import of the sharded driver (obia_tiler_import_seam, obia_amd/csrc/tiling.hip) restated in NumPy -- test infrastructure.

A segment travels as the int32 wire code ``(owner_rank + 1) << 24 | owner_local_id``.  One import translates the codes of a seam
into local ids of rank ``me`` with the help of ``fmap`` (the owner's local id -> my local id, 0: not imported yet) and notes the
wire code of every id it hands out in ``code_of`` (my local id -> wire code):

  * a code ``c <= 0`` gives id 0;
  * for a positive code, owner ``o = (c >> 24) - 1`` and id ``t = c & 0xffffff``;
  * my own rank (``o == me``) gives ``t``;
  * for the owner rank (``o == owner``), ``t_max`` is the largest ``t`` on the seam (ids beyond the map included); with
    ``0 < t < cap`` (``cap = len(fmap)``) the code gives ``fmap[t]`` where that is positive, otherwise ``t`` is a new id;
  * the new ids in ascending order get ``first + rank``: ``fmap[t] = first + rank``, ``code_of[first + rank] = t | ((owner + 1) << 24)``;
  * ``t >= cap``, ``t == 0`` and every other rank give 0.

Nothing else of ``fmap`` and ``code_of`` changes.  ``import_seam`` works on copies and returns them."""
import numpy as np

CODE_SHIFT = 24
ID_MASK = (1 << CODE_SHIFT) - 1


def code(owner, t):
    """wire code(s) of the id(s) `t` of rank(s) `owner`"""
    return (np.asarray(t, np.int64) + ((np.asarray(owner, np.int64) + 1) << CODE_SHIFT)).astype(np.int32)


def import_seam(codes, me, owner, fmap, code_of, first):
    """-> dict(ids (int32, the shape of `codes`), fmap, code_of (updated copies), first, n_new, t_max)"""
    codes = np.asarray(codes, np.int32)
    fmap, code_of = np.array(fmap, np.int32), np.array(code_of, np.int32)
    assert (fmap >= 0).all(), "a map entry below 0 is a claim of an import in flight: no import starts from one"
    cap = len(fmap)
    c = codes.reshape(-1).astype(np.int64)
    o, t = (c >> CODE_SHIFT) - 1, c & ID_MASK
    pos = c > 0
    mine = pos & (o == me)
    theirs = pos & ~mine & (o == owner)
    t_max = int(t[theirs].max()) if theirs.any() else 0
    inside = theirs & (t > 0) & (t < cap)
    known = np.zeros(len(c), bool)
    known[inside] = fmap[t[inside]] > 0
    new = np.unique(t[inside & ~known])                          # ascending, each once
    n_new = len(new)
    assert first + n_new <= len(code_of), "code_of must have room for every new id"
    fmap[new] = first + np.arange(n_new, dtype=np.int64)
    code_of[first:first + n_new] = code(owner, new)
    ids = np.zeros(len(c), np.int64)
    ids[mine] = t[mine]
    ids[inside] = fmap[t[inside]]
    return dict(ids=ids.astype(np.int32).reshape(codes.shape), fmap=fmap, code_of=code_of, first=int(first), n_new=n_new, t_max=t_max)
