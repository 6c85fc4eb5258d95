"""The entry points of include/obia_seed_table.h through guarded outputs (tests/guarded.py, both poisons) with every input off a
16-byte boundary (tests/offset_views.py): the results bit for bit, no stray write, no element left unwritten, the inputs unchanged,
two runs equal; and what is refused before anything is launched writes nothing."""
import ctypes
import functools

import numpy as np
import pytest

from tests import seed_table_restatement as T
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue
from tests.refusal_text import refused_saying

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 333                                                                      # two workgroups, the second ragged
STAGE1 = dict(eps_scale=0.4, min_eps=2.5, max_eps=8, z_thresh=16.0, min_samples=3)
SIDE = 8.0 * (1.0 + 2.0 ** -20)
AFFINE = [0.5, 0.0, 0.0, -0.5, 431000.0, 5012350.0]


@functools.lru_cache(maxsize=None)
def case():
    """a table on the half-unit lattice, its grid by the header's own rule on the host, and what every entry point must write"""
    rs = np.random.RandomState(123)
    xs = 431000.25 + 0.5 * rs.randint(0, 90, N)
    ys = 5012345.75 - 0.5 * rs.randint(0, 70, N)
    hs = rs.uniform(2, 25, N).astype(np.float32)
    hs[rs.rand(N) < 0.2] = 6.25
    cl = rs.randint(0, 60, N).astype(np.int32)
    cx, cy = np.floor(xs / SIDE).astype(np.int32), np.floor(ys / SIDE).astype(np.int32)
    ncx = int(cx.max() - cx.min()) + 3
    key = (cy.astype(np.int64) - cy.min() + 1) * ncx + (cx.astype(np.int64) - cx.min() + 1)
    order = np.argsort(key, kind="stable")
    c = dict(xs=xs, ys=ys, hs=hs, cl=cl, cx=cx, cy=cy, ncx=ncx, order=order, skey=key[order])
    fired, owner = T.fired_and_owner(xs, ys, hs, **STAGE1)
    c["fired"], c["owner"] = fired[order].astype(np.uint8), owner[order].astype(np.int32)
    c["rounds"] = T.stage1_rounds(xs, ys, hs, **STAGE1)[1]
    p = np.lexsort((np.arange(N), -hs.astype(np.float64), cl))               # (cluster, height descending, row)
    c["p"] = p
    c["seg"] = T.segments(cl[p], hs[p], 3.0)
    pos = np.empty(N, np.int32)
    pos[p] = np.arange(N, dtype=np.int32)
    c["pos"] = pos
    keep = np.zeros(N, np.uint8)
    keep[T.nms(xs, ys, hs, cl, 2.5, 0.1)] = 1
    c["keep"] = keep[order]
    rs2 = np.random.RandomState(124)
    chm = rs2.uniform(2, 25, (61, 83)).astype(np.float32)
    chm[rs2.rand(61, 83) < 0.2] = np.nan
    c["chm"] = chm
    h, kept = T.sample_heights(xs, ys, chm, AFFINE)
    valid = np.zeros(N, np.uint8)
    valid[kept] = 1
    assert 0 < valid.sum() < N and 0 < fired.sum() < N and (owner == -1).any() and 0 < keep.sum() < N and c["seg"][2].any()
    c["h"], c["valid"] = h, valid
    return c


def dev_off(a, k):
    return offset_view(torch.as_tensor(np.ascontiguousarray(a)).cuda(), k)


def judge(g, want, name):
    """the guarded output holds `want` bit for bit, nothing around it changed, nothing in it was left as it was"""
    got = g.host()
    bits = {1: np.uint8, 4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    assert np.array_equal(got.view(bits), want.view(bits)), f"{name}: {int((got.view(bits) != want.view(bits)).sum())} differ"
    poison = np.frombuffer(bytes([g.poison]) * want.dtype.itemsize, bits)[0]
    assert g.findings(exempt=want.view(bits) == poison, name=name) == []


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_buffers_off_the_boundary_and_guarded_outputs(k, poison):
    """float32 / int32 buffers 4, 8 and 12 bytes past a 16-byte boundary, float64 / int64 ones 8 bytes (k odd), byte outputs k bytes"""
    from obia_amd import _lib
    from obia_amd.seeds import invert_affine
    lib, ctx = _lib.load(), _lib.default_context(0)
    c = case()
    o, p = c["order"], c["p"]
    xs, ys, hs, cl = dev_off(c["xs"], k), dev_off(c["ys"], k), dev_off(c["hs"], k), dev_off(c["cl"], k)
    xs_s, ys_s, hs_s, cl_s = dev_off(c["xs"][o], k), dev_off(c["ys"][o], k), dev_off(c["hs"][o], k), dev_off(c["cl"][o], k)
    orig, pos_s, skey = dev_off(o.astype(np.int32), k), dev_off(c["pos"][o], k), dev_off(c["skey"], k)
    cl_p, hs_p, chm = dev_off(c["cl"][p], k), dev_off(c["hs"][p], k), dev_off(c["chm"], k)
    assert residue(xs) == (8 * k) % 16 and residue(hs) == 4 * k and residue(skey) == (8 * k) % 16
    ins = [xs, ys, hs, cl, xs_s, ys_s, hs_s, cl_s, orig, pos_s, skey, cl_p, hs_p, chm]
    snaps = [snapshot(t) for t in ins]
    H, W = c["chm"].shape
    inv6 = (ctypes.c_double * 6)(*invert_affine(AFFINE))
    s1 = [float(np.float32(STAGE1[n])) for n in ("eps_scale", "min_eps", "max_eps", "z_thresh")]
    runs = []
    for _ in range(2):
        g = {n: guarded((N,), dt, poison, "cuda", k) for n, dt in (("cx", np.int32), ("cy", np.int32), ("h", np.float32), ("valid", np.uint8),
                                                                   ("fired", np.uint8), ("owner", np.int32), ("rank", np.int32),
                                                                   ("size", np.int32), ("part", np.uint8), ("keep", np.uint8))}
        assert g["cx"].ptr % 16 == 4 * k and g["valid"].ptr % 16 == k
        rounds = ctypes.c_int32(-1)
        torch.cuda.synchronize()
        calls = [lib.obia_seedtab_cells_dev(ctx.handle, xs.data_ptr(), ys.data_ptr(), N, SIDE, g["cx"].ptr, g["cy"].ptr),
                 lib.obia_seedtab_sample_dev(ctx.handle, xs.data_ptr(), ys.data_ptr(), N, chm.data_ptr(), H, W, inv6, g["h"].ptr, g["valid"].ptr),
                 lib.obia_seedtab_stage1_dev(ctx.handle, xs_s.data_ptr(), ys_s.data_ptr(), hs_s.data_ptr(), orig.data_ptr(), skey.data_ptr(), N,
                                             c["ncx"], *s1, STAGE1["min_samples"], g["fired"].ptr, g["owner"].ptr, ctypes.byref(rounds)),
                 lib.obia_seedtab_segments_dev(ctx.handle, cl_p.data_ptr(), hs_p.data_ptr(), N, 3.0, g["rank"].ptr, g["size"].ptr, g["part"].ptr),
                 lib.obia_seedtab_nms_dev(ctx.handle, xs_s.data_ptr(), ys_s.data_ptr(), hs_s.data_ptr(), cl_s.data_ptr(), pos_s.data_ptr(),
                                          skey.data_ptr(), N, c["ncx"], 2.5, 0.1, g["keep"].ptr)]
        assert calls == [0] * 5, (calls, _lib.last_error())
        want = dict(cx=c["cx"], cy=c["cy"], h=c["h"], valid=c["valid"], fired=c["fired"], owner=c["owner"], rank=c["seg"][0], size=c["seg"][1],
                    part=c["seg"][2], keep=c["keep"])
        for n, w in want.items():
            judge(g[n], w, n)
        work = (ctypes.c_int64 * 2)()
        assert lib.obia_seedtab_last_work(ctx.handle, work) == 0
        assert rounds.value == c["rounds"] == work[0] and work[1] == N and 1 < rounds.value <= N
        runs.append({n: g[n].host().tobytes() for n in g})
    assert runs[0] == runs[1]
    assert all(unchanged(t, s) for t, s in zip(ins, snaps))
    # refused before anything is launched: nothing is written
    g = {n: guarded((N,), dt, poison, "cuda", k) for n, dt in (("a", np.int32), ("b", np.int32), ("f", np.float32), ("u", np.uint8))}
    x, y, h4, i4, k8 = xs_s.data_ptr(), ys_s.data_ptr(), hs_s.data_ptr(), orig.data_ptr(), skey.data_ptr()
    a, b, f, u = g["a"].ptr, g["b"].ptr, g["f"].ptr, g["u"].ptr
    refused = [lib.obia_seedtab_cells_dev(ctx.handle, x, y, 0, SIDE, a, b), lib.obia_seedtab_cells_dev(ctx.handle, x, y, 2 ** 31, SIDE, a, b),
               lib.obia_seedtab_cells_dev(ctx.handle, x, y, N, 0.0, a, b), lib.obia_seedtab_cells_dev(ctx.handle, x + 4, y, N, SIDE, a, b),
               lib.obia_seedtab_cells_dev(ctx.handle, x, y, N, SIDE, a + 2, b), lib.obia_seedtab_cells_dev(ctx.handle, x, None, N, SIDE, a, b),
               lib.obia_seedtab_sample_dev(ctx.handle, x, y, N, chm.data_ptr(), 0, W, inv6, f, u),
               lib.obia_seedtab_sample_dev(ctx.handle, x, y, N, chm.data_ptr() + 1, H, W, inv6, f, u),
               lib.obia_seedtab_sample_dev(ctx.handle, x, y, N, chm.data_ptr(), H, W, None, f, u),
               lib.obia_seedtab_stage1_dev(ctx.handle, x, y, h4, i4, k8, N, 2, *s1, 3, u, a, None),
               lib.obia_seedtab_stage1_dev(ctx.handle, x, y, h4, i4, k8, N, c["ncx"], s1[0], -1.0, s1[2], s1[3], 3, u, a, None),
               lib.obia_seedtab_stage1_dev(ctx.handle, x, y, h4, i4, k8, N, c["ncx"], s1[0], 9.0, s1[2], s1[3], 3, u, a, None),
               lib.obia_seedtab_stage1_dev(ctx.handle, x, y, h4, i4, k8, N, c["ncx"], *s1, 0, u, a, None),
               lib.obia_seedtab_stage1_dev(ctx.handle, x, y, h4, i4, k8 + 4, N, c["ncx"], *s1, 3, u, a, None),
               lib.obia_seedtab_stage1_dev(ctx.handle, x, y, h4, i4, k8, N, c["ncx"], *s1, 3, u, a + 1, None),
               lib.obia_seedtab_segments_dev(ctx.handle, i4, h4, N, float("nan"), a, b, u),
               lib.obia_seedtab_segments_dev(ctx.handle, i4, h4, N, 1.0, a, a, u), lib.obia_seedtab_segments_dev(ctx.handle, i4, h4, -1, 1.0, a, b, u),
               lib.obia_seedtab_nms_dev(ctx.handle, x, y, h4, i4, i4, k8, N, c["ncx"], float("nan"), 0.1, u),
               lib.obia_seedtab_nms_dev(ctx.handle, x, y, h4, i4, i4, k8, N, 1, 1.0, 0.1, u),
               lib.obia_seedtab_nms_dev(ctx.handle, x, y, h4, i4, i4, k8, N, c["ncx"], 1.0, 0.1, None)]
    assert refused == [_lib.E_INVALID] * len(refused), refused
    # ... and says so in full: a null output, an output (where it is of bytes: an input) one byte on, an output where the input it is
    # compared with starts (the non-maximum suppression compares nothing)
    hd, C = ctx.handle, chm.data_ptr()
    refused_saying("seed table: cells: bad arguments (null, misaligned or overlapping buffers)", lib.obia_seedtab_cells_dev,
                   (hd, x, y, N, SIDE, None, b), (hd, x, y, N, SIDE, a, b + 1), (hd, x, y, N, SIDE, a, a))
    refused_saying("seed table: sample: bad arguments (null, misaligned or overlapping buffers)", lib.obia_seedtab_sample_dev,
                   (hd, x, y, N, C, H, W, inv6, None, u), (hd, x, y, N, C, H, W, inv6, f, None), (hd, x, y, N, C, H, W, inv6, f + 1, u),
                   (hd, x, y, N, C, H, W, inv6, C, u))
    refused_saying("seed table: stage 1: bad arguments (null, misaligned or overlapping buffers)", lib.obia_seedtab_stage1_dev,
                   (hd, x, y, h4, i4, k8, N, c["ncx"], *s1, 3, u, None, None), (hd, x, y, h4, i4, k8, N, c["ncx"], *s1, 3, None, a, None),
                   (hd, x, y, h4, i4, k8, N, c["ncx"], *s1, 3, u, a + 1, None), (hd, x, y, h4, i4, k8, N, c["ncx"], *s1, 3, u, i4, None))
    refused_saying("seed table: segments: bad arguments (null, misaligned or overlapping buffers)", lib.obia_seedtab_segments_dev,
                   (hd, i4, h4, N, 1.0, None, b, u), (hd, i4, h4, N, 1.0, a, b, None), (hd, i4, h4, N, 1.0, a, b + 1, u),
                   (hd, i4, h4, N, 1.0, a, i4, u), (hd, i4, h4, N, 1.0, i4, b, u))
    refused_saying("seed table: nms: bad arguments (null, misaligned or overlapping buffers)", lib.obia_seedtab_nms_dev,
                   (hd, x, y, h4, i4, i4, k8, N, c["ncx"], 1.0, 0.1, None), (hd, x, y, h4 + 1, i4, i4, k8, N, c["ncx"], 1.0, 0.1, u))
    assert all(v.untouched() for v in g.values())


def test_the_wrapper_bins_as_the_header_says():
    """obia_amd.seeds._grid: the order and the keys the entry points are given are those of the rule restated in case()"""
    from obia_amd import _device, seeds
    c = case()
    x, y = torch.as_tensor(c["xs"]).cuda(), torch.as_tensor(c["ys"]).cuda()
    lib, ctx = _device.begin(0, None)
    order, skey, ncx = seeds._grid(lib, ctx, 0, x, y, 8.0)
    assert ncx == c["ncx"] and np.array_equal(order.cpu().numpy(), c["order"]) and np.array_equal(skey.cpu().numpy(), c["skey"])
