"""The label-domain passes of a tile batch (tiling.hip): the occupancy map of the label raster that lets tile_count_inside_kernel and
tile_mask_kernel skip blocks known to hold only zeros, the valid count that tile_mask_kernel adds up while it writes the mask, and
tile_scatter_kernel resolving a label only where the parent changes down a column.  All of it is integer work: every bar is exact --
np.array_equal on label rasters, == on segment counts -- against oracle/tiler.py, and the map switched off (OBIA_G_OCCUPANCY=0, read once
per call) must give the same raster as the map switched on.  Windows are chosen so that they are unaligned to the map's 64 x 64 blocks
on every side.  (Cases below compactness 5 compare with the oracle under its integer centroid sums, as tests/test_gpu_tiling_random.py
does: the reference's float32 sums can flip a near-tie there, which is no concern of these passes.)"""
import numpy as np
import pytest

from tests.test_gpu_tiling_random import make_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def synth(H, W, C, seed=0):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([350 * np.sin(xx / (9 + 3 * c)) * np.cos(yy / (12 + 2 * c)) + 900 + 60 * c + rs.normal(0, 22, (H, W))
                     for c in range(C)], -1).astype(np.float32)


def oracle_tiled(oracle, img, mask, kw):
    from oracle import tiler
    okw = dict(kw)
    okw["white_order"] = 1 if okw.pop("white_order", "raster") == "parity" else 0
    integer_sums = okw.get("compactness", 10.0) < 5.0
    if integer_sums:
        oracle.set_sum_mode(1)
    try:
        return tiler.create_tiled_segments(img, mask, **okw)
    finally:
        if integer_sums:
            oracle.set_sum_mode(0)


def hip_tiled(img, mask, kw):
    from obia_amd.tiling import create_tiled_segments
    lab, n = create_tiled_segments(torch.as_tensor(img).cuda(), input_mask=mask, **kw)
    return lab.cpu().numpy(), n


def check_on_off_oracle(oracle, monkeypatch, img, mask, kw, what):
    """the result with the map, without it, and the oracle's: identical"""
    ref, n_ref = oracle_tiled(oracle, img, mask, kw)
    monkeypatch.delenv("OBIA_G_OCCUPANCY", raising=False)
    lab, n = hip_tiled(img, mask, kw)
    monkeypatch.setenv("OBIA_G_OCCUPANCY", "0")
    off, n_off = hip_tiled(img, mask, kw)
    monkeypatch.delenv("OBIA_G_OCCUPANCY")
    assert n_off == n_ref and np.array_equal(off, ref), f"{what}, map off: {(off != ref).sum()} px differ from the oracle, n {n_off} vs {n_ref}"
    assert n == n_ref and np.array_equal(lab, ref), f"{what}, map on: {(lab != ref).sum()} px differ from the oracle, n {n} vs {n_ref}"
    if mask is not None:
        assert (lab[~np.asarray(mask, bool)] == 0).all()
    return lab, n


# tile in {80, 100, 150} together with buffer in {9, 13, 15, 25, 30}: (seed: tile, buffer) 2: 150, 30; 14: 80, 30; 25: 150, 30 (9 bands);
# 37: 80, 30 (compactness 0.25); 54: 150, 15 (0.25); 56: 80, 13; 62: 100, 9; 72: 150, 13; 85: 100, 15; 116: 150, 25
@pytest.mark.parametrize("seed", [2, 14, 25, 37, 54, 56, 62, 72, 85, 116])
def test_map_on_equals_map_off_equals_oracle_on_unaligned_windows(oracle, monkeypatch, seed):
    img, mask, kw = make_case(seed)
    assert kw["tile_size"] in (80, 100, 150) and kw["buffer"] in (9, 13, 15, 25, 30)
    check_on_off_oracle(oracle, monkeypatch, img, mask, kw, f"seed {seed} {img.shape} {kw}")


def hand_made(name):
    H, W = 200, 260
    img = synth(H, W, 4, 11)
    kw = dict(crown_radius=4.0, pixel_size=(1.0, 1.0), compactness=10.0)
    mask = None
    if name == "windows_cut_blocks_in_half":
        kw.update(tile_size=64, buffer=16)
    elif name == "one_batch_per_white_tile":          # tile_size <= 2 * buffer
        kw.update(tile_size=64, buffer=32)
    elif name == "parity_classes":                    # a window meets windows processed before and after it in raster order
        kw.update(tile_size=128, buffer=24, white_order="parity")
    elif name == "mask_empties_whole_tiles":          # skipped tiles never scatter: their blocks stay clear while a neighbour's window reaches in
        kw.update(tile_size=64, buffer=16)
        mask = np.ones((H, W), bool)
        mask[0:64, 0:64] = False                      # a black tile
        mask[64:128, 128:192] = False                 # a black tile in the middle
        mask[0:64, 64:128] = False                    # a white tile
        mask[128:200, 192:260] = False                # the last black tile, clipped by the raster
        mask[70:120, 70:75] = False
    else:
        raise KeyError(name)
    return img, mask, kw


@pytest.mark.parametrize("name", ["windows_cut_blocks_in_half", "one_batch_per_white_tile", "parity_classes", "mask_empties_whole_tiles"])
def test_map_on_equals_map_off_equals_oracle_hand_made(oracle, monkeypatch, name):
    img, mask, kw = hand_made(name)
    check_on_off_oracle(oracle, monkeypatch, img, mask, kw, name)


# islands inside white tiles, everything around them masked (make_case kind 4), whose islands reach into the corner squares;
# (seed: tile, buffer) 66: 80, 9; 83: 150, 9; 90: 64, 15; 125: 80, 15
@pytest.mark.parametrize("seed", [66, 83, 90, 125])
def test_a_window_that_meets_nothing_segments_its_corner_squares(oracle, monkeypatch, seed):
    """tile_any == 0 for such a window: every block it touches is clear, no label is read, the mask stays as read and the corner
    squares ARE segmented (tiling.py:261-262)"""
    from oracle import tiler
    img, mask, kw = make_case(seed)
    assert kw["compactness"] >= 5.0
    t = tiler.OracleTiler(img, mask, img.shape[0], 0, **kw)
    nty = -(-img.shape[0] // kw["tile_size"])
    t.run(False, 0, nty)
    t.run(True, 0, nty)
    assert t.untouched_white_tiles, "the case must have a white window that no existing segment meets"
    lab, n = check_on_off_oracle(oracle, monkeypatch, img, mask, kw, f"seed {seed}")
    T, B = kw["tile_size"], kw["buffer"]
    H, W = mask.shape
    seen = 0
    for tj, ti in t.untouched_white_tiles:
        y1, x0, x1 = min(H, tj * T + T + B), max(0, ti * T - B), min(W, ti * T + T + B)
        for sq in (np.s_[y1 - t.cly:y1, x0:x0 + t.clx], np.s_[y1 - t.cly:y1, x1 - t.clx:x1]):
            assert (lab[sq][mask[sq]] > 0).all(), "a valid pixel of a corner square of an untouched window has no segment"
            seen += int(mask[sq].sum())
    assert seen > 0, "no corner square of an untouched window holds a valid pixel: the case shows nothing"


def test_the_session_reads_every_label_the_caller_wrote(oracle):
    """Through obia_tiler_* (the sharded driver's route) the raster is the caller's, who writes it between the calls: ids put into the
    INTERIOR of a white tile after the black pass -- blocks that no scatter of the session has touched, so a map would call them empty --
    must be met by the white pass like any existing segment: the one registered with its true size lies within the polygon and is
    dropped and re-segmented, the one registered with the size of an imported seam segment (0xffffffff: never `within`) is kept and
    masked out.  Expected raster: the oracle's session with the same writes."""
    from obia_amd.distributed import HipTilerEngine
    from oracle import tiler
    H, W, T, B = 300, 320, 128, 16
    img = synth(H, W, 4, 5)
    kw = dict(tile_size=T, buffer=B, crown_radius=4.0, pixel_size=(1.0, 1.0), compactness=10.0)
    t = tiler.OracleTiler(img, None, H, 0, **kw)
    e = HipTilerEngine(torch.as_tensor(img).cuda(), torch.ones((H, W), dtype=torch.uint8, device="cuda"), H, 0, T, B, 4.0, (1.0, 1.0),
                       dict(compactness=10.0), 8)
    try:
        nty = -(-H // T)
        e.run(False, 0, nty)
        t.run(False, 0, nty)
        first = t.next_id
        assert e.next_id() == first and np.array_equal(e.G.cpu().numpy(), t.G)
        within, seam = np.s_[40:43, 150:171], np.s_[20:24, 140:181]        # both inside the block rows 0..63, columns 128..191 of white tile (0, 1)
        assert not t.G[0:64, 128:192].any(), "the block must be untouched by the black pass"
        for G in (t.G, e.G):
            G[within] = first
            G[seam] = first + 1
        sizes = [3 * 21, tiler.HUGE]
        t.set_segments(first, sizes)
        e.set_segments(first, torch.tensor(sizes))
        for parity in (0, 1):
            e.run(True, 0, nty, parity)
            t.run(True, 0, nty, parity)
        G = e.G.cpu().numpy()
        alive = e.get_alive(t.next_id).cpu().numpy()
        assert e.next_id() == t.next_id
        assert (G[seam] == first + 1).all() and alive[first + 1] == 1, "the imported ids did not survive the white pass"
        assert alive[first] == 0 and (G[within] > first + 1).all(), "the segment within the polygon was not dropped and re-segmented"
        assert np.array_equal(G, t.G), f"{(G != t.G).sum()} px differ from the oracle's session"
        assert np.array_equal(alive[1:], np.array([t.alive[g] for g in range(1, t.next_id)], np.uint8))
    finally:
        e.close()


def thin_pieces_and_holes(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    mask = np.zeros((H, W), bool)
    mask[:, ::9] = True                                   # one-pixel columns
    mask[::7, :] = True                                   # one-pixel rows
    mask[H // 5:H // 2, W // 6:W // 2] = True             # a solid piece across tile seams
    mask[(yy % 23 == 5) & (xx % 17 == 3)] = False         # single-pixel holes
    mask[H // 4:H // 4 + 30, W // 4:W // 4 + 41] = False  # a larger hole
    return mask


@pytest.mark.parametrize("shape", [(300, 320), (70, 90)])
def test_valid_counts_from_the_mask_kernel(oracle, monkeypatch, shape):
    """n_segments of a tile = round(valid x pixel_area / crown_area): a wrong count changes the tile's seeds, so the raster pins it.
    300 x 320 at tile 128, buffer 16: the four-pixel form of the mask kernel, black and white batches; 70 x 90 (one tile, a row pitch
    that is no multiple of four): its one-pixel form."""
    H, W = shape
    img = synth(H, W, 4, 3)
    mask = thin_pieces_and_holes(H, W)
    kw = dict(tile_size=128, buffer=16, crown_radius=3.0, pixel_size=(1.0, 1.0), compactness=10.0)
    check_on_off_oracle(oracle, monkeypatch, img, mask, kw, f"{shape}")


def run_start_case(name):
    H, W = 200, 260
    kw = dict(tile_size=128, buffer=16, crown_radius=4.0, pixel_size=(1.0, 1.0), compactness=10.0)
    mask = None
    if name == "salt_and_pepper":                         # most components below min_size: the small_final path (a quarter of the segments
        rs = np.random.RandomState(21)                    # of the clean raster are left, some pixels end without a labelled neighbour)
        img = synth(H, W, 3, 21)
        hit = rs.rand(H, W) < 0.4
        img[hit] += (rs.rand(int(hit.sum()), 3).astype(np.float32) - 0.5) * 1500
        kw["compactness"] = 0.25
    elif name == "single_pixel_holes":                    # parents alternate with -1 down a column
        img = synth(H, W, 4, 8)
        yy, xx = np.mgrid[0:H, 0:W]
        mask = ~((yy % 2 == 1) & (xx % 3 == 0))
    elif name == "flat":                                  # one run per column and segment: the flattest raster that is segmented, two faint
        img = np.zeros((H, W, 2), np.float32)             # ramps (a band without any range makes its tile an empty tile: `constant`)
        img[:, :, 0] = np.arange(W, dtype=np.float32)[None, :] * 1e-3 + 5.0
        img[:, :, 1] = np.arange(H, dtype=np.float32)[:, None] * 1e-3 + 7.0
    elif name == "constant":                              # every tile is skipped: nothing is scattered, no block is ever occupied
        img = np.full((H, W, 2), 3.0, np.float32)
    else:
        raise KeyError(name)
    return img, mask, kw


@pytest.mark.parametrize("name", ["salt_and_pepper", "single_pixel_holes", "flat", "constant"])
def test_labels_resolved_at_run_starts(oracle, monkeypatch, name):
    img, mask, kw = run_start_case(name)
    lab, n = check_on_off_oracle(oracle, monkeypatch, img, mask, kw, name)
    assert (n == 0) == (name == "constant")
