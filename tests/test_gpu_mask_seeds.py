"""``seeding="skimage"`` on the GPU: obia_mask_centroids_dev against scikit-image 0.18.3's own output (the fixtures' `seeds_yx` /
`seed_steps_all`) and against the NumPy restatement (tests/mask_seeds_restatement.py, itself pinned on the fixtures and on SciPy by
tests/test_mask_seeds_restatement_cpu.py).  Every comparison is bit equality: the routine is integer sums, IEEE divisions and square
roots and argmins with a fixed tie rule, so no tolerance exists to be measured."""
import ast
import os

import numpy as np
import pytest
import torch

from tests import mask_seeds_restatement as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIRING = ("mask_128x160x4_c025", "mask_128x160x4_c10", "maskones_96x96x4")


@pytest.fixture(scope="module")
def seg():
    from obia_amd import _lib, segmentation
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return segmentation


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return z, ast.literal_eval(str(z["params"]))


def slic_kwargs(params):
    return dict(n_segments=params["n_segments"], compactness=params["compactness"], max_num_iter=params.get("max_iter", 10),
                convert2lab=params.get("convert2lab", None), start_label=params.get("start_label", 1), _normalize_bands=True)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixtures_bit_for_bit_and_repeatable(seg, name):
    z, params = load(name)
    cent, steps = seg.mask_centroids(z["mask"], params["n_segments"])
    assert cent.dtype == np.float64 and cent.shape == (len(z["seeds_yx"]), 3) and not cent[:, 0].any()
    assert np.array_equal(cent[:, 1:], z["seeds_yx"]), f"{name}: {int((cent[:, 1:] != z['seeds_yx']).any(1).sum())} centroids differ"
    assert steps.dtype == np.float64 and np.array_equal(steps, z["seed_steps_all"]), f"{name}: steps {steps} vs {z['seed_steps_all']}"
    again = seg.mask_centroids(torch.as_tensor(z["mask"]).cuda(), params["n_segments"])     # (and a CUDA mask in)
    assert np.array_equal(again[0], cent) and np.array_equal(again[1], steps)


@pytest.mark.parametrize("name", WIRING)
def test_slic_with_skimage_seeding_is_the_seeded_call(seg, name):
    """``slic(..., seeding="skimage")`` = ``slic(..., seeds=<scikit-image's own seeds>)``, before connectivity and in the final labels:
    it inherits the bar test_gpu_parity.py holds the seeded call to against scikit-image's labels."""
    z, params = load(name)
    raw = torch.as_tensor(z["raw"].astype(np.float32)).cuda()
    mask, kw = z["mask"], slic_kwargs(params)
    seeds = (z["seeds_yx"], z["seed_steps_all"])
    for stage in ("pre", "full"):
        want = seg.slic(raw, mask=mask, seeds=seeds, _stage=stage, **kw)
        got = seg.slic(raw, mask=mask, seeding="skimage", _stage=stage, **kw)
        assert got.dtype == torch.int32 and got.is_cuda and torch.equal(got, want), f"{name}: {stage}"


def test_numpy_image_gives_the_cuda_tensor_labels(seg):
    z, params = load("mask_128x160x4_c025")
    raw, mask, kw = z["raw"].astype(np.float32), z["mask"], slic_kwargs(params)
    host = seg.slic(raw, mask=mask, seeding="skimage", **kw)
    dev = seg.slic(torch.as_tensor(raw).cuda(), mask=torch.as_tensor(mask).cuda(), seeding="skimage", **kw)
    assert isinstance(host, np.ndarray) and host.dtype == np.int64 and np.array_equal(host, dev.cpu().numpy())
    # one layer up: create_segments marks the masked pixels -1 on top of the same labels
    tab = seg.create_segments(raw, mask=mask, seeding="skimage", **{k: v for k, v in kw.items() if k != "_normalize_bands"})
    assert np.array_equal(tab[mask != 0], host[mask != 0]) and (tab[mask == 0] == -1).all()


@pytest.fixture(scope="module")
def references():
    """(mask, n, centroids, steps, info) of every edge case, computed once."""
    out = {}
    for name in R.EDGE_CASES:
        mask, n = R.edge_case(name)
        info = {}
        cent, steps = R.mask_centroids(mask, n, info=info)
        out[name] = (mask, n, cent, steps, info)
    return out


@pytest.mark.parametrize("name", R.EDGE_CASES)
def test_edge_cases_against_the_restatement(seg, references, name):
    from obia_amd import _lib
    mask, n, cent, steps, info = references[name]
    # the case is the case it claims to be
    if name == "no_dense_draw":
        assert info["n_dense"] is None and info["n_valid"] <= 100 * n
    elif name == "n_above_n_valid":
        assert n > info["n_valid"] == info["K"]
    elif name == "empty_cluster":
        assert sum(info["empty_per_iter"]) > 0
    elif name == "ties":
        assert info["ties_first_iter"] > 0
    elif name == "chunk_plus_one":
        assert info["K"] == _lib.MASK_SEEDS_CHUNK + 1 == n
    elif name == "two":
        assert info["K"] == 2
    elif name == "single_row":
        assert mask.any(1).sum() == 1 and mask.shape[0] > 1
    elif name == "blob_k1000":
        assert mask.shape == (384, 384) and info["K"] == 1000 and info["n_valid"] > 100 * 1000 == info["n_dense"]
        assert info["K"] > _lib.MASK_SEEDS_CHUNK or info["n_dense"] > 256 * 256      # many workgroups
    got, gsteps = seg.mask_centroids(mask, n)
    assert got.shape == cent.shape
    assert np.array_equal(got, cent), f"{name}: {int((got != cent).any(1).sum())} of {len(cent)} centroids differ"
    assert np.array_equal(gsteps, steps), f"{name}: steps {gsteps} vs {steps}"


def test_several_code_book_chunks(seg):
    """K = 2 * chunk + 77 on all valid pixels of a 72 x 80 square: three LDS chunks, the last one partly filled."""
    from obia_amd import _lib
    mask, n = np.ones((72, 80), bool), 2 * _lib.MASK_SEEDS_CHUNK + 77
    cent, steps = R.mask_centroids(mask, n)
    got, gsteps = seg.mask_centroids(mask, n)
    assert len(got) == n and np.array_equal(got, cent) and np.array_equal(gsteps, steps)


def test_abi_refusals(seg):
    from obia_amd import _lib
    lib, c = _lib.load(), _lib.default_context(0)
    mask = torch.ones((20, 30), dtype=torch.uint8, device="cuda")      # 600 valid pixels
    yx, steps = np.empty((3, 2)), np.empty(3)

    def call(picks, dense=None, mask_ptr=mask.data_ptr(), out=yx, st=steps, n=None, iters=5):
        picks = None if picks is None else np.asarray(picks, np.int64)
        dense = None if dense is None else np.asarray(dense, np.int64)
        return lib.obia_mask_centroids_dev(c.handle, mask_ptr, 20, 30, _lib.np_ptr(picks), (len(picks) if n is None else n),
                                           _lib.np_ptr(dense), 0 if dense is None else len(dense), iters, _lib.np_ptr(out), _lib.np_ptr(st))

    assert call([5, 100, 599]) == _lib.OBIA_OK
    assert call([5, 100, 599], dense=np.arange(0, 600, 2)) == _lib.OBIA_OK
    for bad in ([100, 5, 599], [5, 5, 599]):                            # unsorted, repeated
        assert call(bad) == _lib.E_INVALID and "ascending" in _lib.last_error()
    assert call([5, 100, 599], dense=[7, 3, 9]) == _lib.E_INVALID and "ascending" in _lib.last_error()
    assert call([5, 100, 600]) == _lib.E_INVALID and "out of range" in _lib.last_error()      # one past the last valid pixel
    assert call([5, 100, 599], dense=[1, 2, 600]) == _lib.E_INVALID and "out of range" in _lib.last_error()
    assert call([-1, 100, 599]) == _lib.E_INVALID
    assert call(None, n=3) == _lib.E_INVALID and "null" in _lib.last_error()
    assert call([5, 100, 599], mask_ptr=None) == _lib.E_INVALID
    assert call([5, 100, 599], out=None) == _lib.E_INVALID
    assert call([5, 100, 599], st=None) == _lib.E_INVALID
    assert call([5, 100, 599], n=0) == _lib.E_INVALID
    assert call([5, 100, 599], iters=-1) == _lib.E_INVALID
    assert lib.obia_mask_centroids_dev(None, mask.data_ptr(), 20, 30, None, 0, None, 0, 5, None, None) == _lib.E_INVALID
    with pytest.raises(ValueError):
        _lib.check(call([100, 5, 599]))
    # the context is still good, and iters = 0 hands the picked pixels back
    assert call([5, 100, 599], iters=0) == _lib.OBIA_OK
    assert np.array_equal(yx, [[0, 5], [3, 10], [19, 29]])
