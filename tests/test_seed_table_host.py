"""The seed-table options, host side: the public names and the argument checks of obia_amd.seeds that fire before the device is
touched."""
import numpy as np
import pytest

STAGES = ("sample_heights", "stage1_clusters", "reduce_stage1", "split_clusters_by_height", "trim_clusters", "nms_per_crown")


def _seeds(n=3, col="ch_max"):
    out = {"x": np.arange(n, dtype=np.float64), "y": np.zeros(n)}
    if col:
        out[col] = np.full(n, 5, np.float32)
    return out


COST = np.zeros((4, 4), np.float32)


@pytest.fixture()
def no_device(monkeypatch):
    """Any use of the library fails the test."""
    from obia_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device library was used")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "default_context", boom)


def test_public_names():
    import inspect
    import obia_amd
    from obia_amd import seeds
    for name in ("canonical_seeds", "stage1_rounds") + STAGES:
        assert getattr(obia_amd, name) is getattr(seeds, name)
    sig = inspect.signature(seeds.canonical_seeds)
    want = dict(chm=None, chm_affine=None, eps_scale=0.4, min_eps=2, max_eps=8, z_thresh=-1, min_samples=2, merge_radius=1.5, cost_weight=0.5,
                xy_thresh=0.8, dz_merge=0, keep_all_stage1=True, stage1_top=1, max_per_cluster=0, nms_base=0, nms_scale=0, debug_dist=True,
                nodata_cost=1, cost_nodata=None, cost_affine=None, ctx=None)
    assert list(sig.parameters)[:4] == ["chm_seeds", "den_seeds", "cost_surface", "out_path"]
    assert {k: p.default for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY} == want
    assert list(sig.parameters)[4:] == list(want)
    assert "canonical_seeds" in seeds.make_canonical_seeds.__doc__ and "canonical_seeds" in seeds.__doc__


BAD_OPTIONS = [(dict(min_eps=-0.5), "min_eps must not be negative"), (dict(min_eps=9), "min_eps must not exceed max_eps"),
               (dict(min_eps=3, max_eps=2.5), "min_eps must not exceed max_eps"), (dict(min_samples=0), "min_samples"),
               (dict(min_samples=-2), "min_samples"), (dict(min_samples=2.5), "min_samples"), (dict(eps_scale=float("inf")), "eps_scale"),
               (dict(z_thresh=float("nan")), "z_thresh"), (dict(dz_merge=float("nan")), "dz_merge"), (dict(dz_merge=1e-60), "dz_merge"),
               (dict(max_per_cluster=1.5), "max_per_cluster"), (dict(nms_base=float("nan")), "nms_base"),
               (dict(nms_scale=float("inf")), "nms_scale")]


@pytest.mark.parametrize("kw,message", BAD_OPTIONS, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in BAD_OPTIONS])
def test_options_are_checked_before_device_use(no_device, kw, message):
    from obia_amd.seeds import canonical_seeds
    with pytest.raises(ValueError, match=message):
        canonical_seeds(_seeds(), _seeds(col="den_max"), COST, **kw)


def test_tables_are_checked_before_device_use(no_device):
    from obia_amd.seeds import canonical_seeds
    nan = _seeds()
    nan["ch_max"] = np.array([5, np.nan, 5], np.float32)
    with pytest.raises(ValueError, match="heights contain NaN"):
        canonical_seeds(nan, _seeds(col="den_max"), COST)
    with pytest.raises(ValueError, match="heights contain NaN"):
        canonical_seeds(_seeds(), dict(_seeds(col=None), height=[1.0, 2.0, float("nan")]), COST)
    with pytest.raises(ValueError, match="chm is needed"):
        canonical_seeds(_seeds(col=None), _seeds(col="den_max"), COST)
    with pytest.raises(ValueError, match="chm is needed"):
        canonical_seeds(_seeds(), _seeds(col=None), COST, dz_merge=1.0)
    short = _seeds()
    short["ch_max"] = short["ch_max"][:2]
    with pytest.raises(ValueError, match="one length"):
        canonical_seeds(short, _seeds(col="den_max"), COST)
    with pytest.raises(ValueError, match="one length"):
        canonical_seeds(_seeds(), dict(_seeds(col="den_max"), y=np.zeros(4)), COST)
    with pytest.raises(ValueError, match="one length"):
        canonical_seeds(_seeds(col=None), dict(_seeds(col=None), x=np.zeros((3, 1))), COST, chm=COST)
    with pytest.raises(ValueError, match="dict with x and y"):
        canonical_seeds([1, 2, 3], _seeds(col="den_max"), COST)
    with pytest.raises(ValueError, match="cost_surface must be"):
        canonical_seeds(_seeds(), _seeds(col="den_max"), np.zeros((4, 4, 2), np.float32))
    with pytest.raises(ValueError, match="chm must be"):
        canonical_seeds(_seeds(col=None), _seeds(col="den_max"), COST, chm=np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="singular"):
        canonical_seeds(_seeds(), _seeds(col="den_max"), COST, cost_affine=[1, 1, 1, 1, 0, 0])


def test_stage_functions_are_checked_before_device_use(no_device):
    from obia_amd import seeds
    x, y, h, c = np.zeros(3), np.zeros(3), np.ones(3, np.float32), np.zeros(3, np.int32)
    bad_h = np.array([1, np.nan, 2], np.float32)
    for call in (lambda: seeds.stage1_clusters(x, y[:2], h), lambda: seeds.reduce_stage1(c, h[:2]), lambda: seeds.trim_clusters(c[:1], h, 2),
                 lambda: seeds.split_clusters_by_height(c, np.ones((3, 1), np.float32), 1.0), lambda: seeds.nms_per_crown(x, y, h, c[:2], 1.0, 0),
                 lambda: seeds.sample_heights(x, y[:2], COST)):
        with pytest.raises(ValueError, match="one length"):
            call()
    for call in (lambda: seeds.stage1_clusters(x, y, bad_h), lambda: seeds.reduce_stage1(c, bad_h), lambda: seeds.trim_clusters(c, bad_h, 2),
                 lambda: seeds.split_clusters_by_height(c, bad_h, 1.0), lambda: seeds.nms_per_crown(x, y, bad_h, c, 1.0, 0)):
        with pytest.raises(ValueError, match="heights contain NaN"):
            call()
    for call in (lambda: seeds.stage1_clusters(x[:0], y[:0], h[:0]), lambda: seeds.trim_clusters(c[:0], h[:0], 2),
                 lambda: seeds.sample_heights(x[:0], y[:0], COST)):
        with pytest.raises(ValueError, match="no seeds"):
            call()
    with pytest.raises(ValueError, match="min_eps must not be negative"):
        seeds.stage1_clusters(x, y, h, min_eps=-1)
    with pytest.raises(ValueError, match="min_eps must not exceed max_eps"):
        seeds.stage1_clusters(x, y, h, min_eps=5, max_eps=4)
    with pytest.raises(ValueError, match="min_samples"):
        seeds.stage1_clusters(x, y, h, min_samples=0)
    with pytest.raises(ValueError, match="max_per_cluster"):
        seeds.trim_clusters(c, h, 2.5)
    with pytest.raises(ValueError, match="dz_merge"):
        seeds.split_clusters_by_height(c, h, float("nan"))
    with pytest.raises(ValueError, match="nms_base"):
        seeds.nms_per_crown(x, y, h, c, float("nan"), 0)
    with pytest.raises(ValueError, match="chm must be"):
        seeds.sample_heights(x, y, np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError, match="singular"):
        seeds.sample_heights(x, y, COST, [1, 1, 1, 1, 0, 0])


def test_more_than_2_31_rows_are_refused(no_device):
    from obia_amd import seeds

    class Huge:
        shape = (2 ** 31,)
    with pytest.raises(ValueError, match="fewer than 2\\^31 rows"):
        seeds.stage1_clusters(Huge(), Huge(), Huge())
    with pytest.raises(ValueError, match="fewer than 2\\^31 rows"):
        seeds.trim_clusters(Huge(), Huge(), 3)


def test_a_cpu_tensor_is_refused(no_device):
    torch = pytest.importorskip("torch")
    from obia_amd import seeds
    with pytest.raises(ValueError, match="must live on the GPU"):
        seeds.stage1_clusters(torch.zeros(3, dtype=torch.float64), np.zeros(3), np.ones(3, np.float32))
    with pytest.raises(ValueError, match="must live on the GPU"):
        seeds.canonical_seeds(_seeds(), _seeds(col="den_max"), torch.zeros(4, 4))
