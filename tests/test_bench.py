"""bench.py's result line and --dump-outputs: what a step hands its caller, written as float .npy files of at most 64 MB, the same
from run to run on the same arguments."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read_dump(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_dump_outputs_samples_labels_and_statistics(tmp_path):
    """dump_outputs on host tensors of the bench's size class: float32 / float64 only, under 64 MB, the samples fixed by the seed."""
    import bench
    H, W, C, n = 3000, 1500, 8, 70000
    g = torch.Generator().manual_seed(0)
    lab = torch.randint(1, n + 1, (H, W), generator=g, dtype=torch.int32)
    st = {"count": torch.randint(0, 100, (n,), generator=g), "mean": torch.rand((n, C), generator=g, dtype=torch.float64),
          "variance": torch.rand((n, C), generator=g, dtype=torch.float64), "min": torch.rand((n, C), generator=g),
          "max": torch.rand((n, C), generator=g), "bands": list(range(C))}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), lab, n, st)
    a, b = _read_dump(tmp_path / "a"), _read_dump(tmp_path / "b")
    assert sorted(a) == sorted(b) and {"labels_row_sum", "labels_sample", "stats_mean", "n_segments"} <= set(a)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        np.testing.assert_array_equal(a[k], b[k])
    assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))) <= 64 << 20
    np.testing.assert_array_equal(a["labels_row_sum"], lab.sum(dim=1, dtype=torch.int64).numpy())
    px = a["labels_sample_index"].astype(np.int64)
    np.testing.assert_array_equal(a["labels_sample"], lab.numpy().reshape(-1)[px])
    seg = a["stats_sample_index"].astype(np.int64)
    assert len(seg) == bench.DUMP_STAT_VALUES // C
    np.testing.assert_array_equal(a["stats_min"], st["min"].numpy()[seg])
    assert a["n_segments"][0] == n


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    """Two plain runs at one tile row: one result line with the headline fields, the breakdown left to --full, identical dumps."""
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--size", "2048",
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for line in lines:
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "Mpixel/s" and line["dtype"] == "f32"
        assert line["stage_ms_per_step"] is None and line["cpu_baseline"] is None and line["quickshift"] is None
    a, b = _read_dump(tmp_path / "a"), _read_dump(tmp_path / "b")
    assert a["n_segments"][0] == lines[0]["config"]["segments"] > 0
    assert sorted(a) == sorted(b)
    for k in a:
        if k in ("stats_mean", "stats_variance"):
            # float64 sums added by atomics in no fixed order (zonal.hip), variance = E[x^2] - E[x]^2: equal up to the last bits
            np.testing.assert_allclose(a[k], b[k], rtol=1e-9, err_msg=k)
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
