"""Diagnostic: what the run kernel of the spatial pre-pass (slic_spatial.hip) does on the bench's raster and tiling -- row segments,
candidates walked, segments proven from their ends, crossings looked for, queued ranges and pixels, runs, and the ticks per phase.
   tools/build_variant.sh rs -DOBIA_RUN_STATS
   OBIA_HIP_LIB=obia_amd/csrc/libobia_hip_rs.so python tools/prepass_run_stats.py [size]"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bench import synth_raster
from obia_amd import _lib
from obia_amd.tiling import create_tiled_segments
_lib.load()
N = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
dev = torch.device("cuda:0")
img = synth_raster(N, N, 8, seed=3, device=dev)
mask = torch.ones((N, N), dtype=torch.uint8, device=dev)
lib = ctypes.CDLL(_lib.LIB_PATH)
buf = np.zeros(16, np.uint64)
lib.obia_debug_run_stats(buf.ctypes.data_as(ctypes.c_void_p), 1)
create_tiled_segments(img, input_mask=mask, tile_size=2048, buffer=64, crown_radius=5, pixel_size=(0.5, 0.5), compactness=10.0)
torch.cuda.synchronize()
lib.obia_debug_run_stats(buf.ctypes.data_as(ctypes.c_void_p), 0)
s = buf.astype(np.float64)
waves = s[0]; tiles = waves / 4.0
print("waves %.0f (tile launches ~ %.0f)" % (waves, tiles))
print("per tile: segments %.1f  candidates per segment %.2f  proven from the ends %.1f  crossing searches %.1f  queued ranges %.1f  queued pixels %.1f  runs %.1f"
      % (s[1] / tiles, s[2] / max(s[1], 1), s[3] / tiles, s[4] / tiles, s[5] / tiles, s[6] / tiles, s[7] / tiles))
names = ["staging", "pruning", "walk", "queue", "barrier+flush"]
tot = s[8:13].sum()
for i, n in enumerate(names):
    print("  %-14s %8.0f ticks per wave  %5.1f %%" % (n, s[8 + i] / waves, 100 * s[8 + i] / tot))
