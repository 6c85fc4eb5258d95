"""Per-kernel and per-grid-size summary of a rocprofv3 kernel trace (csv):
   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --steps 6
   python tools/trace_by_kernel.py DIR STEPS [name-filter ...]
STEPS: the steps the run made, warm-up included (figures are divided by it).  The kernels whose name holds one of the filters are
also listed by grid size (default: the sweeps and the feature passes)."""
import csv, glob, os, sys
from collections import defaultdict


def main():
    d, steps = sys.argv[1], float(sys.argv[2])
    filters = sys.argv[3:] or ["slic_assign", "slic_spatial", "features_planes", "band_minmax", "slic_prep_lane", "broadcast"]
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    print(f"launches: {len(rows)} steps assumed: {steps}")
    by_name, by_grid = defaultdict(list), defaultdict(list)
    for r in rows:
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        by_name[r["Kernel_Name"]].append(us)
        by_grid[(r["Kernel_Name"], f'{r["Grid_Size_X"]}x{r["Grid_Size_Y"]}')].append(us)
    print("== per kernel (all launches of the run, divided by steps in the last columns)")
    total = 0.0
    for name, v in sorted(by_name.items(), key=lambda kv: -sum(kv[1]))[:28]:
        total += sum(v)
        print(f"{sum(v) / 1e3:9.3f} ms {len(v):6d} calls  avg {sum(v) / len(v):8.1f} us  min {min(v):8.1f} max {max(v):8.1f} | per step {sum(v) / 1e3 / steps:7.3f} ms "
              f"{len(v) / steps:7.1f} calls  {name[:80]}")
    print(f"all kernels: {sum(sum(v) for v in by_name.values()) / 1e3 / steps:.3f} ms per step, {len(rows) / steps:.1f} launches per step")
    print("== by grid size")
    for (name, grid), v in sorted(by_grid.items()):
        if not any(f in name for f in filters):
            continue
        print(f"{name[:62]:62s} grid {grid:>12s} {len(v):6d} calls sum {sum(v) / 1e3:9.3f} ms  per step {sum(v) / 1e3 / steps:7.3f} ms  avg {sum(v) / len(v):8.1f} us "
              f"min {min(v):8.1f} max {max(v):8.1f}")


if __name__ == "__main__":
    main()
