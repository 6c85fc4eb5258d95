"""Small commands per tile batch in a rocprofv3 --kernel-trace csv of tools/step_trace.py or bench.py: for the LAST step (as
tools/trace_gaps.py cuts it) the step is split into its batches -- a batch starts at its tile_mask_kernel launch, what precedes the
first one is the step's head -- and per batch the fills (fillBuffer blits and clear_ranges_kernel), the copies (copyBuffer blits),
the other kernels, and the idle time are listed, with the idle time in front of small commands apart from the idle time in front of
other kernels.  Then: the kernels that follow a gap, by name (which command the GPU was waiting for).
   python tools/batch_commands.py DIR"""
import collections, csv, glob, sys


def kind(name):
    if "fillBuffer" in name or "clear_ranges" in name:
        return "fill"
    if "copyBuffer" in name:
        return "copy"
    return "kernel"


def main():
    rows = []
    for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    zi = [i for i, r in enumerate(rows) if "zonal_finalize" in r[2]]
    rows = rows[(zi[-2] + 1 if len(zi) >= 2 else 0):zi[-1] + 1]
    batches, cur = [], []
    for r in rows:
        if "tile_mask_kernel" in r[2] and cur:
            batches.append(cur); cur = []
        cur.append(r)
    batches.append(cur)
    after_gap = collections.Counter(); after_gap_n = collections.Counter()
    prev_end = rows[0][0]
    tot = collections.Counter()
    print("batch  fills copies kernels | busy: fills  copies (ms) | idle: before small cmds, before kernels (ms) | wall ms")
    for bi, b in enumerate(batches):
        n = collections.Counter(); busy = collections.Counter(); idle = collections.Counter()
        for s, e, name in b:
            k = kind(name)
            n[k] += 1; busy[k] += e - s
            if s > prev_end:
                idle["small" if k != "kernel" else "kernel"] += s - prev_end
                key = name.split("(")[0].replace("void ", "")[:56]
                after_gap[key] += s - prev_end; after_gap_n[key] += 1
            prev_end = max(prev_end, e)
        wall = (max(e for _, e, _ in b) - b[0][0]) / 1e6
        print(f"{bi:5d} {n['fill']:6d} {n['copy']:6d} {n['kernel']:7d} | {busy['fill'] / 1e6:11.3f} {busy['copy'] / 1e6:7.3f}      | "
              f"{idle['small'] / 1e6:10.3f} {idle['kernel'] / 1e6:10.3f}                   | {wall:7.3f}")
        for k in ("fill", "copy", "kernel"):
            tot["n_" + k] += n[k]; tot["busy_" + k] += busy[k]
        tot["idle_small"] += idle["small"]; tot["idle_kernel"] += idle["kernel"]
    print(f"step: {tot['n_fill']} fills {tot['busy_fill'] / 1e6:.3f} ms busy, {tot['n_copy']} copies {tot['busy_copy'] / 1e6:.3f} ms busy, "
          f"{tot['n_kernel']} other kernels; idle {(tot['idle_small'] + tot['idle_kernel']) / 1e6:.3f} ms "
          f"({tot['idle_small'] / 1e6:.3f} before small commands, {tot['idle_kernel'] / 1e6:.3f} before kernels); "
          f"wall {(rows[-1][1] - rows[0][0]) / 1e6:.3f} ms, {len(rows)} launches")
    print("idle by the command that follows the gap:")
    for k, v in after_gap.most_common(16):
        print(f"{v / 1e6:8.3f} ms in {after_gap_n[k]:4d} gaps, {v / 1e3 / after_gap_n[k]:7.1f} us each  {k}")


if __name__ == "__main__":
    main()
