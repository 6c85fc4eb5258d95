"""Colour-pass chains in a rocprofv3 --kernel-trace csv of tools/step_trace.py (last step, like tools/trace_gaps.py and
tools/prepass_chains.py):
   python tools/sweep_chains.py DIR
A chain is a run of consecutive slic_prep_lane / colour-sweep launches in start order: one batch's colour pass, from the centroid step
in front of its first colour sweep to the end of its last one.  A colour sweep is slic_assign_collb_kernel or slic_assign_kernel with
IGNORE_COLOR = false (the last pre-pass sweep, slic_assign_rawin_kernel or IGNORE_COLOR = true, ends the chain in front).  Per chain:
its wall time, the sums of both kernels' durations, the time during which at least one of them ran (union), the idle time, the time
during which two or more ran at once (a grouped colour pass: two window groups on two streams), and the centroid steps' own
durations."""
import csv, glob, re, sys


def colour_sweep(name):
    if "slic_assign_collb_kernel" in name:
        return True
    m = re.search(r"slic_assign_kernel<([^>]*)>", name)
    if not m:
        return False
    a = [x.strip() for x in m.group(1).split(",")]
    return len(a) >= 3 and a[2] in ("false", "0")


def main():
    d = sys.argv[1]
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], int(r["Grid_Size_X"]), int(r["Grid_Size_Y"])))
    rows.sort()
    zi = [i for i, r in enumerate(rows) if "zonal_finalize" in r[2]]
    start = zi[-2] + 1 if len(zi) >= 2 else 0
    rows = rows[start:zi[-1] + 1] if zi else rows
    chains, cur = [], []
    for r in rows + [(0, 0, "", 0, 0)]:
        if colour_sweep(r[2]) or "slic_prep_lane" in r[2]:
            cur.append(r)
        else:
            if sum(colour_sweep(x[2]) for x in cur) >= 2: chains.append(cur)
            cur = []
    print("== colour-pass chains of the last step")
    tw = tb = ti = t2 = tp = 0.0
    for c in chains:
        while c and "slic_prep_lane" in c[-1][2]: c = c[:-1]
        t0, t1 = c[0][0], max(x[1] for x in c)
        ev = sorted([(x[0], 1) for x in c] + [(x[1], -1) for x in c])
        busy = two = depth = 0
        last = ev[0][0]
        for t, s in ev:
            if depth >= 1: busy += t - last
            if depth >= 2: two += t - last
            depth += s; last = t
        sw = [x for x in c if colour_sweep(x[2])]; pr = [x for x in c if "slic_prep_lane" in x[2]]
        ssum = sum(x[1] - x[0] for x in sw); psum = sum(x[1] - x[0] for x in pr)
        print(f"chain: {len(sw):3d} colour sweeps (first: {sw[0][3] // 256} workgroups, {(sw[0][1] - sw[0][0]) / 1e3:7.1f} us) {len(pr):3d} centroid steps "
              f"(grid {pr[0][3]}x{pr[0][4]}: sum {psum / 1e3:7.1f} us, {psum / 1e3 / len(pr):5.1f} each) | wall {(t1 - t0) / 1e3:8.1f} us  sweep sum {ssum / 1e3:8.1f}  "
              f"union {busy / 1e3:8.1f}  idle {(t1 - t0 - busy) / 1e3:7.1f}  two running {two / 1e3:8.1f}")
        tw += t1 - t0; tb += busy; ti += t1 - t0 - busy; t2 += two; tp += psum
    print(f"all chains: wall {tw / 1e6:.3f} ms, kernels (union) {tb / 1e6:.3f} ms, idle {ti / 1e6:.3f} ms, two running {t2 / 1e6:.3f} ms, "
          f"centroid steps {tp / 1e6:.3f} ms, {len(chains)} chains")


if __name__ == "__main__":
    main()
