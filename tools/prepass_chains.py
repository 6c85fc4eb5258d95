"""Spatial pre-pass chains in a rocprofv3 --kernel-trace csv of tools/step_trace.py (last step, like tools/trace_gaps.py):
   python tools/prepass_chains.py DIR
A chain is a run of consecutive slic_prep_lane / slic_spatial launches in start order (one batch's pre-pass but its last sweep).  Per
chain: its wall time, the sums of both kernels' durations, the time during which at least one of them ran (union), the idle time and
the time during which two ran at once (a grouped pre-pass: two window groups on two streams)."""
import csv, glob, sys
d = sys.argv[1]
rows = []
for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], int(r["Grid_Size_X"]), int(r["Grid_Size_Y"])))
rows.sort()
zi = [i for i, r in enumerate(rows) if "zonal_finalize" in r[2]]
start = zi[-2] + 1 if len(zi) >= 2 else 0
rows = rows[start:zi[-1] + 1]
chains, cur = [], []
for r in rows:
    if "slic_spatial_kernel" in r[2] or "slic_prep_lane" in r[2]:
        cur.append(r)
    else:
        if sum("slic_spatial" in x[2] for x in cur) >= 2: chains.append(cur)
        cur = []
print("== pre-pass chains of the last step (the centroid step behind a chain's last spatial sweep belongs to the next sweep and is left out)")
tw = tb = ti = 0.0
for c in chains:
    while c and "slic_prep_lane" in c[-1][2]: c = c[:-1]
    t0, t1 = c[0][0], max(x[1] for x in c)
    iv = sorted((x[0], x[1]) for x in c)
    busy, lo, hi = 0, iv[0][0], iv[0][1]
    for a, b in iv[1:]:
        if a > hi: busy += hi - lo; lo, hi = a, b
        else: hi = max(hi, b)
    busy += hi - lo
    sp = [x for x in c if "slic_spatial" in x[2]]; pr = [x for x in c if "slic_prep_lane" in x[2]]
    ssum = sum(x[1] - x[0] for x in sp); psum = sum(x[1] - x[0] for x in pr)
    ov = ssum + psum - busy
    print(f"chain: {len(sp):3d} spatial (first: {sp[0][3] // 256} workgroups) {len(pr):3d} prep | wall {(t1 - t0) / 1e3:8.1f} us  spatial sum {ssum / 1e3:8.1f}  prep sum {psum / 1e3:7.1f}  "
          f"union {busy / 1e3:8.1f}  idle {(t1 - t0 - busy) / 1e3:7.1f}  overlapped {ov / 1e3:7.1f}")
    tw += t1 - t0; tb += busy; ti += t1 - t0 - busy
print(f"all chains: wall {tw / 1e6:.3f} ms, kernels (union) {tb / 1e6:.3f} ms, idle {ti / 1e6:.3f} ms, {len(chains)} chains")
