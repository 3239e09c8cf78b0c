#!/usr/bin/env python3
"""Where the device waits: from a rocprofv3 --kernel-trace CSV, the idle gaps of every hardware queue and of the device as a whole inside
the timed region of a bench.py run (the seam steps come first, the resident steps after them).
   python3 tools/timeline_gaps.py <kernel_trace.csv> [min_gap_us=150]
Per kernel name, for a mapper-only run: inside the window of the last <steps> steps (<chunks> first-tier launches each) the launches
of every pm_ kernel (n, mean, min, max, total), every queue's busy and idle time, and the idle time in front of each kernel name
on its queue.
   python3 tools/timeline_gaps.py --launches <kernel_trace.csv, or a directory that holds one> [steps=4] [chunks=4]"""
import csv, glob, os, sys, re
from collections import defaultdict


def launches(args):

    if len(args) < 1 or len(args) > 3:
        sys.exit(__doc__)
    fn = args[0]
    if os.path.isdir(fn):
        found = sorted(glob.glob(os.path.join(fn, "**", "*kernel_trace.csv"), recursive=True))
        if len(found) != 1:
            sys.exit("%s: %d kernel-trace CSVs, name one" % (fn, len(found)))
        fn = found[0]
    steps = int(args[1]) if len(args) > 1 else 4
    chunks = int(args[2]) if len(args) > 2 else 4
    ev = []
    for r in csv.DictReader(open(fn)):
        n = re.sub(r"\(.*$", "", re.sub(r"^void ", "", r["Kernel_Name"]))
        if n.startswith("pm_"):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n, r.get("Queue_Id", "?")))
    ev.sort()
    first = [e for e in ev if re.match(r"pm_seed4_kernel<\d+, 0>", e[2])]
    if len(first) < steps * chunks:
        sys.exit("%s: %d first-tier launches, fewer than %d steps of %d chunks" % (fn, len(first), steps, chunks))
    t0 = first[-steps * chunks][0]
    ev = [e for e in ev if e[0] >= t0]
    t1 = max(e[1] for e in ev)
    print("window %.2f ms, %d steps" % ((t1 - t0) / 1e6, steps))
    perk = defaultdict(list)
    for s, e, n, q in ev:
        perk[n].append((e - s) / 1e3)
    for n, v in sorted(perk.items(), key=lambda kv: -sum(kv[1])):
        print("  %-40s n %4d avg %9.1f min %9.1f max %9.1f us total %8.2f ms" % (n[:40], len(v), sum(v) / len(v), min(v), max(v), sum(v) / 1e3))
    perq = defaultdict(list)
    for e in ev:
        perq[e[3]].append(e)
    for q, v in sorted(perq.items()):
        busy, idle, end = 0, 0, v[0][0]
        front = defaultdict(list)
        for s, e, n, _ in v:
            if s > end:
                idle += s - end
                front[n].append((s - end) / 1e3)
            busy += max(e, end) - max(s, end)
            end = max(end, e)
        names = defaultdict(int)
        for _, _, n, _ in v:
            names[n.split("<")[0]] += 1
        print("queue %s: n %d busy %.2f ms idle %.2f ms  %s" % (q, len(v), busy / 1e6, idle / 1e6, dict(names)))
        for n, g in sorted(front.items(), key=lambda kv: -sum(kv[1])):
            if sum(g) >= 50.0:
                print("    idle in front of %s: n %d mean %.1f us min %.1f max %.1f  sum %.2f ms" % (n, len(g), sum(g) / len(g), min(g), max(g), sum(g) / 1e3))


if len(sys.argv) > 1 and sys.argv[1] == "--launches":
    launches(sys.argv[2:])
    sys.exit(0)
rows = []
for r in csv.DictReader(open(sys.argv[1])):
    n = re.sub(r"^void ", "", r["Kernel_Name"]); n = re.sub(r"[<(].*$", "", n)
    if n.startswith("pm_"):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n, r.get("Queue_Id", "?")))
rows.sort()
min_gap = float(sys.argv[2]) * 1e3 if len(sys.argv) > 2 else 150e3
# phases: separated by device-wide gaps of more than 20 ms (index build / synth / sync between the seam and the resident run)
phases, cur, end = [], [rows[0]], rows[0][1]
for r in rows[1:]:
    if r[0] - end > 20e6:
        phases.append(cur); cur = []
    cur.append(r); end = max(end, r[1])
phases.append(cur)
for pi, ph in enumerate(phases):
    t0, t1 = ph[0][0], max(r[1] for r in ph)
    n_seed = sum(1 for r in ph if r[2].startswith("pm_seed4"))
    if n_seed < 8:
        continue
    print("== phase %d: %.1f ms, %d kernels, %d pm_seed4 launches" % (pi, (t1 - t0) / 1e6, len(ph), n_seed))
    # device-wide idle
    idle, e = 0, ph[0][1]
    for r in ph[1:]:
        if r[0] > e:
            idle += r[0] - e
        e = max(e, r[1])
    print("   device idle (no pm_ kernel running): %.2f ms" % (idle / 1e6))
    # the seed kernel's own stream: gaps between consecutive pm_seed4 launches
    seeds = [r for r in ph if r[2].startswith("pm_seed4")]
    busy = sum(r[1] - r[0] for r in seeds)
    gaps = [(b[0] - a[1], a[1] - t0) for a, b in zip(seeds, seeds[1:])]
    print("   pm_seed4: busy %.2f ms (avg %.3f), sum of gaps between launches %.2f ms, largest gaps (ms at ms): %s" % (
        busy / 1e6, busy / len(seeds) / 1e6, sum(g for g, _ in gaps) / 1e6,
        ", ".join("%.2f@%.1f" % (g / 1e6, at / 1e6) for g, at in sorted(gaps, reverse=True)[:8])))
    byq = {}
    for r in ph:
        byq.setdefault(r[3], []).append(r)
    for q, rs in sorted(byq.items()):
        b = sum(r[1] - r[0] for r in rs)
        names = {}
        for r in rs:
            names[r[2]] = names.get(r[2], 0) + (r[1] - r[0])
        top = sorted(names.items(), key=lambda kv: -kv[1])[:4]
        print("   queue %s: %d kernels, busy %.2f ms: %s" % (q, len(rs), b / 1e6, ", ".join("%s %.1f" % (k, v / 1e6) for k, v in top)))
