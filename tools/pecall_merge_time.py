#!/usr/bin/env python3
"""What the device merge of the pileup streams costs (pecall_dev_sites_stage_records, PECALLER_DEVICE_MERGE=1).

  python3 tools/pecall_merge_time.py [--samples 64] [--span-log2 20] [--reps 7]
      (a) the merge kernels (mark, scan, tile: HIP events of the library, pecall_dev_sites_merge_ms) on the records of bench.py's
          config-4 generator -- a record for nearly every (slot, sample) -- next to pecall_dev_sites_run's kernel_ms on the columns
          they made; medians of `reps` runs after two warm-up runs; the bytes the kernels have to move over their time as a share
          of the 6.3 TB/s a streaming kernel reaches on this part
  python3 tools/pecall_merge_time.py --guided [--samples 64] [--span-log2 20] [--reps 7]
      (a) for one guided range (pecall_dev_sites_stage_records_guided): the same records, the columns at the positions of exome-like
          intervals (100 to 400 positions, about 2 % of the range); mark = the marks from the intervals and the records' check
  python3 tools/pecall_merge_time.py --cli [--columns 1000000] [--samples 64] [--reps 3] [--exe PATH ...]
      (b) pecaller_hip on the files of tools/pecaller_cli_throughput.py, written once: every executable given (default: this tree's;
          name a build of the parent commit as well to compare) with the switch off and on, `reps` times each in turn; the program's
          closing line of every run and the medians of its figures"""
import argparse
import gzip
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bench

HBM_TBS = 6.3
REC = np.dtype([("pos", "<u4"), ("c", "<u2", 6)])


def kernels(a):
    from pecaller_amd.pecall import PecallDev
    S, span = a.samples, 1 << a.span_log2
    reads, dom = bench.pecall_columns(span, S)
    p0 = 1000
    recs = []
    for s in range(S):
        r = np.zeros(span, REC)
        r["pos"] = np.arange(span, dtype=np.uint32) + p0
        r["c"] = reads[:, s, :]
        recs.append(r[r["c"].sum(axis=1) > 0])
    n_rec = sum(len(r) for r in recs)
    letters = np.frombuffer(b"ACGT", np.uint8)[dom].tobytes()
    pc = PecallDev(0)
    for r in recs:
        pc.pin_host(r)
    ms, wall = [], []
    if a.guided:
        rng = np.random.default_rng(7)
        first, count, at = [], [], 0
        while True:
            at += int(rng.integers(6250, 18251))
            ln = int(rng.integers(100, 401))
            if at + ln > span:
                break
            first.append(at)
            count.append(ln)
            at += ln
        first, count = np.array(first, np.uint32), np.array(count, np.uint32)
    for k in range(a.reps + 2):
        t0 = time.time()
        if a.guided:
            n_cols, _ = pc.sites_stage_records_guided(recs, p0, span, letters, first, count)
        else:
            n_cols, _ = pc.sites_stage_records(recs, p0, span, letters)
        wall.append((time.time() - t0) * 1e3)
        ms.append(pc.sites_merge_ms().copy())
    ms = np.median(np.array(ms[2:]), axis=0)
    if a.guided:
        # the columns are the intervals' positions; what the kernels move: the marks and chromosome bytes written, the records read for
        # the check, the marks scanned, and the tile kernel's runs that hold a marked slot
        slots = np.concatenate([np.arange(f, f + c) for f, c in zip(first, count)])
        got = pc.sites_gather(np.arange(0, n_cols, max(1, n_cols // 1000), dtype=np.uint32))[0]
        assert n_cols == len(slots) and np.array_equal(got, reads[slots[::max(1, n_cols // 1000)]])
        print("guided range: %d samples x %d slots, %d records, %d intervals, %d columns (%.2f %% of the slots)" %
              (S, span, n_rec, len(first), n_cols, 100.0 * n_cols / span))
        print("  mark (intervals + check) %.3f ms, scan %.3f ms, tile %.3f ms; merge kernels %.3f ms" % (ms[0], ms[1], ms[2], float(ms.sum())))
        print("  pecall_dev_sites_stage_records_guided, host wall with the upload from pinned arrays and its two waits: median %.2f ms" % float(np.median(wall[2:])))
        pc.close()
        return
    run = [pc.sites_run() for _ in range(a.reps + 2)][2:]
    # the columns the records made are the generator's columns
    got = pc.sites_gather(np.arange(0, n_cols, max(1, n_cols // 1000), dtype=np.uint32))[0]
    keep = np.flatnonzero(reads.reshape(span, -1).sum(axis=1) > 0)
    assert n_cols == len(keep) and np.array_equal(got, reads[keep[::max(1, n_cols // 1000)]])
    # what has to move: mark reads the records' lines and writes the marks; the scan reads the marks twice and writes two words and two
    # bytes per column; the tile kernel reads the records and writes the columns' rows
    b_mark, b_scan, b_tile = 16 * n_rec + span, 2 * span + 10 * n_cols + span, 16 * n_rec + 12 * S * n_cols + 5 * span
    tot = float(ms.sum())
    print("records: %d samples x %d slots, %d records (%.1f %% of the slots), %d columns" % (S, span, n_rec, 100.0 * n_rec / (S * span), n_cols))
    for name, t, b in (("mark", ms[0], b_mark), ("scan", ms[1], b_scan), ("tile", ms[2], b_tile), ("merge kernels", tot, b_mark + b_scan + b_tile)):
        print("  %-14s %8.3f ms  %8.1f MB  %6.2f TB/s = %4.1f %% of %.1f TB/s" % (name, t, b / 1e6, b / (t * 1e-3) / 1e12, 100.0 * b / (t * 1e-3) / 1e12 / HBM_TBS, HBM_TBS))
    print("  pecall_dev_sites_run kernel_ms on the same columns: median %.3f ms (%s); merge kernels / caller kernels = %.2f" %
          (float(np.median(run)), " ".join("%.2f" % x for x in run), tot / float(np.median(run))))
    print("  pecall_dev_sites_stage_records, host wall with the upload from pinned arrays and its two waits: median %.2f ms (%.0f M columns/s)" %
          (float(np.median(wall[2:])), n_cols / np.median(wall[2:]) / 1e3))
    pc.close()


def cli(a):
    n, S = a.columns, a.samples
    OFF = 1000
    reads, dom = bench.pecall_columns(n, S)
    genome = np.full(OFF + n + 1000, ord("A"), np.uint8)
    genome[OFF:OFF + n] = np.frombuffer(b"ACGT", np.uint8)[dom]
    W = tempfile.mkdtemp()
    open(os.path.join(W, "g1.sdx"), "w").write("1\n%d\tchr1\n" % len(genome))
    gzip.open(os.path.join(W, "g1.seq"), "wb", compresslevel=1).write(genome.tobytes() + b"N" * 15)
    run = os.path.join(W, "run")
    os.mkdir(run)
    for s in range(S):
        r = np.zeros(n, REC)
        r["pos"] = np.arange(n, dtype=np.uint32) + OFF
        r["c"] = reads[:, s, :]
        with open(os.path.join(run, "s%03d.pileup.gz" % s), "wb") as f:
            f.write(gzip.compress(r[r["c"].sum(axis=1) > 0].tobytes(), compresslevel=1))
    exes = a.exe or [os.path.join(ROOT, "pecaller_amd", "pecaller_hip")]
    pat = re.compile(r"in ([\d.]+) s \(([\d.]+) M columns/s; stream merge ([\d.]+) s \+ ([\d.]+) s waiting.*device calls ([\d.]+) s, rows and gz ([\d.]+) s")
    figs = {}
    for rep in range(a.reps + 1):               # (the first round warms the page cache and the driver: not counted)
        for exe in exes:
            for switch in ("0", "1"):
                env = dict(os.environ, PECALLER_DEVICE_MERGE=switch)
                out = subprocess.run([exe, "pileup", os.path.join(W, "g1.sdx"), str(S), "out", "0.95", "0.001", "n", "24", "n"], cwd=run, stdout=subprocess.PIPE,
                                     stderr=subprocess.STDOUT, env=env, timeout=300)
                txt = out.stdout.decode(errors="replace")
                assert out.returncode == 0, txt[-2000:]
                m = pat.search(txt)
                lines = [l.strip() for l in txt.splitlines() if "pecaller_hip:" in l]
                print("[round %d] %s PECALLER_DEVICE_MERGE=%s\n    %s" % (rep, exe, switch, "\n    ".join(lines)), flush=True)
                if rep and m:
                    figs.setdefault((exe, switch), []).append([float(x) for x in m.groups()])
    print("medians of %d runs: wall s, M columns/s, stream merge s, waiting s, device calls s, rows and gz s" % a.reps)
    for (exe, switch), v in figs.items():
        print("  %s switch %s: %s" % (exe, switch, " ".join("%.3f" % x for x in np.median(np.array(v), axis=0))))
    shutil.rmtree(W)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--guided", action="store_true")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--span-log2", type=int, default=20)
    ap.add_argument("--columns", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--exe", action="append")
    a = ap.parse_args()
    if a.reps is None:
        a.reps = 3 if a.cli else 7
    (cli if a.cli else kernels)(a)
