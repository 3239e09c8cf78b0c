#!/usr/bin/env python3
"""What the device-made rows of <outfile>.base.gz cost (pecall_dev_sites_base_text, PECALLER_DEVICE_ROWS=1): both measurements in one
visit to the device.

  python3 tools/pecall_rows_time.py [--columns-log2 20] [--gen-log2 16] [--reps 5] [--cli-columns 1000000] [--cli-reps 3]
                                    [--parent-exe PATH] [--skip-kernels] [--skip-cli]
      (a) the three kernels (length, scan, fill: HIP events of the library) on 2^20 columns x 64 and x 256 samples of bench.py's
          config-4 generator (2^gen-log2 generated columns laid down side by side; the calls come from pecall_dev_call_sites_sparse);
          medians of `reps` runs after one warm-up; the bytes each has to move over its time as a share of the 6.3 TB/s a streaming
          kernel reaches on this part; and the whole entry's wall clock into a page-locked text buffer
      (b) pecaller_hip on the files of tools/pecaller_cli_throughput.py (1 M columns x 64 samples, written once) in four
          configurations, `cli-reps` times each in turn after a warm-up round: the parent commit's binary (--parent-exe: a build of
          the parent commit; left out when not given), this build with the switch off, with PECALLER_DEVICE_ROWS=1, and with
          PECALLER_DEVICE_MERGE=1 as well; the program's own split (merge / device / text) from its closing line"""
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


def kernels(a, S):
    from pecaller_amd.pecall import PecallDev
    n, g = 1 << a.columns_log2, 1 << min(a.gen_log2, a.columns_log2)
    reads, dom = bench.pecall_columns(g, S)
    reads, dom = np.tile(reads, (n // g, 1, 1)), np.tile(dom, n // g)
    names = ["chr1", "chr12_KI270904v1_altern"]
    contig = ((np.arange(n) >> 12) & 1).astype(np.int32)
    pos = (np.arange(n, dtype=np.uint32) + 1000)
    ref = np.frombuffer(b"ACGT", np.uint8)[dom]
    pc = PecallDev(0)
    t0 = time.time()
    _, (site, _), typ, _, _ = pc.call_sites_sparse(reads, dom)
    t_call = time.time() - t0
    ms, wall = [], []
    for k in range(a.reps + 1):
        t0 = time.time()
        text, hole_site, hole_at = pc.base_text(names, contig, pos, ref, pin=True)
        wall.append((time.time() - t0) * 1e3)
        ms.append(pc.rows_ms.copy())
    assert np.array_equal(hole_site, site)
    ms = np.median(np.array(ms[1:]), axis=0)
    n_rows, T = int((typ >= 0).sum()) - len(site), len(text)
    pad = (n + 1024) // 1024 * 1024
    # what has to move: the length kernel reads the posteriors of every column the caller did not skip, the type, the contig and the
    # position, and writes a word; the scan reads the words twice and writes an offset per column and 12 bytes per hole; the fill
    # kernel reads the calls, the words, the offsets and the heads of the rows it makes, and writes the text
    b_len = 8 * S * int((typ >= 0).sum()) + 13 * n
    b_scan = 8 * pad + 8 * pad + 12 * len(site)
    b_fill = S * n_rows + 21 * n + T
    print("rows: %d columns x %d samples (call_sites_sparse %.2f s): %d rows from the device, %d holes, %.1f MB of text" % (n, S, t_call, n_rows, len(site), T / 1e6))
    for name, t, b in (("length", ms[0], b_len), ("scan", ms[1], b_scan), ("fill", ms[2], b_fill), ("three kernels", float(ms.sum()), b_len + b_scan + b_fill)):
        print("  %-14s %8.3f ms  %8.1f MB  %6.2f TB/s = %4.1f %% of %.1f TB/s" % (name, t, b / 1e6, b / (t * 1e-3) / 1e12, 100.0 * b / (t * 1e-3) / 1e12 / HBM_TBS, HBM_TBS))
    print("  base_text through the Python wrapper (a page-locked buffer made and released per call, the text copied out of it): median %.1f ms" % float(np.median(wall[1:])))
    pc.close()


def cli(a):
    n, S, REP = a.cli_columns, 64, 16
    OFF = 1000
    g = n // REP
    reads, dom = bench.pecall_columns(g, S)
    genome = np.full(OFF + g * REP + 1000, ord("A"), np.uint8)
    genome[OFF:OFF + g * REP] = np.tile(np.frombuffer(b"ACGT", np.uint8)[dom], REP)
    W = tempfile.mkdtemp()
    open(os.path.join(W, "g1.sdx"), "w").write("1\n%d\tchr1\n" % len(genome))
    gzip.open(os.path.join(W, "g1.seq"), "wb", compresslevel=1).write(genome.tobytes() + b"N" * 15)
    run = os.path.join(W, "run")
    os.mkdir(run)
    for s in range(S):
        r = np.zeros(g, REC)
        r["c"] = reads[:, s, :]
        keep = r["c"].sum(axis=1) > 0
        with open(os.path.join(run, "s%03d.pileup.gz" % s), "wb") as f:
            for k in range(REP):
                r["pos"] = np.arange(g, dtype=np.uint32) + OFF + k * g
                f.write(gzip.compress(r[keep].tobytes(), compresslevel=1))
    here = os.path.join(ROOT, "pecaller_amd", "pecaller_hip")
    configs = [("this build, switches off", here, {}), ("this build, PECALLER_DEVICE_ROWS=1", here, {"PECALLER_DEVICE_ROWS": "1"}),
               ("this build, PECALLER_DEVICE_ROWS=1 PECALLER_DEVICE_MERGE=1", here, {"PECALLER_DEVICE_ROWS": "1", "PECALLER_DEVICE_MERGE": "1"})]
    if a.parent_exe:
        configs.insert(0, ("parent commit's binary", os.path.abspath(a.parent_exe), {}))
    pat = re.compile(r"in ([\d.]+) s \(([\d.]+) M columns/s; stream merge ([\d.]+) s \+ ([\d.]+) s waiting.*device calls ([\d.]+) s, rows and gz ([\d.]+) s")
    figs, sums = {}, {}
    for rep in range(a.cli_reps + 1):           # (the first round warms the page cache and the driver: not counted)
        for name, exe, extra in configs:
            env = dict(os.environ)
            for k in ("PECALLER_DEVICE_ROWS", "PECALLER_DEVICE_MERGE"):
                env.pop(k, None)
            env.update(extra)
            out = subprocess.run([exe, "pileup", os.path.join(W, "g1.sdx"), str(S), "out", "0.95", "0.001", "n", "24", "n"], cwd=run, stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, env=env, timeout=300)
            txt = out.stdout.decode(errors="replace")
            assert out.returncode == 0, txt[-2000:]
            lines = [l.strip() for l in txt.splitlines() if "pecaller_hip:" in l]
            print("[round %d] %s\n    %s" % (rep, name, "\n    ".join(lines)), flush=True)
            # (every configuration writes the same four files)
            sums.setdefault(name, set()).add(tuple(hash(gzip.open(os.path.join(run, f), "rb").read() if f.endswith(".gz") else open(os.path.join(run, f), "rb").read())
                                                   for f in ("out.base.gz", "out.snp", "out.piles.gz", "out.dist")))
            m = pat.search(txt)
            if rep and m:
                figs.setdefault(name, []).append([float(x) for x in m.groups()])
    assert len(set.union(*sums.values())) == 1, "the configurations wrote different files"
    print("medians of %d runs (all configurations wrote the same files): wall s, M columns/s, stream merge s, waiting s, device calls s, rows and gz s" % a.cli_reps)
    for name, v in figs.items():
        print("  %-60s %s" % (name + ":", " ".join("%.3f" % x for x in np.median(np.array(v), axis=0))))
    shutil.rmtree(W)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns-log2", type=int, default=20)
    ap.add_argument("--gen-log2", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli-columns", type=int, default=1000000)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--parent-exe")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-cli", action="store_true")
    a = ap.parse_args()
    if not a.skip_kernels:
        for S in (64, 256):
            kernels(a, S)
    if not a.skip_cli:
        cli(a)
