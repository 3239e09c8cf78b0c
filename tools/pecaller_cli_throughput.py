#!/usr/bin/env python3
"""wall clock of the host program pecaller_hip on N pileup columns x S samples of bench.py's config-4 generator (30x Poisson, 0.4 %
error, 1 variant per kb), on a genome of its own (the generator's reference bases), the generated columns laid down `repeats` times:  python3 tools/pecaller_cli_throughput.py [columns=1000000] [samples=64] [repeats=1]
(the program prints its own split: merge + device + text)

  --guide            an exome-like BED guide file over the streams: intervals of 100 to 400 positions that cover about 2 % of the range.
                     Every executable is run with it, switch unset; the last one with PECALLER_DEVICE_GUIDE=1 as well
  --exe PATH ...     the executables to run in turn on the same files (default: this tree's; name a build of the parent commit first
                     to compare)
  --reps N           with N > 1: one round to warm up, then N timed rounds; every run's closing lines and the medians of the wall times"""
import argparse, gzip, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bench, refio
ap = argparse.ArgumentParser()
ap.add_argument("columns", nargs="?", type=int, default=1000000)
ap.add_argument("samples", nargs="?", type=int, default=64)
ap.add_argument("repeats", nargs="?", type=int, default=1)
ap.add_argument("--guide", action="store_true")
ap.add_argument("--exe", action="append")
ap.add_argument("--reps", type=int, default=1)
opt = ap.parse_args()
n, S = opt.columns, opt.samples
REP = opt.repeats        # the generated columns laid down REP times, one after the other
OFF = 1000              # (position 0 means 'stream ended' to the merge, pecaller.c:891-907)
reads, dom = bench.pecall_columns(n, S)              # [n][S][6] u16; dom = reference base code of the generator
# a genome of its own: the letter at every column is the generator's reference base
genome = np.full(OFF + n * REP + 1000, ord("A"), np.uint8)
genome[OFF:OFF + n * REP] = np.tile(np.frombuffer(b"ACGT", np.uint8)[dom], REP)
W = tempfile.mkdtemp()
open(os.path.join(W, "g1.sdx"), "w").write("1\n%d\tchr1\n" % len(genome))
gzip.open(os.path.join(W, "g1.seq"), "wb", compresslevel=1).write(genome.tobytes() + b"N" * 15)
run = os.path.join(W, "run")
os.mkdir(run)
rec = np.dtype([("pos", "<u4"), ("c", "<u2", 6)])


def write_sample(s):
    a = np.zeros(n, rec)
    a["c"] = reads[:, s, :]
    keep = a["c"].sum(axis=1) > 0
    with open(os.path.join(run, "s%03d.pileup.gz" % s), "wb") as f:
        for k in range(REP):
            a["pos"] = np.arange(n, dtype=np.uint32) + OFF + k * n
            f.write(gzip.compress(a[keep].tobytes(), compresslevel=1))      # (gz members concatenate)


import multiprocessing
with multiprocessing.get_context("fork").Pool(min(16, os.cpu_count() or 1)) as pool:
    pool.map(write_sample, range(S))
n = n * REP
guide = []
if opt.guide:
    # intervals of 100 to 400 positions (250 on average) a gap apart that makes them 2 % of the range
    rng = np.random.default_rng(7)
    p, n_guided = OFF + 1, 0
    with open(os.path.join(W, "guide.bed"), "w") as f:
        while True:
            p += int(rng.integers(6250, 18251))
            ln = int(rng.integers(100, 401))
            if p + ln > OFF + n:
                break
            f.write("chr1\t%d\t%d\n" % (p, p + ln - 1))
            n_guided += ln
            p += ln
    guide = [os.path.join(W, "guide.bed")]
    print("guide file: %d positions of %d (%.2f %%)" % (n_guided, n, 100.0 * n_guided / n))
    n = n_guided
exes = opt.exe or [os.path.join(ROOT, "pecaller_amd", "pecaller_hip")]
configs = [(exe, {}) for exe in exes] + ([(exes[-1], {"PECALLER_DEVICE_GUIDE": "1"})] if opt.guide else [])
walls = {}
for rnd in range(opt.reps + (1 if opt.reps > 1 else 0)):          # (with several rounds the first warms the page cache and the driver: not counted)
    for exe, env in configs:
        t0 = time.time()
        out = subprocess.run([exe, "pileup", os.path.join(W, "g1.sdx"), str(S), "out", "0.95", "0.001", "n", "24", "n"] + guide,
                             cwd=run, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, **env))
        dt = time.time() - t0
        txt = out.stdout.decode(errors="replace")
        if len(configs) > 1 or opt.reps > 1:
            print("[round %d] %s %s" % (rnd, exe, " ".join("%s=%s" % kv for kv in env.items())))
        for l in txt.splitlines():
            if "pecaller_hip:" in l:
                print(l.strip())
        assert out.returncode == 0, txt[-2000:]
        print("%d columns x %d samples: wall %.2f s = %.3f M columns/s end to end; out.base.gz %d MB, out.snp %d rows" %
              (n, S, dt, n / dt / 1e6, os.path.getsize(os.path.join(run, "out.base.gz")) >> 20, sum(1 for _ in open(os.path.join(run, "out.snp")))), flush=True)
        if opt.reps == 1 or rnd > 0:
            walls.setdefault((exe, tuple(env.items())), []).append(dt)
if opt.reps > 1:
    print("medians of %d runs, wall s:" % opt.reps)
    for (exe, env), v in walls.items():
        print("  %s %s: %.3f s = %.3f M columns/s" % (exe, " ".join("%s=%s" % kv for kv in env), float(np.median(v)), n / float(np.median(v)) / 1e6))
shutil.rmtree(W)
