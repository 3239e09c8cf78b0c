#!/usr/bin/env python3
"""What deflating the device-made rows of <outfile>.base.gz on the device costs and what it saves (pecall_dev_sites_base_gz,
PECALLER_DEVICE_GZ=1 on top of PECALLER_DEVICE_ROWS=1): both measurements in one visit to the device.

  python3 tools/pecall_gz_time.py [--columns-log2 20] [--gen-log2 16] [--reps 5] [--cli-columns 1000000,8000000] [--cli-reps 3]
                                  [--threads 16] [--parent-exe PATH] [--skip-kernels] [--skip-cli]
      (a) on 2^20 columns x 64 samples of bench.py's config-4 generator (2^gen-log2 generated columns laid down side by side; the
          calls come from pecall_dev_call_sites_sparse): the HIP-event times of the library -- length, scan, fill (the three text
          kernels), deflate (runs, scan, piece table, the deflate kernel), pack (scan, pack, holes) -- next to the caller's, medians
          of `reps` runs after one warm-up; the whole entry's wall clock into a page-locked buffer next to base_text's; and the
          members' size next to zlib.compress(text, 2) and zlib.compress(text, 6) of the same text, with what those cost a core
      (b) pecaller_hip on files written as tools/pecaller_cli_throughput.py writes them, for each of `cli-columns` x 64 samples, in
          four configurations, `cli-reps` times each in turn after a warm-up round: the parent commit's binary (--parent-exe: a
          build of the parent commit; left out when not given), this build with the switches off, with PECALLER_DEVICE_ROWS=1, and
          with PECALLER_DEVICE_GZ=1 as well; medians of the program's closing line, the size of out.base.gz, and the hashes of the
          four files (inflated where gzip), which must agree between the configurations"""
import argparse
import gzip
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bench

REC = np.dtype([("pos", "<u4"), ("c", "<u2", 6)])
FILES = ("out.base.gz", "out.snp", "out.piles.gz", "out.dist")


def kernels(a, S):
    from pecaller_amd.pecall import PecallDev, PCG_PIECE
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
    ms, wall_gz, wall_text = [], [], []
    for k in range(a.reps + 1):
        t0 = time.time()
        text, hole_site, hole_at = pc.base_text(names, contig, pos, ref, pin=True)
        wall_text.append((time.time() - t0) * 1e3)
        t0 = time.time()
        gz, gz_site, gz_at = pc.base_gz(names, contig, pos, ref, pin=True)
        wall_gz.append((time.time() - t0) * 1e3)
        ms.append(pc.gz_ms.copy())
    assert np.array_equal(gz_site, site) and np.array_equal(hole_site, site)
    assert gzip.decompress(gz) == text, "the members do not inflate to the text"
    ms = np.median(np.array(ms[1:]), axis=0)
    T = len(text)
    print("gz: %d columns x %d samples (call_sites_sparse %.2f s): %d holes, %.1f MB of text, pieces of %d bytes" % (n, S, t_call, len(site), T / 1e6, PCG_PIECE))
    for name, t in zip(("length", "scan", "fill", "deflate", "pack"), ms):
        print("  %-14s %8.3f ms" % (name, t))
    print("  %-14s %8.3f ms   the two new stages %8.3f ms = %.1f GB/s of text" % ("three text kernels", float(ms[:3].sum()), float(ms[3:].sum()), T / float(ms[3:].sum()) / 1e6))
    print("  through the Python wrapper (a page-locked buffer made and released per call, the bytes copied out of it): base_text median %.1f ms, base_gz median %.1f ms"
          % (float(np.median(wall_text[1:])), float(np.median(wall_gz[1:]))))
    print("  size: the device's members %.2f MB (%.1f : 1)" % (len(gz) / 1e6, T / max(len(gz), 1)))
    for level in (2, 6):
        t0 = time.time()
        z = zlib.compress(text, level)
        dt = time.time() - t0
        print("        zlib.compress(text, %d) %.2f MB (%.1f : 1; the members are %.2f times that), %.2f s of one core" % (level, len(z) / 1e6, T / len(z), len(gz) / len(z), dt))
    pc.close()


def digest(path):
    h = hashlib.sha1()
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        for block in iter(lambda: f.read(64 << 20), b""):
            h.update(block)
    return h.hexdigest()[:16]


def cli(a, n):
    S, OFF = 64, 1000
    REP = max(16, n // 62500)
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
               ("this build, PECALLER_DEVICE_ROWS=1 PECALLER_DEVICE_GZ=1", here, {"PECALLER_DEVICE_ROWS": "1", "PECALLER_DEVICE_GZ": "1"})]
    if a.parent_exe:
        configs.insert(0, ("parent commit's binary", os.path.abspath(a.parent_exe), {}))
    pat = re.compile(r"in ([\d.]+) s \(([\d.]+) M columns/s; stream merge ([\d.]+) s \+ ([\d.]+) s waiting.*device calls ([\d.]+) s, rows and gz ([\d.]+) s")
    figs, sums, size = {}, {}, {}
    print("pecaller_hip: %d columns x %d samples, %d threads" % (g * REP, S, a.threads))
    for rep in range(a.cli_reps + 1):           # (the first round warms the page cache and the driver: not counted; it is the one hashed)
        for name, exe, extra in configs:
            env = {k: v for k, v in os.environ.items() if not k.startswith("PECALLER_DEVICE_")}
            env.update(extra)
            out = subprocess.run([exe, "pileup", os.path.join(W, "g1.sdx"), str(S), "out", "0.95", "0.001", "n", str(a.threads), "n"], cwd=run, stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, env=env, timeout=600)
            txt = out.stdout.decode(errors="replace")
            assert out.returncode == 0, txt[-2000:]
            lines = [l.strip() for l in txt.splitlines() if "pecaller_hip:" in l]
            print("[round %d] %s\n    %s" % (rep, name, "\n    ".join(lines)), flush=True)
            size[name] = os.path.getsize(os.path.join(run, "out.base.gz"))
            if rep == 0:
                sums[name] = tuple(digest(os.path.join(run, f)) for f in FILES)
                print("    hashes (inflated where gzip): %s" % " ".join(sums[name]), flush=True)
            m = pat.search(txt)
            if rep and m:
                figs.setdefault(name, []).append([float(x) for x in m.groups()])
    assert len(set(sums.values())) == 1, "the configurations wrote different files"
    print("medians of %d runs (all configurations wrote the same files): wall s, M columns/s, stream merge s, waiting s, device calls s, rows and gz s; bytes of out.base.gz" % a.cli_reps)
    for name, v in figs.items():
        print("  %-60s %s  %d" % (name + ":", " ".join("%.3f" % x for x in np.median(np.array(v), axis=0)), size[name]))
    shutil.rmtree(W)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns-log2", type=int, default=20)
    ap.add_argument("--gen-log2", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli-columns", default="1000000,8000000")
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-exe")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-cli", action="store_true")
    a = ap.parse_args()
    if not a.skip_kernels:
        kernels(a, 64)
    if not a.skip_cli:
        for n in a.cli_columns.split(","):
            cli(a, int(n))
