#!/usr/bin/env python3
"""What deflating the pileup records on the device costs and what the file weighs (pemap_dev_fetch_records_gz,
PEMAPPER_DEVICE_GZ=1), in one visit to the device.

  python3 tools/pileup_gz_time.py [--genome-log2 26] [--depths 1,5,30,100] [--reps 5] [--sample-mb 64] [--copies 100]
                                  [--skip-cli] [--parent-exe PATH]
      (a) on a synthetic genome of 2^genome-log2 positions (bench.py's generator), after mapping synthetic 2 x 150 pairs up to each
          depth: the four HIP-event times of pemap_dev_fetch_gz_ms for the whole stretch (records, insertion list, deflate, scan +
          pack), medians of `reps` calls after a warm-up, the bytes the deflate and pack kernels have to move (records in, slots out
          and in, members out) as a share of 6.3 TB/s, and the wall clock of a call through the Python mirror (one call of the entry into pageable memory, the bytes copied out of it)
      (b) per depth the members' size against what pgz writes (a gzip member per 32 MB, zlib at its default level) and the same at
          level 1, on the first `sample-mb` MB of the same records, and the seconds those take a core
      (c) pemapper_hip with PEMAPPER_OUTPUT_TIMES=1 on the inputs of tools/cli_throughput.sh, medians of three: this build with the
          switch off and on, and the parent commit's binary (--parent-exe; its outputs time is its wall clock less its "read and
          mapped" time)"""
import argparse
import os
import re
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HBM = 6.3e12
PGZ_PIECE = 32 << 20


def kernels_and_sizes(a):
    from pecaller_amd import PemapDev
    G = 1 << a.genome_log2
    dev = PemapDev(0)
    d_g, contig_len = dev.synth_genome(20240601, G, 4, 0.02)
    dev.build_index_resident(d_g, G, contig_len)
    dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
    B, L, done = 1 << 20, 150, 0
    for depth in [int(x) for x in a.depths.split(",")]:
        want = depth * G // (2 * L)
        while done < want:
            n = min(B, want - done)
            dev.synth_reads(7, n, L, paired=True, sub_rate=0.004, indel_rate=0.0002, first_read=done)
            dev.run()
            done += n
        rec = dev.fetch_records(0, G)
        ms, wall = [], []
        for k in range(a.reps + 1):
            t0 = time.time()
            gz, n_rec, ins = dev.fetch_records_gz(0, G)
            wall.append((time.time() - t0) * 1e3)
            ms.append(dev.fetch_gz_ms())
        med = {k: float(np.median([m[k] for m in ms[1:]])) for k in ms[0]}
        pieces = (n_rec + 511) // 512
        moved_deflate, moved_pack = rec.nbytes + len(gz), 2 * len(gz)
        print("depth %3dx: %d records (%.1f MB), %d insertion sites, %d members, %.1f MB of gz = %.2f : 1" %
              (depth, n_rec, rec.nbytes / 1e6, len(ins), pieces, len(gz) / 1e6, rec.nbytes / max(1, len(gz))))
        print("   kernels, ms: records %.3f, insertion list %.3f, deflate %.3f (%.0f GB/s of records, %.1f %% of 6.3 TB/s by bytes moved), "
              "scan + pack %.3f (%.1f %%); a call's wall clock %.1f ms (min %.1f)" %
              (med["records"], med["insertions"], med["deflate"], rec.nbytes / med["deflate"] / 1e6, 100 * moved_deflate / (med["deflate"] * 1e-3) / HBM,
               med["pack"], 100 * moved_pack / (med["pack"] * 1e-3) / HBM, float(np.median(wall[1:])), min(wall[1:])))
        m = min(len(rec), a.sample_mb * (1 << 20) // 16) // 512 * 512
        if m:
            sample = rec[:m].tobytes()
            last = int(rec["pos"][m - 1])
            gz_s = dev.fetch_records_gz(0, last + 1)[0]
            # what pgz writes: a gzip member per PGZ_PIECE = 32 MB of records (host_io.h), each deflated on its own
            def pgz_size(level):
                t0 = time.time()
                size = sum(18 + len(zlib.compress(sample[o:o + PGZ_PIECE], level)) - 6 for o in range(0, len(sample), PGZ_PIECE))
                return size, time.time() - t0
            z6, t6 = pgz_size(6)
            z1, t1 = pgz_size(1)
            print("   first %.1f MB of records: device members %.2f : 1; pgz's members of 32 MB at zlib 6 %.2f : 1 (%.2f s of a core), at zlib 1 "
                  "%.2f : 1 (%.2f s); the device's file is %.2f x the former, %.2f x the latter" % (len(sample) / 1e6, len(sample) / len(gz_s), len(sample) / z6, t6,
                                                                                                  len(sample) / z1, t1, len(gz_s) / z6, len(gz_s) / z1))
        sys.stdout.flush()
    dev.close()


def cli(a):
    """the inputs of tools/cli_throughput.sh: the golden g1 index and `copies` x its 20,000 pairs as one gz file per mate"""
    import gzip
    import shutil
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refio
    gold = os.path.join(ROOT, "tests", "golden")
    w = tempfile.mkdtemp()
    shutil.copy(os.path.join(gold, "g1.sdx"), w)
    _, seqs = refio.read_fasta(os.path.join(gold, "g1.fa.gz"))
    with gzip.open(os.path.join(w, "g1.seq"), "wb", compresslevel=1) as f:
        f.write(np.concatenate(seqs).tobytes())
    reads = []
    for k in (1, 2):
        one = open(os.path.join(gold, "g1_%d_.fastq.gz" % k), "rb").read()
        reads.append(os.path.join(w, "big_%d_.fastq.gz" % k))
        with open(reads[-1], "wb") as f:
            for _ in range(a.copies):
                f.write(one)
    exe = os.path.join(ROOT, "pecaller_amd", "pemapper_hip")
    configs = [("switch off", exe, {}), ("switch on", exe, {"PEMAPPER_DEVICE_GZ": "1"})]
    if a.parent_exe:
        configs.insert(0, ("parent", a.parent_exe, {}))
    env0 = {k: v for k, v in os.environ.items() if k != "PEMAPPER_DEVICE_GZ"}
    for name, prog, env in configs:
        secs, by_line = [], True
        for k in range(4):
            cmd = [prog, os.path.join(w, "out"), os.path.join(w, "g1.sdx"), "p", reads[0], reads[1], "500", "0", "N", "0.85", "16", "2000000000"]
            t0 = time.time()
            log = subprocess.run(cmd, env=dict(env0, PEMAPPER_OUTPUT_TIMES="1", **env), stdout=subprocess.PIPE, check=True, timeout=120).stdout.decode()
            wall = time.time() - t0
            m = re.search(r"outputs of \S+ written in ([0-9.]+) s", log)
            mapped = re.findall(r"read and mapped in ([0-9.]+) s", log)
            by_line = by_line and m is not None
            secs.append(float(m.group(1)) if m else wall - float(mapped[-1]))
        print("(c) %-10s outputs written in %.3f s (median of three after a warm-up; %.3f .. %.3f)%s; pileup.gz %.1f MB" %
              (name, float(np.median(secs[1:])), min(secs[1:]), max(secs[1:]), "" if by_line else " [wall less read-and-mapped: start-up and index build included]",
               os.path.getsize(os.path.join(w, "out.pileup.gz")) / 1e6))
        sys.stdout.flush()
    shutil.rmtree(w)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-log2", type=int, default=26)
    ap.add_argument("--depths", default="1,5,30,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample-mb", type=int, default=64)
    ap.add_argument("--copies", type=int, default=100)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--parent-exe")
    a = ap.parse_args()
    kernels_and_sizes(a)
    if not a.skip_cli:
        cli(a)
