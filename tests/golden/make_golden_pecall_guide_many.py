#!/usr/bin/env python3
"""Golden vectors for pecaller's BED guide mode with many short intervals (development container only; needs oracle/_ref).

The unmodified reference run with a guide file (pecaller.c:925-1068) on 8 samples and the renamed contig table of
make_golden_pecall_guide.py (pecall_guide.sdx: contigs 2 and 3 are chrY / chrMT).  The BED has 40 lines and 2,665 guided positions:
single positions, adjacent intervals (one ends where the next begins), an interval no sample has a record in (chr1:1700-1720), gaps
that hold records (chr1:1261-1599 is longer than any run of the device's tile kernel), an interval longer than 1,024 positions, the last
bases of chr1 and the first of chrY 15 positions apart, and intervals on chr1, chrY and chrMT.  A second BED has two more lines that go
backwards: one overlaps positions already called, one lies in front of everything.  Both runs read the same pileup files.  Stores
under tests/golden/:

  pecall_guide_many.npz                reads[record][sample][6] and pos[record] (the pileup records), sample names, column order, tail
  pecall_guide_many.bed / _back.bed    the guide intervals
  pecall_guide_many{,_back}.base.txt.gz / .snp.txt / .dist.txt   what the reference wrote (rows sorted)

  python3 tests/golden/make_golden_pecall_guide_many.py [--work /tmp/gold_guide_many]
"""
import argparse
import gzip
import os
import shutil
import struct
import subprocess
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFBIN = os.path.join(ROOT, "oracle", "_ref", "pecaller")
BED = [("chr1", 1001, 1100), ("chr1", 1101, 1150), ("chr1", 1200, 1200), ("chr1", 1202, 1202), ("chr1", 1230, 1260), ("chr1", 1600, 1650),
       ("chr1", 1700, 1720), ("chr1", 1800, 1815), ("chr1", 2500, 2560), ("chr1", 2900, 3100), ("chr1", 3101, 3101), ("chr1", 4000, 4040),
       ("chr1", 5200, 6400), ("chr1", 6405, 6410), ("chr1", 172650, 172700), ("chr1", 172710, 172718),
       ("chrY", 1, 12), ("chrY", 20, 20), ("chrY", 500, 640), ("chrY", 641, 700), ("chrY", 900, 905), ("chrY", 1000, 1003), ("chrY", 1010, 1010),
       ("chrY", 1012, 1030), ("chrY", 1100, 1180), ("chrY", 1500, 1540), ("chrY", 2100, 2130),
       ("chrMT", 200, 330), ("chrMT", 331, 331), ("chrMT", 400, 460), ("chrMT", 470, 470), ("chrMT", 600, 640), ("chrMT", 700, 700),
       ("chrMT", 702, 710), ("chrMT", 800, 850), ("chrMT", 1000, 1040), ("chrMT", 1300, 1330), ("chrMT", 1340, 1345), ("chrMT", 2000, 2050),
       ("chrMT", 2060, 2060)]
BACK = [("chrMT", 1995, 2010), ("chr1", 500, 520)]
UNCOVERED = ("chr1", 1700, 1720)
# records beyond the intervals' surroundings: a long gap between two intervals, and in front of everything
EXTRA = [("chr1", 1261, 1599), ("chr1", 480, 540)]
CNAME = ["chr1", "chrY", "chrMT"]


def write_bed(path, lines):
    with open(path, "w") as f:
        for b in lines:
            f.write("%s\t%d\t%d\n" % b)


def run_reference(rundir, sdx, bed, tag):
    for f in ("out.base.gz", "out.snp", "out.piles.gz", "out.dist"):
        if os.path.exists(os.path.join(rundir, f)):
            os.remove(os.path.join(rundir, f))
    subprocess.check_call([REFBIN, "pileup", sdx, "20", "out", "0.95", "0.001", "n", "2", "n", bed], cwd=rundir, stdout=subprocess.DEVNULL)
    base = gzip.open(os.path.join(rundir, "out.base.gz"), "rt").read().split("\n")
    snp = open(os.path.join(rundir, "out.snp")).read().split("\n")
    with gzip.open(os.path.join(HERE, tag + ".base.txt.gz"), "wt") as f:
        f.write(base[0] + "\n" + "\n".join(sorted(x for x in base[1:] if x)) + "\n")
    with open(os.path.join(HERE, tag + ".snp.txt"), "w") as f:
        f.write(snp[0] + "\n" + "\n".join(sorted(x for x in snp[1:] if x)) + "\n")
    shutil.copy(os.path.join(rundir, "out.dist"), os.path.join(HERE, tag + ".dist.txt"))
    print(tag, "base rows", len([x for x in base[1:] if x]), "snp rows", len([x for x in snp[1:] if x]))
    return [c for c in base[0].split("\t")[3:] if c]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/gold_guide_many")
    a = ap.parse_args()
    W = a.work
    shutil.rmtree(W, ignore_errors=True)
    os.makedirs(W)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refio
    _, seqs = refio.read_fasta(os.path.join(HERE, "g1.fa.gz"))
    seq = b"".join(x.tobytes() for x in seqs)
    sdx = open(os.path.join(HERE, "pecall_guide.sdx")).read().split("\n")
    shutil.copy(os.path.join(HERE, "pecall_guide.sdx"), os.path.join(W, "g1.sdx"))
    with gzip.open(os.path.join(W, "g1.seq"), "wb") as f:
        f.write(seq)
    write_bed(os.path.join(HERE, "pecall_guide_many.bed"), BED)
    write_bed(os.path.join(HERE, "pecall_guide_many_back.bed"), BED + BACK)
    lens = [int(x.split("\t")[0]) + 15 for x in sdx[1:11]]
    starts = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(424242)
    n_samp = 8
    names = ["s%d" % i for i in range(n_samp)]
    depth = [30, 28, 33, 25, 38, 14, 9, 45]
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    # the positions that may have a record: 20 to either side of every interval (skipped by the guide), the extra stretches
    where = set()
    for cn, lo, hi in BED:
        ci = CNAME.index(cn)
        for p1 in range(max(lo - 20, 1), min(hi + 20, lens[ci] - 15) + 1):
            where.add((ci, p1))
    for cn, lo, hi in EXTRA:
        for p1 in range(lo, hi + 1):
            where.add((CNAME.index(cn), p1))
    cn, lo, hi = UNCOVERED
    for p1 in range(lo - 5, hi + 6):
        where.discard((CNAME.index(cn), p1))
    pos, reads = [], []
    for ci, p1 in sorted(where):
        g = int(starts[ci]) + p1 - 1
        r = code.get(seq[g])
        if r is None or rng.random() < 0.05:      # 5 % of the positions have no record at all
            continue
        var = rng.random() < 0.06
        alt = int(rng.integers(0, 6))
        q = rng.uniform(0.1, 0.6)
        col = np.zeros((n_samp, 6), np.uint16)
        for s in range(n_samp):
            if rng.random() < 0.03:
                continue                           # this sample has no record here
            d = int(rng.poisson(depth[s]))
            if ci == 0:
                gt = tuple(alt if (var and rng.random() < q) else r for _ in range(2))
            else:
                a1 = alt if (var and rng.random() < q) else r
                gt = (a1, a1)
            for _ in range(d):
                al = gt[int(rng.integers(0, 2))]
                if rng.random() < 0.004:
                    al = int(rng.integers(0, 4))
                if al == 5:
                    col[s, r] += 1
                col[s, al] += 1
        pos.append(g)
        reads.append(col)
    pos = np.array(pos, np.uint32)
    reads = np.array(reads, np.uint16)
    rundir = os.path.join(W, "run")
    os.makedirs(rundir)
    tail = int(starts[3]) + 5000
    for s in range(n_samp):
        recs = [struct.pack("<I6H", int(pos[i]), *[int(x) for x in reads[i, s]]) for i in range(len(pos)) if reads[i, s].sum() > 0]
        recs += [struct.pack("<I6H", tail + k, 20, 0, 0, 0, 0, 0) for k in range(40)]   # keeps the files open past the last interval
        with gzip.open(os.path.join(rundir, "%s.pileup.gz" % names[s]), "wb") as f:
            f.write(b"".join(recs))
    cols = run_reference(rundir, os.path.join(W, "g1.sdx"), os.path.join(HERE, "pecall_guide_many.bed"), "pecall_guide_many")
    cols2 = run_reference(rundir, os.path.join(W, "g1.sdx"), os.path.join(HERE, "pecall_guide_many_back.bed"), "pecall_guide_many_back")
    assert cols == cols2
    np.savez_compressed(os.path.join(HERE, "pecall_guide_many.npz"), reads=reads, pos=pos, names=np.array(names), columns=np.array(cols),
                        tail=np.array([tail]))
    print("records", len(pos), "guided positions", sum(hi - lo + 1 for _, lo, hi in BED), "columns", cols)


if __name__ == "__main__":
    main()
