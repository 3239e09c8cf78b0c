#!/usr/bin/env python3
"""Golden vectors for the planted columns of tests/site_cases.py (development container only: needs the reference programs under oracle/_ref):
the oracle is the only authority at these edges and was written by the same hands as the kernels, so the UNMODIFIED reference
(oracle/_ref/pecaller, gcc -O1, one worker thread) is run on the planted columns of 8 and of 129 samples.

Every planted column of site_cases.cases(N) goes to the next position of g1's first contig whose letter is its family's reference
base (the reference reads the base from the genome); every column is autosomal there (chr1), whatever chromosome byte the builder
gives it.  Three runs on the same pileups: threshold 0.95 theta 0.001, threshold 0.99 theta 0.01, and HAPLOID with 0.95 0.001.
Stored under tests/golden/, inputs and printed rows only:

  pecall_edges<N>.npz                 reads[site][sample][6] (u16), pos[site], family and name of the site, sample names, the reference's column order
  pecall_edges<N>.base.txt.gz         the reference's <out>.base.gz rows, sorted, of the first run; .snp.txt its <out>.snp rows
  pecall_edges<N>_t99.* / _hap.*      the same of the second and third run

  python3 tests/golden/make_golden_pecall_edges.py [--work /tmp/gold_edges]
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
RUNS = (("", "0.95", "0.001", "n"), ("_t99", "0.99", "0.01", "n"), ("_hap", "0.95", "0.001", "y"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/gold_edges")
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import refio
    import site_cases
    contigs = refio.read_fasta(os.path.join(HERE, "g1.fa.gz"))
    seq = b"".join(x.tobytes() for x in contigs[1])
    for n_samp in (8, 129):
        W = os.path.join(a.work, str(n_samp))
        shutil.rmtree(W, ignore_errors=True)
        os.makedirs(W)
        shutil.copy(os.path.join(HERE, "g1.sdx"), os.path.join(W, "g1.sdx"))
        with gzip.open(os.path.join(W, "g1.seq"), "wb") as f:
            f.write(seq)
        names = ["e%03d" % i for i in range(n_samp)]
        reads, pos, family, name = [], [], [], []
        at = 5000
        for k, (fam, cols) in enumerate(site_cases.cases(n_samp).items()):
            letter = b"ACGT"[site_cases.family_dom(k)]
            for nm, r, _ in cols:
                at += 2                         # (a position without reads between two columns)
                while seq[at] != letter:
                    at += 1
                reads.append(r)
                pos.append(at)
                family.append(fam)
                name.append(nm)
        reads = np.array(reads, np.uint16)
        pos = np.array(pos, np.uint32)
        assert pos[-1] + 100 < len(contigs[1][0])
        rundir = os.path.join(W, "run")
        os.makedirs(rundir)
        pad = 40                                # sites in flight when the reader finishes are lost (pecaller.c:1071, 1207)
        for s in range(n_samp):
            recs = [struct.pack("<I6H", int(pos[i]), *[int(x) for x in reads[i, s]]) for i in range(len(pos)) if reads[i, s].sum() > 0]
            recs += [struct.pack("<I6H", int(pos[-1]) + 1 + k, 20, 0, 0, 0, 0, 0) for k in range(pad)]
            with gzip.open(os.path.join(rundir, "%s.pileup.gz" % names[s]), "wb") as f:
                f.write(b"".join(recs))
        cols0 = None
        for tag, thr, theta, hap in RUNS:
            out = "out" + tag
            subprocess.check_call([REFBIN, "pileup", os.path.join(W, "g1.sdx"), str(n_samp + 5), out, thr, theta, hap, "2", "n"], cwd=rundir,
                                  stdout=subprocess.DEVNULL)
            base = gzip.open(os.path.join(rundir, out + ".base.gz"), "rt").read().split("\n")
            hdr, rows = base[0], sorted(x for x in base[1:] if x)
            cols = [c for c in hdr.split("\t")[3:] if c]       # the column order is the directory order the reference saw
            assert cols0 is None or cols == cols0
            cols0 = cols
            snp = open(os.path.join(rundir, out + ".snp")).read().split("\n")
            last = int(pos[-1]) + 1
            keep_rows = [x for x in rows if int(x.split("\t")[1]) <= last]
            keep_snp = [x for x in sorted(x for x in snp[1:] if x) if int(x.split("\t")[1]) <= last]
            stem = os.path.join(HERE, "pecall_edges%d%s" % (n_samp, tag))
            with gzip.open(stem + ".base.txt.gz", "wt") as f:
                f.write(hdr + "\n" + "\n".join(keep_rows) + "\n")
            with open(stem + ".snp.txt", "w") as f:
                f.write(snp[0] + "\n" + "\n".join(keep_snp) + "\n")
            print("samples", n_samp, "run", tag or "default", "sites", len(pos), "base rows", len(keep_rows), "snp rows", len(keep_snp))
        np.savez_compressed(os.path.join(HERE, "pecall_edges%d.npz" % n_samp), reads=reads, pos=pos, family=np.array(family), name=np.array(name),
                            names=np.array(names), columns=np.array(cols0), pad=np.array([pad]))


if __name__ == "__main__":
    main()
