#!/usr/bin/env python3
"""Regenerate the rpair* fixtures of tests/golden/ from the UNMODIFIED reference programs (development container only).

The genome and the L = 100 read set of tests/pair_cases.py (planted repeats, pairs built for every mapping class and for the
distance limits) -> reference index builder (about 2.5 min, about 20 GB RSS) -> the reference pemapper twice on the same reads:
  rpair_narrow   max_dist 300  min_dist 150  min_match 0.96   (both limits active, the threshold on a score: 96.0 == 100 * 0.96)
  rpair_base     max_dist 500  min_dist 0    min_match 0.85
Reads nothing but oracle/_ref/ binaries (`make -C oracle ref`) and what pair_cases.py generates; writes data files only.

  python3 tests/golden/make_golden_pair.py [--work /tmp/gold_pair] [--skip-run]
"""
import argparse
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pair_cases  # noqa: E402
import refio  # noqa: E402
import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
L = 100
RUNS = {
    # name: (max_dist, min_dist, min_match) as they stand on the command line
    "rpair_narrow": ("300", "150", "0.96"),
    "rpair_base": ("500", "0", "0.85"),
}


def run(cmd, **kw):
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/gold_pair")
    ap.add_argument("--skip-run", action="store_true", help="only collect from an existing work directory")
    a = ap.parse_args()
    W = a.work
    os.makedirs(W, exist_ok=True)
    f1, f2 = os.path.join(W, "rpair_1_.fastq.gz"), os.path.join(W, "rpair_2_.fastq.gz")
    if not a.skip_run:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
        g = pair_cases.genome()
        synth.write_fasta(os.path.join(W, "rpair.fa"), g["contigs"], g["names"])
        r1, r2, _ = pair_cases.read_ends(g, pair_cases.READ_SEED + L, pair_cases.PAIRS, L)
        for path, reads, tag in ((f1, r1, 1), (f2, r2, 2)):
            with gzip.GzipFile(path, "wb", mtime=0) as f:
                for i, r in enumerate(reads):
                    f.write(b"@p%d/%d\n%s\n+\n%s\n" % (i, tag, r, b"I" * len(r)))
        # answers: Screen / max contigs / fasta / basename / not bisulfite   (index_genome_whole.c:117-167)
        p = subprocess.Popen([os.path.join(REF, "index_genome_whole")], stdin=subprocess.PIPE, cwd=W)
        p.communicate(("s\n100\n%s/rpair.fa\n%s/rpair\nn\n" % (W, W)).encode())
        assert p.returncode == 0
        for name, (max_dist, min_dist, min_match) in RUNS.items():
            os.makedirs(os.path.join(W, name), exist_ok=True)
            run([os.path.join(REF, "pemapper"), os.path.join(W, name, "out"), os.path.join(W, "rpair.sdx"), "p", f1, f2, max_dist,
                 min_dist, "N", min_match, "8", "200000000"], stdout=subprocess.DEVNULL)
            for k, fq in ((1, f1), (2, f2)):       # (the .mfile lands beside the fastq file: keep each run's)
                shutil.move(fq + ".mfile", os.path.join(W, name, "m%d" % k))

    meta = {}
    with open(os.path.join(W, "rpair.fa"), "rb") as f, gzip.GzipFile(os.path.join(HERE, "rpair.fa.gz"), "wb", mtime=0) as g:
        shutil.copyfileobj(f, g)
    shutil.copy(os.path.join(W, "rpair.sdx"), os.path.join(HERE, "rpair.sdx"))
    mdx = np.fromfile(os.path.join(W, "rpair.mdx"), dtype="<u4")
    uk, us = refio.idx_to_compact(os.path.join(W, "rpair.idx"))
    seq = gzip.open(os.path.join(W, "rpair.seq"), "rb").read()
    meta["index"] = {"mdx_md5": refio.md5(mdx), "n_mers": int(len(mdx)), "idx_ukmer_md5": refio.md5(uk),
                     "idx_ustart_md5": refio.md5(us), "n_ukmer": int(len(uk)), "seq_md5": hashlib.md5(seq).hexdigest(),
                     "seq_len": len(seq)}
    for fq in (f1, f2):
        shutil.copy(fq, os.path.join(HERE, os.path.basename(fq)))
    for name, (max_dist, min_dist, min_match) in RUNS.items():
        d = os.path.join(W, name)
        for k in (1, 2):
            shutil.copy(os.path.join(d, "m%d" % k), os.path.join(HERE, "%s.m%d" % (name, k)))
        shutil.copy(os.path.join(d, "out.summary.txt"), os.path.join(HERE, name + ".summary.txt"))
        shutil.copy(os.path.join(d, "out.indel.txt.gz"), os.path.join(HERE, name + ".indel.txt.gz"))
        pile = refio.read_pileup(os.path.join(d, "out.pileup.gz"))
        np.save(os.path.join(HERE, name + ".pileup_sample.npy"), pile[::101])
        meta[name] = {"program": "pemapper", "extra_args": [], "paired": True, "max_dist": max_dist, "min_dist": min_dist,
                      "min_match": min_match, "pileup_md5": refio.md5(pile), "pileup_records": int(len(pile)),
                      "pileup_colsum": [int(x) for x in pile["c"].sum(axis=0)]}
    with open(os.path.join(HERE, "rpair.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
