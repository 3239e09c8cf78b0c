#!/usr/bin/env python3
"""Regenerate the ladder* fixtures of tests/golden/ from the UNMODIFIED reference index builder (development container only).

The ladder genome of tests/index_cases.py, written as a deliberately untidy FASTA file (index_cases.write_untidy_fasta) -> the
reference's index_genome_whole twice, without and with bisulfite conversion, one run after the other (each holds tens of GB; about
2.5 min per run) -> per mode the sizes and md5 sums of its .seq, .mdx and the compact (ukmer, ustart) form of its .idx, and the
.sdx (the same text in both modes).  Reads nothing but oracle/_ref/ binaries (`make -C oracle ref`) and what index_cases.py generates; writes data files only.

  python3 tests/golden/make_golden_index.py [--work /tmp/gold_index] [--skip-run]
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
import index_cases  # noqa: E402
import refio  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
MODES = {"plain": "n", "bisulfite": "y"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", default="/tmp/gold_index")
    ap.add_argument("--skip-run", action="store_true", help="only collect from an existing work directory")
    a = ap.parse_args()
    W = a.work
    os.makedirs(W, exist_ok=True)
    fa = os.path.join(W, "ladder.fa")
    g = index_cases.genome()
    if not a.skip_run:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
        index_cases.write_untidy_fasta(fa, g)
        for mode, answer in MODES.items():
            # answers: Screen / max contigs / fasta / basename / bisulfite   (index_genome_whole.c:117-167)
            p = subprocess.Popen([os.path.join(REF, "index_genome_whole")], stdin=subprocess.PIPE, stdout=subprocess.DEVNULL, cwd=W)
            p.communicate(("s\n%d\n%s\n%s/%s\n%s\n" % (len(g["contigs"]) + 2, fa, W, mode, answer)).encode())
            assert p.returncode == 0, mode
    with open(fa, "rb") as f, gzip.GzipFile(os.path.join(HERE, "ladder.fa.gz"), "wb", mtime=0) as o:
        shutil.copyfileobj(f, o)
    meta = {}
    for mode in MODES:
        base = os.path.join(W, mode)
        mdx = np.fromfile(base + ".mdx", dtype="<u4")
        uk, us = refio.idx_to_compact(base + ".idx")
        seq = gzip.open(base + ".seq", "rb").read()
        meta[mode] = {"mdx_md5": refio.md5(mdx), "n_mers": int(len(mdx)), "idx_ukmer_md5": refio.md5(uk), "idx_ustart_md5": refio.md5(us),
                      "n_ukmer": int(len(uk)), "seq_md5": hashlib.md5(seq).hexdigest(), "seq_len": len(seq)}
        shutil.copy(base + ".sdx", os.path.join(HERE, "ladder.sdx"))
    assert open(os.path.join(W, "plain.sdx")).read() == open(os.path.join(W, "bisulfite.sdx")).read()     # (the .sdx knows no mode)
    with open(os.path.join(HERE, "ladder.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(json.dumps(meta, indent=1))


if __name__ == "__main__":
    main()
