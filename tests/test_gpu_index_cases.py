"""The device-built index, the look-up replicas and the seed stage's reading of them on the ladder genome of index_cases.py: buckets of
exactly 1 .. 12, 98, 99, 100, 101 and 250 positions, k-mers 0 and 0xFFFFFFFF with positions in them, both indexing modes, contig
ends on the builder's tile, round and wave seams.  Expectations: refio.kmer_index (tied to the reference builder's files by
test_index_cases_cpu.py) and the oracle (index_cases.expected)."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import fixtures
import index_cases as ic
import refio

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MODES = (("plain", False), ("bisulfite", True))


def _worker(*args):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, HERE]))
    r = subprocess.run([sys.executable, os.path.join(HERE, "index_gpu_worker.py")] + list(args), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and b"index ok" in r.stdout, r.stdout[-3000:]
    print(r.stdout.decode().strip().split("\n")[-1])


@pytest.mark.parametrize("size", ["full", "trunc"])
@pytest.mark.parametrize("mode", ["plain", "bisulfite"])
def test_index_arrays_equal_the_reference_builders(mode, size):
    """pemap_dev_build_index on the ladder genome, and on its first contigs alone (a length that is a multiple of the builder's 4096
    tile): the positions byte for byte with the reference's .mdx md5, contig starts, letters, index_info, and the prefix table over
    all 2^32 + 1 entries (reduced to its change points on the device, compared with (ukmer, ustart) and the reference's md5)."""
    _worker("arrays", mode, size)


@pytest.mark.parametrize("mode", ["plain", "bisulfite"])
def test_lookup_replicas_over_every_kmer(mode):
    """replica 0 against the expected table at every one of the 2^32 k-mers (empty, the only position, a record of 2 .. 99 positions in
    .mdx order padded with zeros to its unit, the marker at 100 or more and for the all-T k-mer's wrapped length), every ladder
    size present; replicas 1 .. 7 as rep[p][swap_fields(k, p)] == rep[0][k] over all k; record_bytes."""
    _worker("replicas", mode, "full")


def _compare_with_oracle(dev, e, n):
    dbg = dev.debug_hits(2 * n)
    counts, ins = dev.fetch_pileup()
    assert np.array_equal(counts, e["counts"])
    assert sorted(ins) == e["ins"]
    assert np.array_equal(np.array(dev.summary()), np.array(e["summary"]))
    for which, od in enumerate(e["d"]):
        nh = dbg["n_hits"][which::2]
        assert np.array_equal(nh, od["n_hits"]), np.nonzero(nh != od["n_hits"])[0][:10]
        for i in np.nonzero(nh)[0]:
            k = nh[i]
            x = 2 * i + which
            assert np.array_equal(dbg["spot"][x, :k], od["spot"][i, :k]), x
            assert np.array_equal(dbg["orient"][x, :k], od["orient"][i, :k]), x
            assert np.array_equal(dbg["win_start"][x, :k].astype(np.int32), od["win_start"][i, :k]), x
            assert np.array_equal(dbg["win_len"][x, :k], od["win_len"][i, :k]), x
            assert np.array_equal(dbg["score"][x, :k].view(np.uint64), od["score"][i, :k].view(np.uint64)), (x, k)
            assert np.array_equal(dbg["start_k"][x, :k], od["start"][i, :k, 0]), x
            assert np.array_equal(dbg["start_i"][x, :k], od["start"][i, :k, 1]), x


@pytest.mark.parametrize("env", [{}, {"PEMAP_REPLICAS": "0"}, {"PEMAP_BIG_BLOCKS_PER_CU": "1"}], ids=["default", "no_replicas", "big_grid_1"])
@pytest.mark.parametrize("bis", [False, True], ids=["plain", "bisulfite"])
@pytest.mark.parametrize("L", [64, 150])
def test_mapping_at_the_limit(L, bis, env, monkeypatch):
    """the reads that tile the families and the homopolymer stretches at every phase, through the fused seed kernel, the reference's
    table layout and another grid of pm_seed_kernel: coordinates, classes, pileup, insertions, summary, and per end the hit list,
    the window geometry, the score bits and the start cells equal the oracle's.  The ends of 150 bases that hold four segments of
    the n99x3 unit have 4 x 297 positions on a strand, over the 1,024 the wave-per-end kernels keep: at least they must take the
    big-end path (a floor from the index alone; each seed path has its own capacity and sends more, the fused kernel also ends of
    64 bases)."""
    from pecaller_amd import PemapDev
    for k, v in env.items():
        monkeypatch.setenv(k, v)           # the knobs are read by pemap_dev_create, once per object
    ix = ic.index(bis)
    b1, l1, b2, l2 = ic.reads(L, bis)
    e = ic.expected(L, bis)
    n = len(l1)
    dev = PemapDev(0)
    dev.build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
    assert dev.lookup_replicas()[0] == (0 if env.get("PEMAP_REPLICAS") == "0" else 8)
    dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85, bisulfite=bis)
    m1, m2, mt = dev.map_batch(b1, l1, b2, l2)
    stats, _ = dev.run_stats()
    try:
        assert np.array_equal(m1, e["m1"]), np.nonzero(m1 != e["m1"])[0][:10]
        assert np.array_equal(m2, e["m2"]), np.nonzero(m2 != e["m2"])[0][:10]
        assert np.array_equal(mt, e["mt"])
        _compare_with_oracle(dev, e, n)
    finally:
        dev.close()
    # ends that must be big: four whole segments of the n99x3 unit, the unit untouched, read in the orientation that the index holds
    must = sum(1 for p in ic.read_plan(L) if p["kind"] == "n99x3" and p["sib"] == 0 and ic.segments_inside(p, L) == 4
               and (p["broken"] or p["subs"] == 0) and not (bis and p["strand"] == 1))
    print("big_ends", stats["big_ends"], "at least", must)
    assert (must > 0) == (L == 150) and stats["big_ends"] >= must, (stats, must)
    assert stats["ends"] == 2 * n


@pytest.mark.parametrize("mode,bis", MODES)
def test_index_builder_cli_on_the_untidy_fasta(tmp_path, mode, bis, monkeypatch):
    """index_genome_hip on the FASTA file that needs toupper, the isalpha filter and the 255-byte pieces (lower case, digits, '*',
    '-', CRLF, lines of 700 and 5,000 letters, headers with a description), answering N and Y to the bisulfite question: .sdx,
    .seq, .mdx and the compacted .idx are the reference builder's.  Without conversion the four files then go into pemapper_hip
    (PEMAP_INDEX_FROM_FILES=1) with the 150-base reads: the oracle's coordinates."""
    exe = os.path.join(ROOT, "pecaller_amd", "index_genome_hip")
    assert os.path.exists(exe)
    with open(os.path.join(fixtures.GOLD, "ladder.json")) as f:
        m = json.load(f)[mode]
    fa = tmp_path / "ladder.fa"
    with gzip.open(os.path.join(fixtures.GOLD, "ladder.fa.gz"), "rb") as f, open(fa, "wb") as o:
        shutil.copyfileobj(f, o)
    base = str(tmp_path / "lx")
    ans = "S\n%d\n%s\n%s\n%s\n" % (len(ic.genome()["contigs"]) + 2, fa, base, "Y" if bis else "N")
    subprocess.run([exe], input=ans.encode(), stdout=subprocess.DEVNULL, check=True)
    assert open(base + ".sdx").read() == open(os.path.join(fixtures.GOLD, "ladder.sdx")).read()
    seq = gzip.open(base + ".seq", "rb").read()
    assert len(seq) == m["seq_len"] and refio.md5(np.frombuffer(seq, np.uint8)) == m["seq_md5"]
    mdx = np.fromfile(base + ".mdx", dtype="<u4")
    assert len(mdx) == m["n_mers"] and refio.md5(mdx) == m["mdx_md5"]
    uk, us = refio.idx_to_compact(base + ".idx")
    assert len(uk) == m["n_ukmer"] and refio.md5(uk) == m["idx_ukmer_md5"] and refio.md5(us) == m["idx_ustart_md5"]
    if bis:
        return
    r1, r2, _ = ic.read_ends(150, False)
    files = []
    for tag, rs in ((1, r1), (2, r2)):
        files.append(str(tmp_path / ("lad_%d_.fastq.gz" % tag)))
        with gzip.open(files[-1], "wb", compresslevel=1) as f:
            for i, r in enumerate(rs):
                f.write(b"@p%d/%d\n%s\n+\n%s\n" % (i, tag, r, b"I" * len(r)))
    monkeypatch.setenv("PEMAP_INDEX_FROM_FILES", "1")
    r = subprocess.run([os.path.join(ROOT, "pecaller_amd", "pemapper_hip"), str(tmp_path / "out"), base + ".sdx", "p", files[0], files[1],
                        "500", "0", "N", "0.85", "8", "200000000"], stdout=subprocess.PIPE)
    assert r.returncode == 0, r.stdout[-2000:]
    e = ic.expected(150, False)
    assert np.array_equal(np.fromfile(files[0] + ".mfile", dtype="<u4"), e["m1"])
    assert np.array_equal(np.fromfile(files[1] + ".mfile", dtype="<u4"), e["m2"])


def test_unindexable_genomes_are_refused_and_the_object_lives_on():
    """a contig of 15 letters, and a genome without a 16-mer free of N: each refused with its message (error returns checked on the
    host; the reference accepts contigs under 16 letters), and the same object then builds the ladder index"""
    from pecaller_amd import PemapDev, PemapError
    rng = np.random.default_rng(3)
    dev = PemapDev(0)
    g = ic.ACGT[rng.integers(0, 4, 1015)]
    with pytest.raises(PemapError, match="contig 1 has 15 letters"):
        dev.build_index(g, np.array([500, 15, 500], np.uint32))
    g = ic.ACGT[rng.integers(0, 4, 64)].copy()
    g[15::16] = ord("N")
    with pytest.raises(PemapError, match="no 16-mer free of N"):
        dev.build_index(g, np.array([32, 32], np.uint32))
    ix = ic.index(False)
    dev.build_index(ix["genome"], ix["contig_len"])
    assert dev.index_info() == (len(ix["mers"]), len(ix["genome"]), len(ix["contig_len"]), 16)
    assert np.array_equal(dev.read_buffer(1, np.uint32), ix["mers"])
    assert np.array_equal(dev.read_buffer(3, np.uint32), ix["contig_starts"])
    dev.close()
