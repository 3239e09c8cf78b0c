"""The ladder genome of index_cases.py, CPU only: the numpy index builder (refio.kmer_index) against the files of the reference's
index_genome_whole for both modes (tests/golden/ladder*, made by make_golden_index.py), floors that say the genome holds what it
was built for -- every ladder bucket size, both ends of the k-mer range, contig ends on the builder's tile, round and wave seams --
and the oracle's results on the reads, which test_gpu_index_cases.py expects of the device.  The floors are read from
refio.kmer_index's output and the oracle's debug records alone: a changed generator cannot quietly lose a case.

Reads whose results change (coordinates, hit counts or hit lists) when the oracle is built with one deliberate error, as measured
(read length, b = bisulfite; 2,213 pairs of 64 bases, 6,210 of 150):

  variant                                   64   64b   150  150b
  limit 99  (this_tot >= 99)               500   261   762   385
  limit 101 (this_tot >= 101)              219   108   381   213
  the rule on the sum of the 49 buckets    483   288   889   552
  no 32-bit wrap of `which + 1`             48   127    31   178
"""
import json
import os

import numpy as np
import pytest

import fixtures
import index_cases as ic
import refio

MODES = (("plain", False), ("bisulfite", True))
DROPPED = {("f100", 0), ("f101", 0), ("n99_100", 0), ("n99_100", 1)}        # a bucket of the segment's 49 is on or over the limit


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(fixtures.GOLD, "ladder.json")) as f:
        return json.load(f)


def test_untidy_fasta_reads_to_the_generated_letters():
    """lower case, digits, '*', '-', blanks, CRLF, lines of 700 and 5,000 letters, headers with a description: refio.read_fasta gives
    the generator's contigs and the names the reference builder makes"""
    g = ic.genome()
    names, contigs = refio.read_fasta(os.path.join(fixtures.GOLD, "ladder.fa.gz"))
    assert names == g["names"]
    assert len(contigs) == len(g["contigs"]) and all(np.array_equal(a, b) for a, b in zip(contigs, g["contigs"]))
    import gzip
    raw = gzip.open(os.path.join(fixtures.GOLD, "ladder.fa.gz"), "rb").read()
    lines = raw.split(b"\n")
    seq = [x for x in lines if not x.startswith(b">")]
    assert max(len(x) for x in seq) > 4195 and sum(255 < len(x) <= 4195 for x in seq) >= 1
    assert any(x.endswith(b"\r") for x in seq) and any(not x.endswith(b"\r") for x in seq)
    body = b"".join(seq)
    assert all(body.count(ch) > 0 for ch in b"0123456789*-acgtnACGTN")
    assert any(b" " in x and x.rstrip(b"\r").endswith(b";") for x in lines if x.startswith(b">"))


@pytest.mark.parametrize("mode,bis", MODES)
def test_numpy_index_equals_reference_files(meta, mode, bis):
    g = ic.genome()
    ix = ic.index(bis)
    m = meta[mode]
    assert len(ix["mers"]) == m["n_mers"] and refio.md5(ix["mers"]) == m["mdx_md5"]
    assert len(ix["ukmer"]) == m["n_ukmer"] and refio.md5(ix["ukmer"]) == m["idx_ukmer_md5"]
    assert refio.md5(ix["ustart"]) == m["idx_ustart_md5"]
    assert len(ix["genome"]) == m["seq_len"] and refio.md5(ix["genome"]) == m["seq_md5"]
    assert ic.sdx_text(g["names"], g["contigs"]) == open(os.path.join(fixtures.GOLD, "ladder.sdx")).read()     # (one file: the modes' are equal)
    lens, names, idepth = refio.read_sdx(os.path.join(fixtures.GOLD, "ladder.sdx"))
    assert np.array_equal(np.cumsum([0] + lens), ix["contig_starts"]) and idepth == 16


@pytest.mark.parametrize("mode,bis", MODES)
def test_planted_buckets_have_their_sizes(mode, bis):
    g = ic.genome()
    ix = ic.index(bis)
    cst = ix["contig_starts"].astype(np.int64)
    assert tuple(sorted(g["islands"])) == ic.ISLANDS
    for c, (mer, places) in g["islands"].items():
        k = ic.kmer_of(mer, bis)
        assert ic.bucket_len(ix, k) == c == len(places)
        i = int(np.searchsorted(ix["ukmer"], k))
        # ... and hold the planted positions, in genome order
        assert ix["mers"][ix["ustart"][i]:ix["ustart"][i + 1]].tolist() == [int(cst[cc] + o) for cc, o in places]
    assert [name for name, _ in ic.FAMILIES] == list(g["families"])
    for (name, copies), group in zip(ic.FAMILIES, g["families"].values()):
        assert tuple(len(p) for _, p in group) == copies
        for unit, places in group:
            assert all(ic.bucket_len(ix, ic.kmer_of(unit[o:o + 16], bis)) == len(places) for o in range(ic.UNIT - 15)), name
            assert min(b[1] - a[1] for a, b in zip(places, places[1:]) if a[0] == b[0]) >= 300
        # every 16-mer of a sibling is one substitution from the unit's, and not the same k-mer in either mode
        for unit, _ in group[1:]:
            for o in range(ic.UNIT - 15):
                a, b = group[0][0][o:o + 16], unit[o:o + 16]
                assert sum(x != y for x, y in zip(a, b)) == 1 and ic.kmer_of(a, bis) != ic.kmer_of(b, bis)
    # how many buckets there are of each size of the ladder's upper end: the islands' and 45 per family unit
    want = {60: 90, 98: 1 + 45, 99: 1 + 45 * 7, 100: 1 + 45 * 2, 101: 1 + 45, 250: 1}
    ln = np.diff(ix["ustart"].astype(np.int64))
    assert {s: int((ln == s).sum()) for s in want} == want
    assert int((ln >= ic.TOO_MANY).sum()) == want[100] + want[101] + want[250]
    for s in (1, 2, 3, 4, 5, 7, 8, 11, 12):
        assert int((ln == s).sum()) >= 1
    # both ends of the table: k-mer 0 (the 40 A) and the all-T k-mer (the 40 T; under bisulfite indexing also the C / T stretch)
    assert int(ix["ukmer"][0]) == 0 and ic.bucket_len(ix, 0) == 25
    assert int(ix["ukmer"][-1]) == 0xFFFFFFFF
    t = ic.bucket_len(ix, 0xFFFFFFFF)
    assert t == 25 if not bis else t >= 25 + 45
    c, o, n = g["homopolymers"]["T40"]
    i = len(ix["ukmer"]) - 1
    assert set(range(int(cst[c]) + o, int(cst[c]) + o + 25)) <= set(ix["mers"][ix["ustart"][i]:ix["ustart"][i + 1]].tolist())
    for name, letters in (("CT60", b"CT"), ("GA60", b"GA")):
        c, o, n = g["homopolymers"][name]
        x = g["contigs"][c]
        assert set(x[o:o + n].tobytes()) == set(letters) and n == 60 and x[o - 1] not in letters and x[o + n] not in letters


def test_letters_and_contig_layout():
    g = ic.genome()
    cs = g["contigs"]
    real = ic.real_starts(cs)
    ix = ic.index(False)
    # every seam and distance occurs as the real position of a contig end
    upper = {ic.WAVE: ic.ROUND, ic.ROUND: ic.TILE}
    seen = set()
    for c, base, delta in g["ends"]:
        e = int(real[c + 1]) - delta
        assert e % base == 0 and (base == ic.TILE or e % upper[base] != 0), (c, base, delta)
        seen.add((base, delta))
    assert seen == {(b, d) for b in (ic.TILE, ic.ROUND, ic.WAVE) for d in ic.DELTAS}
    assert real[-1] % ic.TILE != 0 and real[g["n_trunc"]] % ic.TILE == 0 and 0 < g["n_trunc"] < len(cs)
    assert 300000 <= real[-1] <= 500000
    # the small contigs: one k-mer, two, none
    st = ix["contig_starts"].astype(np.int64)
    for key, n_letters, n_kmers in (("c16", 16, 1), ("c17", 17, 2), ("c16n", 16, 0)):
        c = g["small"][key]
        assert len(cs[c]) == n_letters and st[c + 1] - st[c] == n_letters - 15
        assert int(((ix["mers"] >= st[c]) & (ix["mers"] < st[c + 1])).sum()) == n_kmers
    assert cs[g["first_n"]][0] == ord("N") and cs[g["last_n"]][-1] == ord("N")
    for n, (c, o) in g["n_runs"].items():
        x = cs[c]
        assert (x[o:o + n] == ord("N")).all() and x[o - 1] != ord("N") and x[o + n] != ord("N")
    assert sorted(g["n_runs"]) == [1, 15, 16, 17]
    letters = set(np.concatenate(cs).tobytes())
    assert set(b"RYKMSW") <= letters


@pytest.mark.parametrize("bis", [False, True])
@pytest.mark.parametrize("L", [64, 150])
def test_oracle_results_show_the_rule(L, bis):
    """the designed ends on the families, read from the oracle's debug records: where the unit's segments decide (64 bases: at least
    two of the four segments inside the unit and no substitution; 150 bases: the reads with broken flanks and at least three
    segments inside), an end on a family whose segment holds a bucket of 100 or more finds no hit at all, and an end on a family
    that stays below finds its place -- f99 against f100, the 60 + 60 siblings (kept) against 99 next to 100 (dropped).  Under
    bisulfite conversion only the ends that read the converted strand forward can map."""
    e = ic.expected(L, bis)
    plan = ic.read_plan(L)
    assert len(plan) == len(e["m1"]) and len(plan) > 2000
    nh, found = ic.designed_hits(L, bis)
    tally = {}
    for i, p in enumerate(plan):
        if p["kind"] not in dict(ic.FAMILIES) or (bis and p["strand"] == 1):
            continue
        inside = ic.segments_inside(p, L)
        decides = (p["broken"] and inside >= 3) if L >= 100 else (p["subs"] == 0 and inside >= 2)
        if not decides:
            continue
        key = (p["kind"], p["sib"])
        t = tally.setdefault(key, [0, 0])
        t[0] += 1
        if key in DROPPED:
            assert nh[i] == 0, (i, p)
        else:
            assert nh[i] >= 1, (i, p)
            t[1] += int(found[i])
    print(L, bis, tally)
    assert set(tally) == {(name, s) for name, copies in ic.FAMILIES for s in range(len(copies))}
    assert all(t[0] >= 5 for t in tally.values()), tally
    # (the place itself is in the list but for stray reads: another copy may gain a segment by chance, under conversion above all)
    assert all(t[1] >= 0.8 * t[0] for key, t in tally.items() if key not in DROPPED), tally
    # the homopolymer stretches are read from both strands and the ordinary reads map
    kinds = {p["kind"] for p in plan}
    assert set(ic.HOMOPOLYMERS) <= kinds and "ordinary" in kinds
    assert {(p["strand"], p["subs"]) for p in plan if p["kind"] == "T40"} >= {(s, n) for s in (0, 1) for n in (0, 1, 2)}
    for name in dict(ic.FAMILIES):          # every phase: the designed end starts at copy start - L + 16 ... copy start + 60
        ph = {p["start"] - p["target"] for p in plan if p["kind"] == name and p["sib"] == 0}
        assert ph == set(range(-L + 16, ic.UNIT + 1))
    assert int((e["m1"] > 0).sum()) > len(plan) // 4
