"""The second tier of the fused seed kernel (pm_seed4_kernel < *, 1 >, pemap_seed4.hip.h) has a hand-out and a record phase of its
own: one read-end per fetch of the work counter (the first tier takes four), TAIL_DEPTH = 8 loads of 64 tail elements requested
before the first is stored (the first tier: 2), and the record headers of round r + 1 requested before round r's tails are walked.
Planted genomes as in test_gpu_seed_list_boundary.py; the expectations are the oracle's results and hit counts, and `positions` of
run_stats against a count made on the CPU from the index: an end processed twice shows there, an end skipped shows in its hits.

hand-out   PEMAP_FIRST_TIER=0 (every end goes to the second tier) and PEMAP_TIER2_WAVES=1 (a grid of one wave per CU): N distinct
           64-base ends of a random genome, N = 1, grid - 1, grid, grid + 1 and 4 grid + 3 -- a wave owns its first end by its
           number and draws every other from the counter, two values ahead of their use.
tails      a record is {count, p1, p2, p3 | p4 ...} in 16-byte units: the 4th and later positions of the records of a round are ONE
           flattened list, walked 64 TAIL_DEPTH = 512 elements a trip.  One end each whose flattened tail holds 511, 512, 513 and
           3 x 512 + 5 elements, made of records of 2, 3, 4 and 99 positions (0, 0, 1 and 96 tail elements: the first unit's boundary)
           and one of the size that completes the sum; once among islands only (the end does not map), once with the read itself
           planted too (it maps there).  Through the second tier (PEMAP_FIRST_TIER=0), and the ends of at most 1,424 positions through
           the first, whose depth is 2.
headers    ends with 128, 129, 256 and 257 records (rounds of 128), and the `limit` rule: while records of a LATER round still wait
           at the list's back, the front must stop at KCAP - nm (nm = the end's records).  An end of 129 records and 5,690
           positions -- 56 records of 99 and 73 of 2 -- fits the second tier's list of 5,696, but whichever record is the 129th, the
           first round's 128 hold at least 5,690 - 99 = 5,591 positions, more than 5,696 - 129 = 5,567: by the rule (rec_round's
           `nf > limit`, unchanged since the lists were made one) the second tier passes it on to pm_seed_kernel, mono_ends = 1."""
import functools

import numpy as np
import pytest

import oracle_py
import refio

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", np.uint8)
N1 = np.frombuffer(b"N", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[:] = ord("N")
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
KCAP1, KCAP2 = 1424, 4 * 1424               # PmSeed4Shared < 10, 0 / 1 >::KCAP
TOO_MANY = 100
DEPTH = 8                                   # PmSeed4Shared < *, 1 >::TAIL_DEPTH
LEN = 128                                   # the planted ends: 8 segments, the kernel form of the 2 x 150 headline (< 10, * >)


def _index(g):
    n = len(g) // 3
    contigs = [g[:n], g[n:2 * n], g[2 * n:]]
    mers, ukmer, ustart, cs = refio.kmer_index(contigs)
    return dict(mers=mers, ukmer=ukmer, ustart=ustart, genome=g, contig_starts=cs, contig_len=np.array([len(c) for c in contigs], np.uint32),
                names=["b0", "b1", "b2"])


def _kmer(x):
    k = 0
    for c in x:
        k = (k << 2) | b"ACGT".index(c)
    return k


def _sizes(ix):
    return dict(zip((int(k) for k in ix["ukmer"]), (int(n) for n in np.diff(ix["ustart"].astype(np.int64)))))


def buckets_of(size, read):
    """the sizes of the buckets the seed stage lists for an end of ACGT letters: per strand and segment the 49 buckets of the k-mer
    and its one-substitution neighbours, none when one of them holds too_many_spots or more (positions_of of
    test_gpu_seed_list_boundary.py, bucket by bucket)"""
    L = len(read)
    cuts = L // 16 - (1 if L % 16 == 0 else 0)
    offs = [16 * i for i in range(cuts)] + [L - 16]
    out = []
    for strand in (read, COMP[np.frombuffer(read, np.uint8)][::-1].tobytes()):
        for o in offs:
            k = _kmer(strand[o:o + 16])
            nb = [k] + [(k & ~(3 << (2 * f))) | (a << (2 * f)) for f in range(16) for a in range(4) if a != (k >> (2 * f)) & 3]
            sizes = [size.get(x, 0) for x in nb]
            if max(sizes) < TOO_MANY:
                out += [s for s in sizes if s]
    return out


def plant(rng, pieces, spec, locus):
    """a read of LEN random letters whose buckets are `spec` (positions per record, at least 2 each): record k is the bucket of
    segment k % 8 -- the segment's own k-mer for k < 8, then its one-substitution siblings --, planted as islands (N + 16 letters
    + N, 300 bases apart).  With `locus` the read itself is planted too, and the eight own k-mers have one island fewer."""
    S = LEN // 16
    read = ACGT[rng.integers(0, 4, LEN)].copy()
    assert max(spec) < TOO_MANY and min(spec) >= 2 and len(spec) <= 49 * S
    for k, c in enumerate(spec):
        seg, j = k % S, k // S
        s = read[16 * seg:16 * seg + 16].copy()
        if j:
            f, a = (j - 1) // 3, (j - 1) % 3
            s[f] = ACGT[ACGT != s[f]][a]
        for _ in range(c - (1 if locus and j == 0 else 0)):
            pieces += [N1, s, N1, ACGT[rng.integers(0, 4, 282)]]
    if locus:
        pieces += [N1, read, N1, ACGT[rng.integers(0, 4, 282)]]
    return read.tobytes()


def tail_spec(tail):
    """records of 2, 3, 4 and 99 positions and one more, `tail` 4th-and-later positions together"""
    n99 = (tail - 2) // 96
    rest = tail - 1 - 96 * n99
    assert 1 <= rest <= 95
    return [2, 3, 4] + [99] * n99 + [rest + 3]


TAILS = (DEPTH * 64 - 1, DEPTH * 64, DEPTH * 64 + 1, 3 * DEPTH * 64 + 5)
RECORDS = (128, 129, 256, 257)
LIMIT_SPEC = [99] * 56 + [2] * 73


@functools.lru_cache(maxsize=None)
def tails_genome():
    """-> (index, {(tail, locus): read})"""
    rng = np.random.default_rng(5120)
    pieces, reads = [ACGT[rng.integers(0, 4, 500)]], {}
    for t in TAILS:
        for locus in (False, True):
            reads[(t, locus)] = plant(rng, pieces, tail_spec(t), locus)
    ix = _index(np.concatenate(pieces))
    return ix, reads, _sizes(ix)


@functools.lru_cache(maxsize=None)
def headers_genome():
    """-> (index, {records: read, "limit": read}): every tenth record has 5 positions (a tail of 2), the others 2; the ends map"""
    rng = np.random.default_rng(1280)
    pieces, reads = [ACGT[rng.integers(0, 4, 500)]], {}
    for n in RECORDS:
        reads[n] = plant(rng, pieces, [5 if k % 10 == 9 else 2 for k in range(n)], True)
    reads["limit"] = plant(rng, pieces, LIMIT_SPEC, False)
    ix = _index(np.concatenate(pieces))
    return ix, reads, _sizes(ix)


@functools.lru_cache(maxsize=None)
def handout_genome():
    """-> (index, 4 x 304 + 3 distinct 64-base ends, the positions of each): ends cut 96 bases apart from a random genome"""
    rng = np.random.default_rng(640)
    g = ACGT[rng.integers(0, 4, 150000)]
    ix = _index(g)
    size = _sizes(ix)
    third = len(g) // 3                     # (_index cuts the genome into three contigs: no end across a cut)
    reads = [g[s:s + 64].tobytes() for s in range(1000, len(g) - 1000, 96) if s % third < third - 100][:4 * 304 + 3]
    assert len(set(reads)) == len(reads)
    return ix, reads, [sum(buckets_of(size, r)) for r in reads]


def run(ix, reads, mp, first_tier, tier2_waves=None):
    """-> (stats, device n_hits, device results, oracle n_hits, oracle results) of `reads` mapped as single ends"""
    from pecaller_amd import PemapDev
    b, l = refio.pack_reads(reads)
    o = oracle_py.Oracle(ix, paired=False, min_align=0.85)
    m1, _, mt, d1, _ = o.map_batch(b, l, debug=True, threads=4)
    if first_tier:
        mp.delenv("PEMAP_FIRST_TIER", raising=False)
    else:
        mp.setenv("PEMAP_FIRST_TIER", "0")
    if tier2_waves is None:
        mp.delenv("PEMAP_TIER2_WAVES", raising=False)
    else:
        mp.setenv("PEMAP_TIER2_WAVES", str(tier2_waves))
    dev = PemapDev(0)                       # (the knobs are read once per object)
    try:
        dev.build_index(ix["genome"], ix["contig_len"])
        assert dev.lookup_replicas()[0] == 8
        dev.set_params(paired=False, min_dist=0, max_dist=500, min_align=0.85)
        g1, _, gt = dev.map_batch(b, l, None, None)
        stats, _ = dev.run_stats()
        dbg = dev.debug_hits(len(reads))
    finally:
        dev.close()
    print(stats["positions"], stats["big_ends"], stats["mono_ends"], int(dbg["n_hits"].sum()))
    return stats, dbg["n_hits"], (g1, gt), d1["n_hits"], (m1, mt)


def test_the_planted_ends_hold_what_they_say():
    """(no device) tails, records and positions of the planted ends, counted from the index; which of them map"""
    ix, reads, size = tails_genome()
    for (t, locus), r in reads.items():
        bk = buckets_of(size, r)
        recs = [c for c in bk if c >= 2]
        assert sum(c - 3 for c in recs if c > 3) == t and len(recs) <= 128, (t, locus)
        assert sorted(recs) == sorted(tail_spec(t)), (t, locus)
        assert len(recs) >= LEN // 16 and sum(bk) - sum(recs) <= 2      # (every own k-mer is a record; a stray bucket of one position may join)
    assert [sum(tail_spec(t)) <= KCAP1 for t in TAILS] == [True, True, True, False]
    b, l = refio.pack_reads([reads[(t, locus)] for t in TAILS for locus in (False, True)])
    m1 = oracle_py.Oracle(ix, paired=False, min_align=0.85).map_batch(b, l, threads=4)[0]
    assert [bool(m > 0) for m in m1] == [False, True] * len(TAILS)
    ix, reads, size = headers_genome()
    for n in RECORDS:
        bk = buckets_of(size, reads[n])
        assert sum(1 for c in bk if c >= 2) == n and sum(bk) <= KCAP1
    bk = buckets_of(size, reads["limit"])
    recs = sorted(c for c in bk if c >= 2)
    assert recs == sorted(LIMIT_SPEC) and sum(bk) == 5690 <= KCAP2
    assert sum(bk) - max(recs) > KCAP2 - len(recs)
    b, l = refio.pack_reads([reads[n] for n in RECORDS])
    assert (oracle_py.Oracle(ix, paired=False, min_align=0.85).map_batch(b, l, threads=4)[0] > 0).all()


@pytest.mark.parametrize("n_of_grid", [lambda g: 1, lambda g: g - 1, lambda g: g, lambda g: g + 1, lambda g: 4 * g + 3],
                         ids=["one", "grid-1", "grid", "grid+1", "4grid+3"])
def test_hand_out_one_end_per_fetch(n_of_grid, monkeypatch):
    """every end exactly once: N ends over a grid of one second-tier wave per CU"""
    import torch
    grid = torch.cuda.get_device_properties(0).multi_processor_count
    ix, reads, npos = handout_genome()
    n = n_of_grid(grid)
    assert 1 <= n <= len(reads), "the planted ends suffice for 4 grid + 3"
    stats, nh, got, onh, exp = run(ix, reads[:n], monkeypatch, first_tier=False, tier2_waves=1)
    assert stats["ends"] == n and stats["big_ends"] == n and stats["mono_ends"] == 0, stats
    assert stats["positions"] == sum(npos[:n]), stats
    assert np.array_equal(nh, onh)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert (exp[0] > 0).all() and len(set(int(x) for x in exp[0])) == n         # distinct ends, distinct places


@pytest.mark.parametrize("tier", [1, 2], ids=["first_tier", "second_tier"])
def test_tails_at_the_depth_of_a_trip(tier, monkeypatch):
    """the eight ends of `tails_genome` in one batch, one wave each: tails of 511, 512, 513 and 1,541 elements, among islands
    only and with a true locus"""
    ix, reads, size = tails_genome()
    keys = [(t, locus) for t in TAILS for locus in (False, True)]
    npos = [sum(buckets_of(size, reads[k])) for k in keys]
    stats, nh, got, onh, exp = run(ix, [reads[k] for k in keys], monkeypatch, first_tier=(tier == 1))
    # the first tier keeps an end of at most 1,424 positions; the two of 1,600 it passes on, as PEMAP_FIRST_TIER=0 passes every end
    assert stats["big_ends"] == (len(keys) if tier == 2 else sum(n > KCAP1 for n in npos)) and stats["mono_ends"] == 0, stats
    assert stats["positions"] == sum(npos), stats
    assert np.array_equal(nh, onh)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert [bool(m > 0) for m in exp[0]] == [locus for _, locus in keys]


@pytest.mark.parametrize("tier", [1, 2], ids=["first_tier", "second_tier"])
def test_header_rounds(tier, monkeypatch):
    """ends of 128, 129, 256 and 257 records in one batch: one round, one round and a record, two rounds, two and a record"""
    ix, reads, size = headers_genome()
    rs = [reads[n] for n in RECORDS]
    stats, nh, got, onh, exp = run(ix, rs, monkeypatch, first_tier=(tier == 1))
    assert stats["big_ends"] == (len(rs) if tier == 2 else 0) and stats["mono_ends"] == 0, stats
    assert stats["positions"] == sum(sum(buckets_of(size, r)) for r in rs), stats
    assert np.array_equal(nh, onh)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert (exp[0] > 0).all()


def test_the_front_stops_below_the_records_of_later_rounds(monkeypatch):
    """the `limit` rule (module docstring): 5,690 positions fit the second tier's list, 129 records make it two rounds, and the
    first round's positions pass KCAP - nm: the end goes on to pm_seed_kernel, as it always did"""
    ix, reads, _ = headers_genome()
    stats, nh, got, onh, exp = run(ix, [reads["limit"]], monkeypatch, first_tier=True)
    assert stats["big_ends"] == 1 and stats["mono_ends"] == 1, stats
    assert np.array_equal(nh, onh)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
