"""The lists of the fused seed kernel hold PM_S4_KCAP = 1,424 positions of both strands of a read-end of up to 160 bases in the first
tier (pemap_seed4.hip.h; 1,536 before) and four times as many, 5,696, in the second (6,144 before); the overflow test is the one in
rec_round: an end whose positions pass the capacity goes to the next tier.  Per tier two ends of 64 bases on a planted genome, one
with exactly the capacity and one with one position more.

Per end four random 16-mers, one per segment, and one-substitution siblings of each, every one planted as an island (N + 16
letters + N, 300 bases apart) fewer than too_many_spots = 100 times.  First tier: 99 + 99 + 99 + 56 copies in buckets that are
records and three siblings planted once (entries that are the bucket's only position), 356 positions a segment; second tier: 14 x 99
+ 36 and two single ones, 1,424 a segment.  All are found on the forward strand through the k-mer's own bucket and its neighbours'.
The second end has one copy more of one sibling.  The islands stand alone, so no two segments meet on a diagonal: no candidate
anchor (min_match is 3), the candidates' capacity plays no part, the ends do not map.  The count is checked on the CPU from the
index (49 buckets per segment and strand, a segment with a bucket of 100 or more dropped); on the device `positions`, `big_ends`
and `mono_ends` of run_stats tell how many positions the end had and which tier took it, and the results are the oracle's."""
import functools

import numpy as np
import pytest

import oracle_py
import refio

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[:] = ord("N")
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
KCAP = {1: 1424, 2: 4 * 1424}               # the list of the first tier and of the second (PmSeed4Shared < 10, * >::KCAP)
TOO_MANY = 100
# copies of a segment's k-mer and of its siblings, a quarter of the capacity together
COPIES = {1: (99, 99, 99, 56, 1, 1, 1), 2: (99,) * 14 + (36, 1, 1)}
SIB_AT = (1, 4, 6, 9, 12, 14, 0, 2, 3, 5, 7, 8, 10, 11, 13, 15)


@functools.lru_cache(maxsize=None)
def planted(tier):
    """-> (index dict, [read with KCAP[tier] positions, read with one more])"""
    rng = np.random.default_rng(14240 + tier)
    copies = COPIES[tier]
    assert 4 * sum(copies) == KCAP[tier] and max(copies) < TOO_MANY
    pieces, reads = [ACGT[rng.integers(0, 4, 500)]], []
    for extra in (0, 1):
        read = []
        for seg in range(4):
            k = ACGT[rng.integers(0, 4, 16)].copy()
            read.append(k)
            sibs = [k]
            for at in SIB_AT[:len(copies) - 1]:
                s = k.copy()
                s[at] = ACGT[ACGT != s[at]][int(rng.integers(0, 3))]
                sibs.append(s)
            for j, (s, c) in enumerate(zip(sibs, copies)):
                for _ in range(c + (extra if (seg, j) == (2, len(copies) - 3) else 0)):
                    pieces += [np.frombuffer(b"N", np.uint8), s, np.frombuffer(b"N", np.uint8), ACGT[rng.integers(0, 4, 282)]]
        reads.append(np.concatenate(read).tobytes())
    g = np.concatenate(pieces)
    n = len(g) // 3
    contigs = [g[:n], g[n:2 * n], g[2 * n:]]
    mers, ukmer, ustart, cs = refio.kmer_index(contigs)
    ix = dict(mers=mers, ukmer=ukmer, ustart=ustart, genome=g, contig_starts=cs, contig_len=np.array([len(c) for c in contigs], np.uint32),
              names=["b0", "b1", "b2"])
    return ix, reads


def _kmer(x):
    k = 0
    for c in x:
        k = (k << 2) | b"ACGT".index(c)
    return k


def positions_of(read, tier):
    """what the seed stage lists for an end of ACGT letters: per strand and segment the 49 buckets of the k-mer and its
    one-substitution neighbours, none when one of them holds too_many_spots or more"""
    ix = planted(tier)[0]
    size = dict(zip((int(k) for k in ix["ukmer"]), (int(n) for n in np.diff(ix["ustart"].astype(np.int64)))))
    L = len(read)
    cuts = L // 16 - (1 if L % 16 == 0 else 0)
    offs = [16 * i for i in range(cuts)] + [L - 16]
    total = 0
    for strand in (read, COMP[np.frombuffer(read, np.uint8)][::-1].tobytes()):
        for o in offs:
            k = _kmer(strand[o:o + 16])
            nb = [k] + [(k & ~(3 << (2 * f))) | (a << (2 * f)) for f in range(16) for a in range(4) if a != (k >> (2 * f)) & 3]
            assert len(nb) == 49
            sizes = [size.get(x, 0) for x in nb]
            if max(sizes) < TOO_MANY:
                total += sum(sizes)
    return total


@pytest.mark.parametrize("tier", [1, 2])
def test_the_planted_ends_hold_the_capacity_and_one_more(tier):
    """(no device)"""
    reads = planted(tier)[1]
    assert [positions_of(r, tier) for r in reads] == [KCAP[tier], KCAP[tier] + 1]


@pytest.mark.parametrize("which", [0, 1], ids=["capacity", "one_more"])
@pytest.mark.parametrize("tier", [1, 2], ids=["first_tier", "second_tier"])
def test_the_list_takes_its_capacity_and_not_one_more(tier, which):
    """first tier: 1,424 positions stay (big_ends 0), 1,425 go to the second tier (big_ends 1).  Second tier: both ends are passed
    to it; 5,696 positions stay there, 5,697 go on to pm_seed_kernel (`mono_ends` of run_stats counts what the second tier leaves)"""
    from pecaller_amd import PemapDev
    ix, reads = planted(tier)
    b, l = refio.pack_reads([reads[which]])
    o = oracle_py.Oracle(ix, paired=False, min_align=0.85)
    m1, _, mt, d1, _ = o.map_batch(b, l, debug=True, threads=1)
    dev = PemapDev(0)
    try:
        dev.build_index(ix["genome"], ix["contig_len"])
        assert dev.lookup_replicas()[0] == 8
        dev.set_params(paired=False, min_dist=0, max_dist=500, min_align=0.85)
        g1, _, gt = dev.map_batch(b, l, None, None)
        stats, _ = dev.run_stats()
        dbg = dev.debug_hits(1)
    finally:
        dev.close()
    print(stats["positions"], stats["big_ends"], stats["mono_ends"], int(dbg["n_hits"][0]))
    assert stats["ends"] == 1
    if tier == 1:
        assert stats["big_ends"] == which and stats["mono_ends"] == 0, stats
    else:
        assert stats["big_ends"] == 1 and stats["mono_ends"] == which, stats
    if stats["mono_ends"] == 0:         # (the fused kernel's tiers count the positions of the ends they keep)
        assert stats["positions"] == KCAP[tier] + which, stats
    assert np.array_equal(dbg["n_hits"], d1["n_hits"])
    assert np.array_equal(g1, m1) and np.array_equal(gt, mt)
