"""The seed kernel's hit list (pemap_seed4.hip.h): the first tier for reads of up to 160 bases keeps the first NKEEP = 76 hits of an end
in the back of the vote's tables until the next iteration writes them out; an end with more tied hits stores the rest at the end of
its walk.  The walk stops at PM_MAX_HITS = 200 in every tier.

A planted genome in the style of the ladder's islands: per case one random 16-mer and two one-substitution siblings of it, each
planted fewer than too_many_spots = 100 times (N + 16 letters + N), T copies together.  The read is the 16-mer and 16 random
letters behind it: two segments, the second without a position (a strand whose segments ALL hold more than PM_MAX_HITS positions is
not searched, pemapper.c:2200-2207), min_match 1, so every copy -- found through the k-mer's own bucket or a neighbour's -- is a
tied hit, one position each.  An end
reaches the first tier's walk with up to RCAP = 160 positions next to candidates, so T = 75, 76, 77 and 150 are served by the first
tier (big_ends == 0 is asserted); 199, 200 and 230 pass to the second tier, whose tables hold all PM_MAX_HITS hits (no hit beyond
NKEEP there).  So the first tier's path for the hits beyond NKEEP is run with up to 150 hits, and RCAP makes more than 160
unreachable in it.  Reads of 32 bases, not 64: a hit of a 64-base end takes three or four of the RCAP positions (min_match 3), which
ends the first tier at 40 to 53 tied hits, below NKEEP.  Expectation: the oracle's hit lists in order, n_hits, coordinates."""
import functools

import numpy as np
import pytest

import oracle_py
import refio

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", np.uint8)
NKEEP = 76
FIRST_TIER = (NKEEP - 1, NKEEP, NKEEP + 1, 150)
SECOND_TIER = (199, 200, 230)
TOO_MANY = 100


@functools.lru_cache(maxsize=None)
def planted():
    """-> (index dict, {T: 16-mer}): contigs of random letters with the copies 300 bases apart"""
    rng = np.random.default_rng(1376)
    pieces, kmers = [ACGT[rng.integers(0, 4, 500)]], {}
    for T in FIRST_TIER + SECOND_TIER:
        k = ACGT[rng.integers(0, 4, 16)].copy()
        kmers[T] = k.tobytes()
        sibs = [k]
        for at in (5, 11):
            s = k.copy()
            s[at] = ACGT[ACGT != s[at]][0]
            sibs.append(s)
        left = T
        for s in sibs:
            c = min(left, TOO_MANY - 1)
            left -= c
            for _ in range(c):
                pieces += [np.frombuffer(b"N", np.uint8), s, np.frombuffer(b"N", np.uint8), ACGT[rng.integers(0, 4, 282)]]
        assert left == 0
    g = np.concatenate(pieces)
    n = len(g) // 3
    contigs = [g[:n], g[n:2 * n], g[2 * n:]]
    mers, ukmer, ustart, cs = refio.kmer_index(contigs)
    ix = dict(mers=mers, ukmer=ukmer, ustart=ustart, genome=g, contig_starts=cs, contig_len=np.array([len(c) for c in contigs], np.uint32),
              names=["p0", "p1", "p2"])
    return ix, kmers


@functools.lru_cache(maxsize=None)
def expected(cases):
    ix, kmers = planted()
    rng = np.random.default_rng(77)
    b, l = refio.pack_reads([kmers[T] + ACGT[rng.integers(0, 4, 16)].tobytes() for T in cases])
    o = oracle_py.Oracle(ix, paired=False, min_align=0.85)
    m1, _, mt, d1, _ = o.map_batch(b, l, debug=True, threads=2)
    return b, l, m1, mt, d1


def test_the_oracle_finds_the_planted_counts():
    """(no device) T tied hits for T <= 200, 200 beyond"""
    for cases in (FIRST_TIER, SECOND_TIER):
        d1 = expected(cases)[4]
        assert [int(x) for x in d1["n_hits"]] == [min(T, 200) for T in cases]


@pytest.mark.parametrize("cases", [FIRST_TIER, SECOND_TIER], ids=["first_tier", "second_tier"])
def test_hit_lists_in_order(cases):
    from pecaller_amd import PemapDev
    ix = planted()[0]
    b, l, m1, mt, d1 = expected(cases)
    n = len(l)
    dev = PemapDev(0)
    try:
        dev.build_index(ix["genome"], ix["contig_len"])
        assert dev.lookup_replicas()[0] == 8
        dev.set_params(paired=False, min_dist=0, max_dist=500, min_align=0.85)
        g1, _, gt = dev.map_batch(b, l, None, None)
        stats, _ = dev.run_stats()
        dbg = dev.debug_hits(n)
    finally:
        dev.close()
    print(stats["big_ends"], list(dbg["n_hits"]))
    assert np.array_equal(dbg["n_hits"], d1["n_hits"])
    for i in range(n):
        k = int(d1["n_hits"][i])
        assert np.array_equal(dbg["spot"][i, :k], d1["spot"][i, :k]), (cases[i], np.nonzero(dbg["spot"][i, :k] != d1["spot"][i, :k])[0][:5])
        assert np.array_equal(dbg["orient"][i, :k], d1["orient"][i, :k]), cases[i]
    assert np.array_equal(g1, m1) and np.array_equal(gt, mt)
    assert stats["ends"] == n
    if cases is FIRST_TIER:
        assert stats["big_ends"] == 0, stats
    else:
        assert stats["big_ends"] == n, stats
