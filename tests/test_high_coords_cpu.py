"""What test_gpu_high_coords.py expects, checked on the oracle alone (CPU only).  The oracle on a genome placed behind a filler of F
letters N gives the low-coordinate run's results shifted by F -- and test_oracle_golden.py pins the low run to the files the
unmodified reference printed, so the expectations at coordinates above 2^31 hang on the reference by that chain.  Then the
conditions on the read sets (properties of the inputs, not measurements of the code under test): on `straddle` a quarter of the
mapped ends on either side of position 2^31, the boundary pairs with their mates on two sides of it and every pileup row around it
touched, on `top` every coordinate in the last g + 401 of the u32 range; and units() against a brute-force count."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fixtures
import high_cases as hc
import oracle_py

PARAMS = dict(min_dist=0, max_dist=500, min_align=0.85)


def _oracle(ix, paired, reads, bis=False):
    o = oracle_py.Oracle(ix, paired=paired, bisulfite=bis, **PARAMS)
    m1, m2, mt, _, _ = o.map_batch(*reads, threads=8)
    return o, m1, m2, mt


def _shift(m, F):
    return np.where(m > 0, (m.astype(np.uint64) + F).astype(np.uint32), np.uint32(0))


def _any_counts(counts, lo, hi):
    """whether a counter of rows lo .. hi is non-zero (the oracle's array is calloc'ed: rows never written stay unbacked, and reading
    them costs page faults, not memory; eight threads take them side by side)"""
    step = 1 << 26
    with ThreadPoolExecutor(8) as ex:
        return any(ex.map(lambda a: bool(counts[a:min(a + step, hi)].any()), range(lo, hi, step)))


@functools.lru_cache(maxsize=None)
def _low_r150():
    r = tuple(x[:3000] for x in fixtures.reads("r150"))
    o, m1, m2, mt = _oracle(fixtures.index(), True, r)
    return dict(m1=m1, m2=m2, mt=mt, counts=o.counts().copy(), ins=o.insertions(), summary=o.summary())


@pytest.mark.parametrize("placement", ["straddle", "top"])
def test_high_run_is_the_low_run_shifted(placement):
    """g1, the first 3,000 r150 pairs: coordinates plus F where non-zero, same classes and summary, the pileup rows F .. F + g equal
    to the low run's and no counter outside them, insertions shifted by F"""
    _, contigs = fixtures.genome()
    F = getattr(hc, placement)(contigs)
    ix = hc.high_index(contigs, F)
    g = ix["g"]
    low = _low_r150()
    o, m1, m2, mt = _oracle(ix, True, tuple(x[:3000] for x in fixtures.reads("r150")))
    assert np.array_equal(m1, _shift(low["m1"], F)) and np.array_equal(m2, _shift(low["m2"], F))
    assert np.array_equal(mt, low["mt"])
    assert np.array_equal(o.summary(), low["summary"])
    counts = o.counts()
    assert counts.shape == (F + g, 6)
    assert np.array_equal(counts[F:F + g], low["counts"])
    assert not _any_counts(counts, 0, F)
    assert o.insertions() == [(p + F, s) for p, s in low["ins"]] and len(low["ins"]) > 0
    # the conditions of this read set
    mapped = int((m1 > 0).sum())
    below, above = hc.sides(np.concatenate([m1, m2]))
    print(placement, "F", F, "mapped pairs' first ends", mapped, "ends below / at or above 2^31", below, above)
    assert mapped >= 2700                                   # 90 % of the 3,000
    if placement == "straddle":
        assert 4 * below >= below + above and 4 * above >= below + above
        assert F + hc.mid_contig(contigs)[1] + hc.mid_contig(contigs)[2] == hc.HALF
    else:
        assert F + g == (1 << 32) - 401 and below == 0
        both = np.concatenate([m1, m2])
        assert int(both[both > 0].min()) - 1 > (1 << 32) - g - 401


def test_straddle_read_sets_on_g1():
    """r100 single-end and the edge pairs: a quarter of the mapped ends on either side.  The boundary pairs, 400 of 150 bases and 400
    of 16 .. 278: at least 100 pairs with their mates on two sides of position 2^31 (a pair's later end lies at or above it in about
    half of them, so these sets hold fewer than a quarter of their ends below: the two-sided count is their condition), nearly all
    mapped as pairs, and together with their mates' every pileup row of [2^31 - 300, 2^31 + 300) touched."""
    _, contigs = fixtures.genome()
    ix = hc.high_index(contigs, hc.straddle(contigs))
    for name, paired, reads in hc.g1_sets(contigs, ("r100", "b150", "b16_278", "edge")):
        o, m1, m2, mt = _oracle(ix, paired, reads)
        ends = np.concatenate([m1, m2]) if paired else m1
        below, above = hc.sides(ends)
        print(name, "ends", len(ends), "below / at or above", below, above)
        if name in ("b150", "b16_278"):
            both = (m1 > 0) & (m2 > 0)
            two = both & ((m1.astype(np.int64) - 1 < hc.HALF) != (m2.astype(np.int64) - 1 < hc.HALF))
            rows = o.counts()[hc.HALF - 300:hc.HALF + 300].astype(np.int64).sum(axis=1)
            print(name, "pairs", int(both.sum()), "two-sided", int(two.sum()), "rows touched", int((rows > 0).sum()))
            assert int(both.sum()) >= 390 and int(two.sum()) >= 100
            assert (rows > 0).all()
        else:
            assert 4 * below >= below + above and 4 * above >= below + above and below + above >= len(ends) * 2 // 5
        del o


def _quarter(name, m1, m2, floor):
    below, above = hc.sides(np.concatenate([m1, m2]))
    print(name, "ends", 2 * len(m1), "below / at or above", below, above)
    assert 4 * below >= below + above and 4 * above >= below + above and below + above >= floor, (name, below, above)


def test_straddle_read_sets_on_the_other_genomes():
    """bisulfite g1 with the ragged pairs; the adversarial genome with the band's and the gapless rule's reads, of which a tenth of
    the fragments cover position 2^31 (counted as pairs with one end mapped on either side, or an end that begins within a read
    length below it), and with edge pairs whose windows really are clipped (g1's contigs begin and end in runs of N: its edge
    pairs map by the inner end alone); the repeat family"""
    from test_gpu_edge import _repeat_family_genome
    _, contigs = fixtures.genome()
    ix = hc.high_index(contigs, hc.straddle(contigs), bisulfite=True)
    for name, paired, reads in hc.bisulfite_sets():
        o, m1, m2, mt = _oracle(ix, paired, reads, bis=True)
        _quarter(name, m1, m2, len(m1))
    del o, ix
    contigs = hc.adversarial_contigs()
    ix = hc.high_index(contigs, hc.straddle(contigs))
    for name, paired, reads in hc.adversarial_sets(contigs):
        o = oracle_py.Oracle(ix, paired=True, **PARAMS)
        m1, m2, mt, d1, d2 = o.map_batch(*reads, debug=True, threads=8)
        _quarter(name, m1, m2, len(m1))
        if name == "edge":
            clipped = sum(int((d["win_len"][i, :d["n_hits"][i]] < reads[2 * k + 1][i] + 21).sum())
                          for k, d in enumerate((d1, d2)) for i in range(len(m1)))
            print(name, "clipped windows", clipped, "classes", np.bincount(mt, minlength=9))
            assert clipped >= len(m1) * 3 // 4 and ((m1 > 0) & (m2 > 0)).sum() >= len(m1) * 3 // 4
        else:
            p1, p2 = m1.astype(np.int64) - 1, m2.astype(np.int64) - 1
            cover = ((m1 > 0) & (m2 > 0) & ((p1 < hc.HALF) != (p2 < hc.HALF))) | ((m1 > 0) & (abs(p1 - hc.HALF) < 150)) \
                | ((m2 > 0) & (abs(p2 - hc.HALF) < 150))
            print(name, "fragments over 2^31", int(cover.sum()))
            assert int(cover.sum()) >= len(m1) // 10
        del o
    del ix
    contigs, spots = _repeat_family_genome(4242)
    ix = hc.high_index(contigs, hc.straddle(contigs))
    for name, paired, reads in hc.family_sets(contigs, spots):
        o, m1, m2, mt = _oracle(ix, paired, reads)
        _quarter(name, m1, m2, len(m1))


def test_units_against_a_brute_force_count():
    """units() on a small index with buckets of 1, 2, 3, 4, 5, 99 and 100 positions and the all-T k-mer (whose length get_mers
    computes with a wrapped `which + 1`: never a record), against a dictionary of every 16-mer"""
    rng = np.random.default_rng(8)
    contigs = [hc.ACGT[rng.integers(0, 4, 6000)].copy() for _ in range(7)]
    mer = [hc.ACGT[rng.integers(0, 4, 16)] for _ in range(7)]
    at = 40
    for m, copies in zip(mer, (2, 3, 4, 5, 99, 100, 7)):
        for _ in range(copies):
            contigs[at // 5000][at % 5000:at % 5000 + 16] = m
            at += 40
    contigs[6][5000:5040] = ord("T")            # 25 positions in k-mer 0xFFFFFFFF
    code = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
    seen = {}
    for c in contigs:
        s = bytes(c)
        for i in range(len(s) - 15):
            w = s[i:i + 16]
            if b"N" not in w:
                k = 0
                for ch in w:
                    k = k * 4 + code[ch]
                seen[k] = seen.get(k, 0) + 1
    assert seen[0xFFFFFFFF] == 25
    brute = sum((n + 4) // 4 for k, n in seen.items() if 2 <= n < 100 and k != 0xFFFFFFFF)
    sizes = sorted(n for n in seen.values() if n > 1)
    assert [n for n in (2, 3, 4, 5, 7, 99, 100) if n in sizes] == [2, 3, 4, 5, 7, 99, 100], sizes
    ix = hc.low_index(contigs)
    assert hc.units(ix) == brute
    kmers, codes, u = hc.record_codes(ix, 1000)
    assert int(u.sum()) == brute and codes[0] == 1000 and int(codes[-1] + u[-1]) == 1000 + brute and 0xFFFFFFFF not in kmers


def test_code_space_genomes_hold_398_and_399_units():
    """the two genomes of the `top` placement's code-space test: exactly as many record units as fit the codes between the largest
    genome's size and 0xFFFFFFFE, and one more; every planted site holds a 16-mer with a bucket of at least two"""
    room = hc.CODES - hc.LARGEST - 1
    assert room == 398          # units < 0xFFFFFFFE - gsize
    for target in (room, room + 1):
        contigs, sites = hc.code_space_genome(target)
        ix = hc.low_index(contigs)
        assert hc.units(ix) == target and len(ix["genome"]) == 500000
        sizes = dict(zip(ix["ukmer"].tolist(), np.diff(ix["ustart"].astype(np.int64)).tolist()))
        for c, o in sites:
            k = 0
            for ch in contigs[c][o:o + 16]:
                k = k * 4 + b"ACGT".index(ch)
            assert sizes[k] >= 2
        kmers, codes, u = hc.record_codes(ix, hc.LARGEST)
        assert int(codes[-1] + u[-1]) - 1 == 0xFFFFFFFC + (target - room)
        # the site pairs hang on the records: every site end has a hit, and none once the buckets of 2 .. 99 positions are taken out
        # of the index (what a look-up that misreads a record amounts to)
        reads = hc.site_pairs(contigs, sites, 1000)
        us = ix["ustart"].astype(np.int64)
        ln = np.diff(us)
        keep = ~((ln >= 2) & (ln < 100))
        cut = dict(ix, mers=np.concatenate([ix["mers"][us[i]:us[i + 1]] for i in np.nonzero(keep)[0]]), ukmer=ix["ukmer"][keep],
                   ustart=np.concatenate([[0], np.cumsum(ln[keep])]).astype(np.uint32))
        for index, without in ((ix, 0), (cut, 1000)):
            o = oracle_py.Oracle(index, paired=True, **PARAMS)
            _, _, _, d1, d2 = o.map_batch(*reads, debug=True, threads=8)
            assert int((d1["n_hits"] == 0).sum() + (d2["n_hits"] == 0).sum()) == without
