"""Genomes at the top of the u32 coordinate range (checker side, CPU only): a filler contig of F letters N in front of a small genome
puts the small genome's positions at F .. F + g.  Two placements: `straddle`, real position 2^31 in the middle of the middle
contig, and `top`, the largest genome pemap_dev_index_alloc accepts (2^32 - 401 letters), where the look-up replicas' record codes
(entries >= genome size and < 0xFFFFFFFE, pemap_aux.hip.h) have 398 units of room.  The filler is never indexed: it holds no
16-mer free of N, so the small genome's index shifted by F - 15 compressed coordinates is the whole genome's."""
import numpy as np

import refio

HALF = 1 << 31
LARGEST = (1 << 32) - 401          # pemap_dev_index_alloc refuses genome_size >= 2^32 - 400
CODES = 0xFFFFFFFE                 # record codes end below the "too many" marker
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[:] = ord("N")
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b


def high_index(contigs, F, bisulfite=False):
    """the index dict that oracle_py.Oracle and PemapDev.build_index take, of [F x N] + contigs"""
    assert len(contigs) >= 7 and F >= 16          # (the oracle's find_chrom: parity for 1 or at least 8 contigs)
    mers, ukmer, ustart, cs = refio.kmer_index(contigs, bisulfite=bisulfite)
    g = int(sum(len(c) for c in contigs))
    assert F + g <= LARGEST
    genome = np.full(F + g, ord("N"), np.uint8)
    genome[F:] = np.concatenate(contigs)
    shift = F - 15                                # the filler's length in compressed coordinates
    return dict(mers=(mers.astype(np.uint64) + shift).astype(np.uint32), ukmer=ukmer, ustart=ustart, genome=genome,
                contig_starts=np.concatenate([[0], cs.astype(np.uint64) + shift]).astype(np.uint32),
                contig_len=np.array([F] + [len(c) for c in contigs], dtype=np.uint32), F=F, g=g)


def low_index(contigs, bisulfite=False):
    mers, ukmer, ustart, cs = refio.kmer_index(contigs, bisulfite=bisulfite)
    return dict(mers=mers, ukmer=ukmer, ustart=ustart, genome=np.concatenate(contigs), contig_starts=cs,
                contig_len=np.array([len(c) for c in contigs], dtype=np.uint32))


def mid_contig(contigs):
    """(contig, its offset in the small genome, the offset inside it that `straddle` puts at 2^31)"""
    k = len(contigs) // 2
    return contigs[k], int(sum(len(c) for c in contigs[:k])), len(contigs[k]) // 2


def straddle(contigs):
    _, start, B = mid_contig(contigs)
    return HALF - start - B


def top(contigs):
    return LARGEST - int(sum(len(c) for c in contigs))


def units(index):
    """ix_rep_units_kernel restated: 16-byte units of the records, (ln + 4) // 4 over the buckets of 2 .. 99 positions; the all-T
    k-mer's length is get_mers' wrapped pos_index[0] - pos_index[0xFFFFFFFF]"""
    us = index["ustart"].astype(np.int64)
    ln = np.diff(us)
    if len(ln) and int(index["ukmer"][-1]) == 0xFFFFFFFF:
        ln[-1] = (0 - us[-2]) & 0xFFFFFFFF
    ln = ln[(ln >= 2) & (ln < 100)]
    return int(((ln + 4) // 4).sum())


def record_codes(index, multi_base):
    """(k-mers with a record, their replica entries, units of each) as ix_rep_encode_kernel lays them out: records in k-mer order"""
    us = index["ustart"].astype(np.int64)
    ln = np.diff(us)
    if len(ln) and int(index["ukmer"][-1]) == 0xFFFFFFFF:
        ln[-1] = (0 - us[-2]) & 0xFFFFFFFF
    sel = (ln >= 2) & (ln < 100)
    u = (ln[sel] + 4) // 4
    return index["ukmer"][sel], multi_base + np.concatenate([[0], np.cumsum(u)[:-1]]), u


def _substitute(x, rng, rate=0.01):
    m = rng.random(len(x)) < rate
    x[m] = ACGT[rng.integers(0, 4, int(m.sum()))]


def _pair(c, s, fl, la, lb, rng):
    a = c[s:s + la].copy()
    b = COMP[c[s + fl - lb:s + fl]][::-1].copy()
    _substitute(a, rng)
    _substitute(b, rng)
    if rng.random() < 0.5:
        a, b = b, a
    return a.tobytes(), b.tobytes()


def boundary_pairs(contig, B, n, lo, hi, seed=0):
    """pairs whose fragment covers offsets B - 1 and B of the contig: 1 % substitutions, mates swapped at random"""
    rng = np.random.default_rng(seed)
    r1, r2 = [], []
    for _ in range(n):
        la, lb = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
        fl = int(rng.integers(max(la, lb) + 20, 481))
        s = int(rng.integers(B - fl + 1, B))
        assert 0 <= s < B < s + fl <= len(contig)
        a, b = _pair(contig, s, fl, la, lb, rng)
        r1.append(a)
        r2.append(b)
    return refio.pack_reads(r1) + refio.pack_reads(r2)


def edge_pairs(contigs, reps=4, lo=100, hi=200, seed=0):
    """fragments that start at offsets 0 .. 8 of the first contig (the window of the end that lies there is clipped against the
    filler's end) and fragments that end at the last 0 .. 8 bases of the last contig (on `top` the end of the largest genome)"""
    rng = np.random.default_rng(seed)
    r1, r2 = [], []
    for rep in range(reps):
        for off in range(9):
            for first in (True, False):
                c = contigs[0] if first else contigs[-1]
                la, lb = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
                fl = int(rng.integers(max(la, lb) + 20, 481))
                s = off if first else len(c) - fl - off
                a, b = _pair(c, s, fl, la, lb, rng)
                r1.append(a)
                r2.append(b)
    return refio.pack_reads(r1) + refio.pack_reads(r2)


def join(*sets):
    """read sets (rows1, len1, rows2, len2) one behind the other"""
    return tuple(np.concatenate([s[k] for s in sets]) for k in range(4))


def around(gen, contig, B, *args):
    """`gen`'s reads from the 4,000 letters of the contig around offset B alone (gen takes contigs and is position-free): the
    fragments that its repeat-seeking branch draws start 100 .. 200 letters before B and nearly all of them cover it"""
    return gen([contig[B - 1700:B + 2300]], *args)


def sides(m):
    """mapped coordinates (position + 1, 0 = unmapped) -> (number below position 2^31, number at or above it)"""
    p = m[m > 0].astype(np.int64) - 1
    return int((p < HALF).sum()), int((p >= HALF).sum())


# ---- test 6: a genome whose records fill the code space of the `top` placement exactly, and one unit more
def code_space_genome(target, seed=5):
    """ten random contigs of 50 kb with 16-mers copied into them until units() == target -> (contigs, sites): sites are the
    (contig, offset) of every 16-mer that has a copy, source and copy alike"""
    rng = np.random.default_rng(seed)
    contigs = [ACGT[rng.integers(0, 4, 50000)].copy() for _ in range(10)]
    have = units(low_index(contigs))
    assert have <= target
    sites = []
    slot = 0                     # plantings go to slots of 200 letters, so that no copy overwrites another or a source
    while have < target:
        # most of the way in one step, the rest one copy at a time; a step that overshoots is undone and halved
        step = max(1, (target - have) * 9 // 10)
        while True:
            saved = [c.copy() for c in contigs]
            new = []
            for j in range(step):
                c, o = (slot + j) % 10, 1000 + 200 * ((slot + j) // 10)
                sc, so = int(rng.integers(0, 10)), 100 + 200 * int(rng.integers(0, 240))      # a source in the middle of a slot
                contigs[c][o:o + 16] = contigs[sc][so:so + 16]
                new += [(c, o), (sc, so)]
            now = units(low_index(contigs))
            if now <= target:
                slot += step
                have = now
                sites += new
                break
            contigs = saved
            if step == 1:
                slot += 1        # this very copy adds more than one unit: another one
            step = max(1, step // 2)
    assert units(low_index(contigs)) == target
    return contigs, sites


def site_pairs(contigs, sites, n, L=150, seed=0):
    """pairs with one end that hangs on a planted 16-mer (all sites in turn): segment j of its ten (cut at 0, 16 .. 128 and L - 16,
    initial_map) is the site's 16-mer, three more of segments 0 .. 7 are intact, and every other segment carries two substitutions,
    beyond the single one the neighbour look-ups forgive.  A hit needs four segments on one diagonal: the end maps only through the
    position that the look-up of the planted 16-mer's bucket -- two or more positions, a record -- returns.  The mate has 1 % of
    substitutions; the site's end is the fragment's first or, read on the other strand, its far end."""
    assert L == 150
    rng = np.random.default_rng(seed)
    r1, r2 = [], []
    for k in range(n):
        ci, o = sites[k % len(sites)]
        c = contigs[ci]
        fl = int(rng.integers(L + 20, 481))
        j = int(rng.integers(0, min(8, o // 16 + 1)))
        lo = o - 16 * j
        far = k % 2 == 1 and lo - (fl - L) >= 0
        s = lo - (fl - L) if far else lo
        assert 0 <= s and s + fl <= len(c)
        x = c[lo:lo + L].copy()
        keep = {j} | set(int(q) for q in rng.choice([q for q in range(8) if q != j], 3, replace=False))
        spans = [(16 * q, 16 * q + 16) for q in range(8) if q not in keep] + [(134, 144)]      # (134 .. 143: segments 8 and 9 both)
        for a0, a1 in spans:
            for q in rng.choice(np.arange(a0, a1), 2, replace=False):
                x[q] = ACGT[(b"ACGT".index(x[q]) + int(rng.integers(1, 4))) % 4]
        if far:
            y = c[s:s + L].copy()
            _substitute(y, rng)
            a, b = y, COMP[x][::-1].copy()
        else:
            y = COMP[c[s + fl - L:s + fl]][::-1].copy()
            _substitute(y, rng)
            a, b = x, y
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a.tobytes())
        r2.append(b.tobytes())
    return refio.pack_reads(r1) + refio.pack_reads(r2)


# ---- the read sets of test_gpu_high_coords.py, (name, paired, (rows1, len1, rows2, len2)); test_high_coords_cpu.py holds their
# conditions on the oracle alone
def adversarial_contigs():
    from test_gpu_edge import _adversarial_genome
    contigs = _adversarial_genome(78)
    for c in contigs[:3]:          # the planted reference Ns of test_banded_dp_on_indels_near_read_ends
        c[np.random.default_rng(len(c)).integers(0, len(c), 300)] = ord("N")
    return contigs


def g1_sets(contigs, which=("r150", "r100", "b150", "b16_278", "edge")):
    import fixtures
    c, _, B = mid_contig(contigs)
    make = dict(r150=lambda: (True, tuple(x[:3000] for x in fixtures.reads("r150"))),
                r100=lambda: (False, tuple(x[:3000] for x in fixtures.reads("r100")[:2]) + (None, None)),
                b150=lambda: (True, boundary_pairs(c, B, 400, 150, 150, seed=150)),
                b16_278=lambda: (True, boundary_pairs(c, B, 400, 16, 278, seed=16)),
                edge=lambda: (True, edge_pairs(contigs)))
    return [(k,) + make[k]() for k in which]


def bisulfite_sets():
    from test_gpu_edge import ragged_reads
    return [("ragged", True, ragged_reads(1250, 2000, 90, 160))]


def adversarial_sets(contigs, n=2000, L=150):
    """the banded DP's and the gapless rule's reads; a tenth and more of the fragments cover the middle contig's middle: 600 of the
    2,000 are drawn from the 4,000 letters around it, of which the branch that starts at offsets 1,500 .. 1,600 nearly always does"""
    from test_gpu_edge import _adversarial_genome, _adversarial_reads, _band_reads
    c, _, B = mid_contig(contigs)
    near = 3 * n // 10
    clean = _adversarial_genome(78)        # _adversarial_reads substitutes A / C / G / T only: it draws from the letters before the Ns
    assert all(len(a) == len(b) for a, b in zip(clean, contigs))
    return [("band", True, join(_band_reads(contigs, 159, n - near, L), around(_band_reads, c, B, 160, near, L))),
            ("adversarial", True, join(_adversarial_reads(clean, 155, n - near, L),
                                        around(_adversarial_reads, mid_contig(clean)[0], B, 156, near, L))),
            ("edge", True, edge_pairs(contigs, seed=3))]


def family_sets(contigs, spots, n=1500, L=150):
    from test_gpu_edge import _family_reads
    return [("family", True, _family_reads(contigs, spots, 99, n, L))]


def code_space_sets(contigs, sites, n=2000, L=150):
    """half over the planted copies, a tenth edge_pairs (the last contig's end is the genome's: single positions just below the
    first record code), the rest boundary-free pairs from anywhere"""
    rng = np.random.default_rng(len(sites))
    r1, r2 = [], []
    e = edge_pairs(contigs, reps=n // 10 // 18 + 1, seed=7)
    e = tuple(x[:n // 10] for x in e)
    for _ in range(n - n // 2 - n // 10):
        c = contigs[int(rng.integers(0, len(contigs)))]
        fl = int(rng.integers(L + 20, 481))
        a, b = _pair(c, int(rng.integers(0, len(c) - fl)), fl, L, L, rng)
        r1.append(a)
        r2.append(b)
    return [("codes", True, join(site_pairs(contigs, sites, n // 2, L, seed=11), e, refio.pack_reads(r1) + refio.pack_reads(r2)))]
