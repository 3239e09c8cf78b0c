"""The fused seed kernel's look-ups, one neighbour at a time (pemap_seed4.hip.h: lane j of a wave holds the table entry of neighbour j
of a segment's k-mer, requested by the lane itself; pemap_seed_entry.h is the address).  Reads that map only if ONE particular entry
is read correctly, in every form of the kernel.

A small genome of random letters holds, per read length, two planted units a few hundred bases apart (a pair's first end is read
from the first on the forward strand, its second end from the second on the reverse strand).  A read is a copy of its unit in which
exactly min_match segments can seed (pemapper.c:1642-1645: 3 of the 4 segments of 64 bases, 4 of the 10 / 16 / 17 of 150 / 245 / 270):
one of them -- the target -- carries a single substitution at base b to alternative a inside its 16-mer, so that it is found only
through the neighbour look-up that puts the unit's letter back; min_match - 1 are exact; every other segment is spoiled by two
substitutions inside its 16-mer, outside the seeding ones (150, 245 and 270 are no multiples of 16: the last segment overlaps the one
before it).  With one entry misread an end has min_match - 1 segments on its diagonal and does not map.

Which lane serves a target: the one of field 15 - b whose rank is that of the unit's letter among the three that differ from the
read's.  A unit's letter reaches two of a field's three lanes at most, so the target segments of a unit are coded alike but for a
shift of the letters (A -> C -> G -> T -> A, once per target): three shifts reach all 48 lanes, which is asserted.

The construction is the condition, and the reference alone must satisfy it (no device): the oracle maps every read, and a count from
the index finds exactly min_match segments with a position on the unit's diagonal, all on the strand the read was taken from.  On the
device: m1, m2, mapping_type, n_hits and the hit lists are the oracle's, and no end of the first four groups leaves the first tier.
The fifth group sends 150-base ends through the second tier: the spoiled segments of four of them are the 16-mers of
test_gpu_seed_list_boundary's planted end of 1,425 positions, whose islands are part of that group's genome."""
import functools

import numpy as np
import pytest

import index_cases as ic
import oracle_py
import refio
import test_gpu_seed_list_boundary as slb

pytestmark = pytest.mark.gpu
ACGT = np.frombuffer(b"ACGT", np.uint8)
CODE = {c: i for i, c in enumerate(b"ACGT")}
COMP = slb.COMP
MAX_DIST = 1000
MIN_ALIGN = 0.85
MIN_ALIGN_TIER2 = 0.3           # (64 of a second-tier end's 150 letters are another place's: it aligns, but not at 0.85)
GAP = 2500                      # random letters between the planted places
LENGTHS = (64, 150, 245, 270)
N_TIER2 = 3                     # pairs of the second-tier group


def min_match_of(L):
    cuts = len(ic.offsets(L)) - 1
    mm = max(1, cuts)
    if cuts > 4:
        mm = (4 * cuts) // 5
    return min(mm, 4)


def targets_of(L):
    """the segments enumerated: all four of a 64-base read, else the first, an inner and the last"""
    S = len(ic.offsets(L))
    return list(range(S)) if L == 64 else [0, S // 2, S - 1]


def make_unit(rng, L):
    """random letters; the 16-mers of the target segments after the first are the first one's with the letters shifted"""
    u = ACGT[rng.integers(0, 4, L)].copy()
    offs, tg = ic.offsets(L), targets_of(L)
    for shift, t in list(enumerate(tg))[::-1]:         # (the last segment may overlap its neighbour: written first, the others over it)
        src = u[offs[tg[0]]:offs[tg[0]] + 16]
        u[offs[t]:offs[t] + 16] = ACGT[(np.array([CODE[x] for x in src.tobytes()]) + shift) % 4]
    return u


def edited(unit, L, t, b, a, islands=None):
    """-> (the unit's letters as a read of target segment t, base b, alternative a sees them; the seeding segments)"""
    offs = ic.offsets(L)
    S, mm = len(offs), min_match_of(L)
    seq = unit.copy()
    q = offs[t] + b
    seq[q] = ACGT[ACGT != unit[q]][a]
    exact = [s for s in ((t + d) % S for d in range(1, S)) if not offs[s] <= q < offs[s] + 16][:mm - 1]
    keep = np.zeros(L, bool)
    for s in exact + [t]:
        keep[offs[s]:offs[s] + 16] = True
    spoiled = [s for s in range(S) if s not in exact and s != t]
    for s in spoiled:
        free = [p for p in range(offs[s], offs[s] + 16) if not keep[p]]
        assert len(free) >= 2
        for p in (free[0], free[-1]):
            seq[p] = ACGT[ACGT != unit[p]][(p + a) % 3]
    if islands is not None:     # whole 16-mers of another place over four spoiled segments that overlap no seeding one
        room = [s for s in spoiled if not keep[offs[s]:offs[s] + 16].any()][:4]
        assert len(room) == 4
        for s, mer in zip(room, islands):
            seq[offs[s]:offs[s] + 16] = np.frombuffer(mer, np.uint8)
    for s in exact:
        assert np.array_equal(seq[offs[s]:offs[s] + 16], unit[offs[s]:offs[s] + 16])
    return seq, sorted(exact + [t])


def lane_of(unit, L, t, b, a):
    """the lane whose entry the target needs: neighbour j of the READ's k-mer that is the unit's k-mer"""
    q = ic.offsets(L)[t] + b
    g = CODE[int(unit[q])]
    r = CODE[int(ACGT[ACGT != unit[q]][a])]
    return 1 + 3 * (15 - b) + (g - (1 if g > r else 0))


def cases_of(L):
    """-> [(t, b, a)]"""
    return [(t, b, a) for t in targets_of(L) for b in range(16) for a in range(3)]


def _index_of(g):
    mers, ukmer, ustart, cs = refio.kmer_index([g])
    return dict(mers=mers, ukmer=ukmer, ustart=ustart, genome=g, contig_starts=cs, contig_len=np.array([len(g)], np.uint32))


def _clear_chance_copies(g, places):
    """every 16-mer of a planted unit must stand in the genome once (as the ladder genome is repaired, index_cases._repair): a chance
    copy elsewhere gets its middle letter changed"""
    inside = np.zeros(len(g), bool)
    for at, L in places:
        inside[at:at + L] = True
    for _ in range(10):
        ix = _index_of(g)
        changed = 0
        for at, L in places:
            for o in range(L - 15):
                k = ic.kmer_of(g[at + o:at + o + 16])
                i = int(np.searchsorted(ix["ukmer"], k))
                for p in ix["mers"][int(ix["ustart"][i]):int(ix["ustart"][i + 1])].tolist():
                    if p != at + o:
                        free = [x for x in range(p, p + 16) if not inside[x]]
                        assert free, "a planted unit repeats one of its own 16-mers"
                        x = free[len(free) // 2]
                        g[x] = ACGT[(CODE[int(g[x])] + 1) % 4]
                        changed += 1
        if not changed:
            return ix
    raise AssertionError("the planted 16-mers could not be cleared of chance copies")


@functools.lru_cache(maxsize=None)
def planted():
    """-> (index of the small genome, {L: (unit 1, its place, unit 2, its place)})"""
    rng = np.random.default_rng(1500)
    pieces, units, at = [ACGT[rng.integers(0, 4, GAP)]], {}, GAP
    for L in LENGTHS:
        u1, u2 = make_unit(rng, L), make_unit(rng, L)
        mid = ACGT[rng.integers(0, 4, 60)]
        units[L] = (u1, at, u2, at + L + 60)
        fill = ACGT[rng.integers(0, 4, GAP)]
        pieces += [u1, mid, u2, fill]
        at += 2 * L + 60 + GAP
    g = np.concatenate(pieces)
    # (one contig: compressed and real coordinates are the same)
    ix = _clear_chance_copies(g, [(p, len(u)) for u1, p1, u2, p2 in units.values() for u, p in ((u1, p1), (u2, p2))])
    for u1, p1, u2, p2 in units.values():
        assert np.array_equal(g[p1:p1 + len(u1)], u1) and np.array_equal(g[p2:p2 + len(u2)], u2)
    return ix, units


@functools.lru_cache(maxsize=None)
def planted_tier2():
    """-> (index: two 150-base units and the islands of test_gpu_seed_list_boundary's first-tier genome, units, the four 16-mers of
    its end with 1,425 positions)"""
    bix, breads = slb.planted(1)
    rng = np.random.default_rng(1501)
    L = 150
    u1, u2 = make_unit(rng, L), make_unit(rng, L)
    head = [ACGT[rng.integers(0, 4, GAP)], u1, ACGT[rng.integers(0, 4, 60)], u2, ACGT[rng.integers(0, 4, GAP)], np.frombuffer(b"N", np.uint8)]
    g = np.concatenate(head + [bix["genome"]])
    ix = _clear_chance_copies(g, [(GAP, L), (GAP + L + 60, L)])
    read = breads[1]
    return ix, {L: (u1, GAP, u2, GAP + L + 60)}, [read[16 * i:16 * i + 16] for i in range(4)]


def pairs_of(units, L, cases, islands=None):
    """-> (first ends, second ends as bytes; per pair the seeding segments; the lanes)"""
    u1, p1, u2, p2 = units[L]
    e1, e2, seeds, lanes = [], [], [], set()
    for t, b, a in cases:
        s1, sd = edited(u1, L, t, b, a, islands)
        s2, sd2 = edited(u2, L, t, b, a, islands)
        assert sd == sd2
        e1.append(s1.tobytes())
        e2.append(COMP[s2][::-1].tobytes())
        seeds.append(sd)
        lanes |= {lane_of(u1, L, t, b, a), lane_of(u2, L, t, b, a)}
    return e1, e2, seeds, lanes


def seeding(ix, read, place):
    """-> ({(strand, segment)} with a position on the diagonal of `place`, the positions the seed stage lists for the end)"""
    size_at = ix["ukmer"]
    L = len(read)
    offs = ic.offsets(L)
    on, total = set(), 0
    for strand, s in enumerate((read, COMP[np.frombuffer(read, np.uint8)][::-1].tobytes())):
        for seg, o in enumerate(offs):
            k = slb._kmer(s[o:o + 16])
            nb = [k] + [(k & ~(3 << (2 * f))) | (a << (2 * f)) for f in range(16) for a in range(4) if a != (k >> (2 * f)) & 3]
            pos = []
            for x in nb:
                i = int(np.searchsorted(size_at, x))
                if i < len(size_at) and int(size_at[i]) == x:
                    pos.append(ix["mers"][int(ix["ustart"][i]):int(ix["ustart"][i + 1])])
            if any(len(p) >= slb.TOO_MANY for p in pos):
                continue
            total += sum(len(p) for p in pos)
            if any(int(x) - o == place for p in pos for x in p.tolist()):
                on.add((strand, seg))
    return on, total


@functools.lru_cache(maxsize=None)
def group(name):
    """-> dict: the packed pairs of a group, the oracle's answers, what the construction says"""
    if name == "tier2":
        ix, units, islands = planted_tier2()
        L = 150
        S = len(ic.offsets(L))
        cases = [(S // 2, b, a) for b, a in ((0, 0), (7, 1), (15, 2))][:N_TIER2]
    else:
        ix, units = planted()
        islands = None
        L = int(name)
        cases = cases_of(L)
    e1, e2, seeds, lanes = pairs_of(units, L, cases, islands)
    r1, l1 = refio.pack_reads(e1)
    r2, l2 = refio.pack_reads(e2)
    ma = MIN_ALIGN_TIER2 if name == "tier2" else MIN_ALIGN
    o = oracle_py.Oracle(ix, paired=True, min_dist=0, max_dist=MAX_DIST, min_align=ma)
    m1, m2, mt, d1, d2 = o.map_batch(r1, l1, r2, l2, debug=True, threads=8)
    return dict(ix=ix, units=units[L], L=L, cases=cases, e1=e1, e2=e2, seeds=seeds, lanes=lanes, min_align=ma, r1=r1, l1=l1, r2=r2, l2=l2, m1=m1, m2=m2, mt=mt,
                d1=d1, d2=d2)


GROUPS = ["64", "150", "245", "270", "tier2"]


@pytest.mark.parametrize("name", GROUPS)
def test_the_reference_maps_every_read_through_exactly_min_match_segments(name):
    """(no device) the construction: every end maps where its unit lies, exactly min_match segments have a position on that
    diagonal -- the target and the exact ones, on the strand the end was read from -- and the targets need every lane"""
    gr = group(name)
    L, mm = gr["L"], min_match_of(gr["L"])
    u1, p1, u2, p2 = gr["units"]
    n = len(gr["cases"])
    assert 2 * n == {"64": 384, "150": 288, "245": 288, "270": 288, "tier2": 2 * N_TIER2}[name]
    assert {"64": (4, 3), "150": (10, 4), "245": (16, 4), "270": (17, 4), "tier2": (10, 4)}[name] == (len(ic.offsets(L)), mm)
    assert (gr["d1"]["n_hits"] == 1).all() and (gr["d2"]["n_hits"] == 1).all()
    assert (gr["d1"]["orient"][:, 0] == 0).all()
    assert (gr["d2"]["orient"][:, 0] == 1).all()
    assert (gr["m1"] > 0).all() and (gr["m2"] > 0).all(), (np.nonzero(gr["m1"] == 0)[0][:5], np.nonzero(gr["m2"] == 0)[0][:5])
    step = 1 if name in ("64", "tier2") else 5          # (the count from the index is slow in Python: every fifth pair of the long reads)
    for i in range(0, n, step):
        on1, tot1 = seeding(gr["ix"], gr["e1"][i], p1)
        on2, tot2 = seeding(gr["ix"], gr["e2"][i], p2)
        assert on1 == {(0, s) for s in gr["seeds"][i]} and len(on1) == mm, (i, on1)
        assert on2 == {(1, s) for s in gr["seeds"][i]} and len(on2) == mm, (i, on2)
        if name == "tier2":
            assert tot1 > slb.KCAP[1] and tot2 > slb.KCAP[1] and tot1 <= slb.KCAP[2] and tot2 <= slb.KCAP[2]
    if name != "tier2":
        assert gr["lanes"] == set(range(1, 49)), sorted(set(range(1, 49)) - gr["lanes"])


def _device(ix):
    from pecaller_amd import PemapDev
    dev = PemapDev(0)
    dev.build_index(ix["genome"], ix["contig_len"])
    return dev


@pytest.fixture(scope="module")
def devs():
    """the device of a group's genome, the replicas built once per genome: the four first-tier groups share one.  One device at a
    time -- the replicas of two do not fit an MI355X side by side"""
    made = {}

    def get(name):
        key = "tier2" if name == "tier2" else "small"
        if key not in made:
            for d in made.values():
                d.close()
            made.clear()
            made[key] = _device(group(name)["ix"])
            assert made[key].lookup_replicas()[0] == 8
        return made[key]
    yield get
    for d in made.values():
        d.close()


def _check(dev, gr, tier2, tiers=True):
    n = len(gr["cases"])
    dev.set_params(paired=True, min_dist=0, max_dist=MAX_DIST, min_align=gr["min_align"])
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(gr["r1"], gr["l1"], gr["r2"], gr["l2"])
    stats, _ = dev.run_stats()
    dbg = dev.debug_hits(2 * n)
    print(stats)
    for which, od, want in ((0, gr["d1"], gr["m1"]), (1, gr["d2"], gr["m2"])):
        nh = dbg["n_hits"][which::2]
        bad = np.nonzero(nh != od["n_hits"])[0]
        assert len(bad) == 0, ("n_hits", which, [gr["cases"][i] for i in bad[:8]])
        for i in range(n):
            k = int(nh[i])
            assert np.array_equal(dbg["spot"][2 * i + which, :k], od["spot"][i, :k]), (which, gr["cases"][i])
            assert np.array_equal(dbg["orient"][2 * i + which, :k], od["orient"][i, :k]), (which, gr["cases"][i])
    assert np.array_equal(m1, gr["m1"]), [gr["cases"][i] for i in np.nonzero(m1 != gr["m1"])[0][:8]]
    assert np.array_equal(m2, gr["m2"]), [gr["cases"][i] for i in np.nonzero(m2 != gr["m2"])[0][:8]]
    assert np.array_equal(mt, gr["mt"])
    assert stats["ends"] == 2 * n
    if tiers:
        assert stats["big_ends"] == (2 * n if tier2 else 0) and stats["mono_ends"] == 0, stats
    return stats


@pytest.mark.parametrize("name", GROUPS)
def test_every_neighbour_entry_reaches_the_vote(devs, name):
    """< 10, 0 > with 4 and with 10 segments, < 16, 0 >, < 19, 0 >, and < 10, 1 > behind < 10, 0 >"""
    gr = group(name)
    stats = _check(devs(name), gr, name == "tier2")
    if name != "tier2":         # (nothing but the planted places answers in the small genome: min_match positions an end)
        assert stats["positions"] == 2 * len(gr["cases"]) * min_match_of(gr["L"]), stats


def test_the_reference_table_layout_agrees(monkeypatch):
    """the cross-check of the test itself: the 64-base group without the replicas (pm_lookup_wave_kernel reads the reference's table)"""
    monkeypatch.setenv("PEMAP_REPLICAS", "0")
    gr = group("64")
    dev = _device(gr["ix"])
    try:
        assert dev.lookup_replicas()[0] == 0
        _check(dev, gr, False, tiers=False)
    finally:
        dev.close()
