"""Inputs that put the full DP (pm_sw_kernel) and its traceback (pm_walk_kernel) to work in every lane geometry pick_geom can choose
(checker side, CPU only; shared by test_dp_cases_cpu.py, which holds the conditions on them, and test_gpu_dp_geometries.py).

A geometry is lanes x W: `lanes` lanes share one alignment and each owns W read columns; the read is right-aligned, pad = lanes * W - mm
wildcard columns in front of it.  A batch's longest read chooses the geometry, so every batch made for a geometry has reads of exactly
`hi` bases in it and none longer.  Per geometry:
  seam    a gap of 1, 3 or 10 bases, once as a deletion and once as an insertion, one column before, at and one column after every
          lane seam, at read lengths whose pads are 0, 1, W - 1, W, W + 1 and several lanes
  sweep   every read length from 16 to hi: clean, one substitution, a 2-base deletion in the middle, a window clipped at the contig's start
  twins   reads from three contigs that have a near-copy each: two and more hits per end (the DP without directions, then the re-score)
  odd     reads from a contig with IUPAC letters and Ns (pm_slow_mask)
  tiny    single-end batches of 1, TPW - 1, TPW and TPW + 1 problems, TPW = 64 / lanes the problems a wave takes at a time
Everything is drawn from fixed seeds."""
import functools

import numpy as np

import refio

ACGT = np.frombuffer(b"ACGT", np.uint8)
ODD_LETTERS = np.frombuffer(b"NRYKMSW", np.uint8)        # test_gpu_edge._edge_genome's (upper case only: .seq holds no lower case)
COMP = np.zeros(256, np.uint8)
COMP[:] = ord("N")
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b

PARAMS = dict(min_dist=0, max_dist=500, min_align=0.85)
# (lanes, W, hi): hi = the longest read of every batch made for the geometry
GEOMS = [(8, 13, 104), (8, 19, 152), (16, 10, 160), (16, 13, 208), (16, 16, 256), (16, 19, 278)]
# pick_geom's rule as a table: (longest read from, to, (lanes, W) by default, (lanes, W) with PEMAP_GAPLESS=0)
PICK_GEOM = [(16, 104, (8, 13), (8, 13)),
             (105, 152, (16, 10), (8, 19)),
             (153, 160, (16, 10), (16, 10)),
             (161, 208, (16, 13), (16, 13)),
             (209, 256, (16, 16), (16, 16)),
             (257, 278, (16, 19), (16, 19))]
KINDS = ("seam", "sweep", "twins", "odd", "tiny")
GAP_SIZES = (1, 3, 10)
PLAIN = range(3, 12)          # contigs of uniform random letters without a twin
TWINNED = (0, 1, 2, 12, 13, 14)
ODD = 15
BIS_GEOM = 3                  # the geometry whose seam and sweep batches also run in bisulfite mode (16 x 13)


def geom_name(gi):
    return "%dx%d" % GEOMS[gi][:2]


def picked(read_len, gapless_on=True):
    for lo, hi, dflt, off in PICK_GEOM:
        if lo <= read_len <= hi:
            return dflt if gapless_on else off
    raise ValueError(read_len)


def tiny_sizes(lanes):
    tpw = 64 // lanes
    return (1, tpw - 1, tpw, tpw + 1)


# ---- the genome
@functools.lru_cache(maxsize=None)
def contigs():
    """12 contigs of 5,000 uniform random letters (test_gpu_traceback._contigs), twins of contigs 0..2 (a substitution about every 60
    bases, a 2-base deletion about every 700) as contigs 12..14, and an odd contig: one of NRYKMSW about every 40 bases and an N run"""
    rng = np.random.default_rng(2024)
    cs = [ACGT[rng.integers(0, 4, 5000)].copy() for _ in range(12)]
    rng = np.random.default_rng(2025)
    for k in range(3):
        t = cs[k].copy()
        # (evenly spread, 50 .. 70 bases apart: never two in one 16-base seed segment, which a twin's hit would not survive)
        for q in range(30, len(t) - 30, 60):
            q += int(rng.integers(-10, 11))
            t[q] = ACGT[(b"ACGT".index(t[q]) + int(rng.integers(1, 4))) % 4]
        keep = np.ones(len(t), bool)
        for q in range(350, len(t) - 30, 700):
            q += int(rng.integers(-100, 101))
            keep[q:q + 2] = False
        cs.append(t[keep].copy())
    odd = ACGT[rng.integers(0, 4, 5000)].copy()
    m = rng.random(len(odd)) < 1 / 40
    odd[m] = ODD_LETTERS[rng.integers(0, len(ODD_LETTERS), int(m.sum()))]
    odd[2600:2617] = ord("N")
    cs.append(odd)
    for c in cs:
        c.flags.writeable = False
    return tuple(cs)


@functools.lru_cache(maxsize=None)
def index(bis=False):
    cs = contigs()
    mers, ukmer, ustart, starts = refio.kmer_index(cs, bisulfite=bis)
    return dict(mers=mers, ukmer=ukmer, ustart=ustart, genome=np.concatenate(cs), contig_starts=starts,
                contig_len=np.array([len(c) for c in cs], dtype=np.uint32))


# ---- pairs.  An end is built as letters of the forward strand; the fragment's right end is then read on the other strand.
def _emit(r1, r2, left, right, rng):
    """-> whether the fragment's left end became read 1"""
    a, b = left, COMP[right][::-1]
    first = bool(rng.random() < 0.5)
    if not first:
        a, b = b, a
    r1.append(a.tobytes())
    r2.append(b.tobytes())
    return first


def _fragment(c, span, lb, rng, s=None):
    """a fragment for a subject end that covers `span` reference bases and a mate of lb bases which starts 20..200 bases apart from it
    (at most 480 bases in all: max_dist is 500) -> (fragment start, fragment length)"""
    fl = min(max(span, lb) + int(rng.integers(20, 201)), 480)
    if s is None:
        s = int(rng.integers(0, len(c) - fl + 1))
    return s, fl


def _substitute(x, rng, rate=0.01):
    """as high_cases._substitute: a random letter at 1 % of the bases (one in four is the letter that stood there)"""
    m = rng.random(len(x)) < rate
    x[m] = ACGT[rng.integers(0, 4, int(m.sum()))]


def _deleted(c, lo, mm, p, b):
    """mm read bases from reference position lo that skip b reference bases after read offset p"""
    return np.concatenate([c[lo:lo + p], c[lo + p + b:lo + mm + b]])


def _inserted(c, lo, mm, p, b, rng):
    """... that carry b random bases after read offset p, cut to mm"""
    return np.concatenate([c[lo:lo + p], ACGT[rng.integers(0, 4, b)], c[lo + p:lo + mm]])[:mm]


def seam_lengths(lanes, W, hi):
    return sorted({hi, hi - 1, hi - W + 1, hi - W, hi - W - 1, max(hi - 3 * W - 5, 40)}, reverse=True)


def insertion_fits(mm, b):
    """an insertion of b bases leaves at most mm - b matches: below min_align's floor (with one base to spare) it cannot map"""
    return not (mm - b - 2 - (b - 1) / 36 < 0.85 * mm + 1)


def seam_plan(lanes, W, hi):
    """(mm, g, off, p, b, insertion) of every planted gap, the longest reads first"""
    plan = []
    for mm in seam_lengths(lanes, W, hi):
        pad = lanes * W - mm
        for g in range(1, lanes):
            for off in (-1, 0, 1):
                p = g * W - pad + off          # read columns p and p + 1 (1-based) sit left and right of the gap
                if not 1 <= p <= mm - 1:
                    continue
                for b in GAP_SIZES:
                    plan.append((mm, g, off, p, b, False))
                    if insertion_fits(mm, b):
                        plan.append((mm, g, off, p, b, True))
    return plan


def seedable(x, c, lo, shift):
    """whether initial_map (pemapper.c:1539-1690) can find the end x, made from reference position lo with one gap that moves its
    diagonal by `shift`: the read is cut at 0, 16, ... and mm - 16, a segment is found when it differs from the reference in at most
    one letter (the neighbour look-ups), on diagonals up to 11 apart, and a hit needs min (4, cuts or 4/5 of them) segments"""
    mm = len(x)
    cuts = mm // 16 - (mm % 16 == 0)
    need = min(4, (4 * cuts) // 5 if cuts > 4 else max(1, cuts))
    found = 0
    for o in [16 * i for i in range(cuts)] + [mm - 16]:
        found += any(int((x[o:o + 16] != c[lo + o + sh:lo + o + sh + 16]).sum()) <= 1 for sh in (0, shift))
    return found >= need


SEAM_DT = np.dtype([("mm", "<i4"), ("g", "<i4"), ("off", "<i4"), ("p", "<i4"), ("b", "<i4"), ("ins", "?"), ("first", "?"), ("reverse", "?")])


def _seam(gi):
    lanes, W, hi = GEOMS[gi]
    cs = contigs()
    rng = np.random.default_rng(1000 + gi)
    plan = seam_plan(lanes, W, hi)
    meta = np.zeros(len(plan), SEAM_DT)
    r1, r2 = [], []
    for k, (mm, g, off, p, b, ins) in enumerate(plan):
        span = mm if ins else mm + b
        lb = int(rng.integers(max(40, hi - 60), hi + 1))
        reverse = bool(rng.random() < 0.5)       # the gapped end is the fragment's right end, read on the other strand
        # The site is drawn again until the seed stage can find the end (a gap near the end of a 60-base read leaves two of its four
        # segments whole where three are needed: whether such an end is seeded hangs on the letters beside the gap), and it keeps 30
        # bases from the contig's ends: a clipped window has no room for a 10-base deletion.  This batch is about the DP.
        for _ in range(200):
            c = cs[int(rng.integers(PLAIN.start, PLAIN.stop))]
            fl = _fragment(c, span, lb, rng)[1]
            s = int(rng.integers(30, len(c) - fl - 29))
            lo = s + fl - span if reverse else s
            x = _inserted(c, lo, mm, p, b, rng) if ins else _deleted(c, lo, mm, p, b)
            if seedable(x, c, lo, -b if ins else b):
                break
        else:
            raise AssertionError("no seedable site for %r" % ((mm, g, off, p, b, ins),))
        assert len(x) == mm
        mate = c[s:s + lb] if reverse else c[s + fl - lb:s + fl]
        left_first = _emit(r1, r2, mate if reverse else x, x if reverse else mate, rng)
        meta[k] = (mm, g, off, p, b, ins, left_first != reverse, reverse)
    return refio.pack_reads(r1) + refio.pack_reads(r2), meta


SWEEP_KINDS = ("clean", "sub", "del", "clipped")
SWEEP_DT = np.dtype([("mm", "<i4"), ("kind", "<i4"), ("first", "?")])


def _sweep(gi):
    lanes, W, hi = GEOMS[gi]
    cs = contigs()
    rng = np.random.default_rng(2000 + gi)
    meta = []
    r1, r2 = [], []
    for mm in range(16, hi + 1):
        for kind in range(4):
            c = cs[int(rng.integers(PLAIN.start, PLAIN.stop))]
            lb = int(rng.integers(16, hi + 1))
            dele = kind == 2 and mm >= 48
            span = mm + 2 if dele else mm
            clipped = kind == 3
            s, fl = _fragment(c, span, lb, rng, s=int(rng.integers(0, 3)) if clipped else None)
            reverse = (not clipped) and bool(rng.random() < 0.5)
            lo = s + fl - span if reverse else s
            x = _deleted(c, lo, mm, mm // 2, 2) if dele else c[lo:lo + mm].copy()
            if kind == 1:
                q = int(rng.integers(0, mm))
                x[q] = ACGT[(b"ACGT".index(x[q]) + int(rng.integers(1, 4))) % 4]
            mate = c[s:s + lb] if reverse else c[s + fl - lb:s + fl]
            left_first = _emit(r1, r2, mate if reverse else x, x if reverse else mate, rng)
            meta.append((mm, kind, left_first != reverse))
    return refio.pack_reads(r1) + refio.pack_reads(r2), np.array(meta, SWEEP_DT)


def _two_ends(gi, seed, n, which, dele_every=0):
    """n pairs of hi - 30 .. hi bases (the first pair's left end has hi) from the contigs `which`; dele_every: every that many pairs,
    one end with a 2-base deletion in its middle and the rest clean, else 1 % substitutions"""
    lanes, W, hi = GEOMS[gi]
    cs = contigs()
    rng = np.random.default_rng(seed + gi)
    r1, r2 = [], []
    for k in range(n):
        c = cs[which[int(rng.integers(0, len(which)))]]
        la, lb = (hi if k == 0 else int(rng.integers(hi - 30, hi + 1))), int(rng.integers(hi - 30, hi + 1))
        fl = int(rng.integers(max(la, lb) + 22, 481))
        s = int(rng.integers(0, len(c) - fl + 1))
        dele = dele_every and k % dele_every == 1
        left = _deleted(c, s, la, la // 2, 2) if dele else c[s:s + la].copy()
        right = c[s + fl - lb:s + fl].copy()
        if not dele_every:
            _substitute(left, rng)
            _substitute(right, rng)
        _emit(r1, r2, left, right, rng)
    return refio.pack_reads(r1) + refio.pack_reads(r2)


@functools.lru_cache(maxsize=None)
def batches(gi):
    """{name: (paired, (rows1, len1, rows2, len2), meta or None)} of one geometry, in the order they are mapped"""
    lanes, W, hi = GEOMS[gi]
    seam, meta = _seam(gi)
    out = dict(seam=(True, seam, meta))
    sweep, smeta = _sweep(gi)
    out["sweep"] = (True, sweep, smeta)
    out["twins"] = (True, _two_ends(gi, 3000, 600, TWINNED), None)
    out["odd"] = (True, _two_ends(gi, 4000, 400, (ODD,), dele_every=2), None)
    # the gapped ends of the first seam pairs on their own
    k = max(tiny_sizes(lanes))
    rows = np.stack([seam[0][i] if meta["first"][i] else seam[2][i] for i in range(k)])
    lens = np.array([seam[1][i] if meta["first"][i] else seam[3][i] for i in range(k)], np.int32)
    for n in tiny_sizes(lanes):
        out["tiny%d" % n] = (False, (rows[:n].copy(), lens[:n].copy(), None, None), meta[:n])
    for paired, reads, _ in out.values():
        for a in reads:
            if a is not None:
                a.flags.writeable = False
    return out


def names_of(gi, kind):
    """the batches behind one test id"""
    return ["tiny%d" % n for n in tiny_sizes(GEOMS[gi][0])] if kind == "tiny" else [kind]


@functools.lru_cache(maxsize=None)
def bisulfite_batch(name):
    """the BIS_GEOM geometry's seam or sweep batch with 95 % of the reads' C turned into T"""
    paired, reads, meta = batches(BIS_GEOM)[name]
    rng = np.random.default_rng(5000 + len(name))
    out = []
    for rows, lens in (reads[:2], reads[2:]):
        rows = rows.copy()
        conv = (rows == ord("C")) & (rng.random(rows.shape) < 0.95)
        rows[conv] = ord("T")
        rows.flags.writeable = False
        out += [rows, lens]
    return paired, tuple(out), meta


def longest(reads):
    return int(max(reads[1].max(), reads[3].max() if reads[3] is not None else 0))


def gapped_end(reads, meta, i):
    """(row, length) of seam pair i's end that carries the gap"""
    k = 0 if meta["first"][i] else 2
    return reads[k][i], int(reads[k + 1][i])
