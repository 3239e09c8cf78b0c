"""The "ladder" genome and its reads: inputs for the index builder, the look-up replicas and the seed stage's reading of them at the
bucket-size edges (the too_many_spots rule `this_tot >= 100`, pemapper.c:1599-1606 and 1627; get_mers' 32-bit `which + 1`,
pemapper.c:2163).  Shared by test_index_cases_cpu.py, test_gpu_index_cases.py and tests/golden/make_golden_index.py; a plain module
like pair_cases.py.

  genome(seed)            contigs of random letters that hold, each with its places recorded:
      islands             for c in ISLANDS one random 16-mer planted c times as N + 16 letters + N: a bucket of exactly c positions
      families            a 60-base unit planted into F random contexts 320 bases apart: every 16-mer of the unit has a bucket of F.
                          Siblings of a unit differ from it in every 16th base (A <-> G <-> ... never C <-> T, so also under
                          bisulfite indexing): every 16-mer of one is a one-substitution neighbour of a 16-mer of the other
      homopolymers        40 T (k-mer 0xFFFFFFFF), 40 A (k-mer 0), 60 bases of C / T only and 60 of G / A only, inside ordinary sequence
      letters             IUPAC letters, N runs of 1, 15, 16 and 17, an N as a contig's first letter and one as a last letter
      contigs             of exactly 16 letters, of 17, of 16 with an N; ends of the others on multiples of 4096, 256 and 64
                          +- {0, 1, 15, 16} in real positions; contigs[:n_trunc] is a genome whose length is a multiple of 4096
  index(bisulfite, trunc) refio.kmer_index of it as the mappers and the oracle take it
  reads(L, bisulfite)     pairs whose designed end tiles copies of every family and every homopolymer stretch at every phase
  expected(L, bisulfite)  the oracle's results for them (computed once, shared, never modified)
  write_untidy_fasta      the genome as the committed ladder.fa.gz holds it: mixed case, digits * and - in the lines, CRLF, long lines
"""
import functools

import numpy as np

import oracle_py
import refio

ACGT = np.frombuffer(b"ACGT", np.uint8)
AG = np.frombuffer(b"AG", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[:] = ord("N")
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b

SEED = 1
READ_SEED = 4100
TOO_MANY = 100                     # too_many_spots, pemapper.c:163
ISLANDS = (1, 2, 3, 4, 5, 7, 8, 11, 12, 98, 99, 100, 101, 250)
UNIT, STEP = 60, 320               # a family's unit and the distance between the starts of two copies
SIB_AT = (5, 21, 37, 53)           # where siblings differ: one place inside every 16-mer of the unit
SIB_LETTERS = b"AGAG"              # the letter there, by sibling number (never C against T)
# name -> copies of the unit and of each sibling
FAMILIES = (("f98", (98,)), ("f99", (99,)), ("f100", (100,)), ("f101", (101,)),
            ("n99_100", (99, 100)),          # own bucket below the limit, a neighbour's on it: the segment is dropped
            ("n60_60", (60, 60)),            # no bucket reaches the limit, their sum does: the segment is kept
            ("n99_99", (99, 99)),
            ("n99x3", (99, 99, 99)))         # 297 positions per segment: four segments pass the 1,024 of the wave-per-end kernels
SIB3_AT = (13, 29, 45)             # the third sibling differs from the unit elsewhere (it is two substitutions from the second)
HOMOPOLYMERS = ("T40", "A40", "CT60", "GA60")
TILE, ROUND, WAVE = 4096, 256, 64
DELTAS = (0, 1, 15, 16, -1, -15, -16)
MIN_CONTIG = 20000


def _header(i):
    """the FASTA header of contig i: every third with trailing punctuation, every third with a description"""
    return b">lad%d" % i + (b"", b"...", b" ladder genome, test;")[i % 3]


def _name(i):
    """what the builder makes of it (index_genome_whole.c:228-240): cut after the last letter or digit, white space -> '_'"""
    return "lad%d" % i + ("", "", "_ladder_genome,_test")[i % 3]


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _next_target(pos, base, delta):
    """smallest m * base + delta >= pos + 40 where m * base is not a multiple of the next larger unit"""
    upper = {WAVE: ROUND, ROUND: TILE, TILE: 0}[base]
    m = (pos + 40 - delta + base - 1) // base
    while upper and (m * base) % upper == 0:
        m += 1
    return m * base + delta


@functools.lru_cache(maxsize=None)
def genome(seed=SEED):
    """-> dict(names, contigs, islands, families, homopolymers, n_runs, ends, n_trunc, small)
    islands[c] = (16-mer as bytes, [(contig, offset of the 16 letters)]); families[name] = list per sibling of (unit, [(contig,
    offset)]); homopolymers[name] = (contig, offset, length); n_runs[length] = (contig, offset); ends = list of (contig, base,
    delta) of the contigs whose end was placed; small = dict(c16, c17, c16n) of contig numbers"""
    rng = np.random.default_rng(seed)
    contigs, cur, real = [], [], [0]
    targets = [(b, d) for d in DELTAS for b in (TILE, ROUND, WAVE)]
    targets.remove((TILE, 0))       # kept for the contig before the last ones: the truncated genome ends on it
    ends, rec = [], dict(islands={}, families={}, homopolymers={}, n_runs={}, small={})

    def cur_len():
        return sum(len(x) for x in cur)

    def add(x):
        cur.append(np.asarray(x, np.uint8))
        return len(contigs), cur_len() - len(x)

    def close(target=None):
        """end the open contig: on the next target of the list (filled up with random letters), or where it stands"""
        if target is None and targets:
            target = targets.pop(0)
        if target is not None:
            pos = real[0] + cur_len()
            add(_rand(rng, _next_target(pos, *target) - pos))
            ends.append((len(contigs), target[0], target[1]))
        c = np.concatenate(cur)
        contigs.append(c)
        real[0] += len(c)
        cur.clear()

    def roll():
        if cur_len() >= MIN_CONTIG:
            close()
            add(_rand(rng, 450))

    # ---- families: unit + 260 random letters per copy, the siblings of a group one after the other
    add(_rand(rng, 450))
    for name, copies in FAMILIES:
        unit = _rand(rng, UNIT)
        group = []
        for sib, n in enumerate(copies):
            u = unit.copy()
            for q in SIB_AT:
                u[q] = SIB_LETTERS[sib]
            if sib == 2:
                for q in SIB3_AT:
                    u[q] = ord("G") if unit[q] != ord("G") else ord("A")
            places = []
            for _ in range(n):
                places.append(add(u))
                add(_rand(rng, STEP - UNIT))
                roll()
            group.append((u.tobytes(), places))
        rec["families"][name] = group
    close()
    # ---- homopolymers, IUPAC letters and N runs inside ordinary sequence
    for name in HOMOPOLYMERS:
        flank = ord("C") if name in ("A40", "GA60") else ord("G")      # the stretch begins and ends where it says, in both modes
        add(np.concatenate([_rand(rng, 600), [flank]]))
        if name in ("T40", "A40"):
            x = np.full(40, ord(name[0]), np.uint8)
        else:
            x = np.frombuffer(name[:2].encode(), np.uint8)[rng.integers(0, 2, 60)].copy()
            x[:2] = np.frombuffer(name[:2].encode(), np.uint8)
        c, o = add(x)
        rec["homopolymers"][name] = (c, o, len(x))
        add([flank])
    add(_rand(rng, 600))
    for k, letter in enumerate(b"RYKMSWRYKMSW"):
        add([letter])
        add(_rand(rng, 37 + 11 * k))
    for n in (1, 15, 16, 17):
        c, o = add(np.full(n, ord("N"), np.uint8))
        rec["n_runs"][n] = (c, o)
        add(_rand(rng, 300))
    add(_rand(rng, 5000))
    close()
    # ---- islands, back to back
    add(np.concatenate([[ord("N")], _rand(rng, 300)]))      # (an N as the first letter of a contig)
    rec["first_n"] = len(contigs)
    for c in ISLANDS:
        mer = _rand(rng, 16)
        places = []
        for _ in range(c):
            add([ord("N")])
            places.append(add(mer))
            add([ord("N")])
        add(_rand(rng, 40))
        rec["islands"][c] = (mer.tobytes(), places)
    add(_rand(rng, 400))
    close()
    # ---- ordinary contigs on the targets that are left, one of them with an N as its last letter
    while targets:
        add(_rand(rng, 2000))
        close()
    add(_rand(rng, 3000))
    close((TILE, 0))
    rec["last_n"] = len(contigs) - 2
    contigs[rec["last_n"]][-1] = ord("N")
    n_trunc = len(contigs)
    # ---- the small contigs and a last one that leaves the length off the tile
    for key in ("c16", "c17", "c16n"):
        x = _rand(rng, 17 if key == "c17" else 16)
        if key == "c16n":
            x[9] = ord("N")
        rec["small"][key] = len(contigs)
        contigs.append(x)
        real[0] += len(x)
    add(_rand(rng, 1234))
    close((WAVE, 1))
    _repair(contigs, rec)
    names = [_name(i) for i in range(len(contigs))]
    return dict(rec, names=names, contigs=contigs, ends=ends, n_trunc=n_trunc)


def _keys(c, bisulfite):
    """the k-mer code at every window start of one contig (windows with an N: -1)"""
    code = np.zeros(256, np.int64)
    code[ord("C")], code[ord("G")], code[ord("T")] = (3 if bisulfite else 1), 2, 3
    n = len(c) - 15
    k = np.zeros(n, np.int64)
    for i in range(16):
        k = (k << 2) | code[c[i:i + n]]
    isn = np.concatenate([[0], np.cumsum(c == ord("N"))])
    k[(isn[16:] - isn[:-16]) > 0] = -1
    return k


def _repair(contigs, rec):
    """Random sequence holds a planted 16-mer by chance now and then (one window in a hundred under bisulfite indexing, where C
    reads as T): every such window outside the planted places gets one letter outside them changed (A -> G -> C -> A, T -> G: another
    code in both modes, and no way back to a sibling unit), until every planted bucket has the size it was planted with."""
    swap = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"GACG"):
        swap[a] = b
    planted = [np.zeros(len(c), bool) for c in contigs]         # window starts that are planted
    inside = [np.zeros(len(c), bool) for c in contigs]          # letters of the planted units and islands
    wanted = {False: set(), True: set()}
    for group in rec["families"].values():
        for unit, places in group:
            for bis in (False, True):
                wanted[bis].update(kmer_of(unit[o:o + 16], bis) for o in range(UNIT - 15))
            for c, o in places:
                planted[c][o:o + UNIT - 15] = True
                inside[c][o:o + UNIT] = True
    for mer, places in rec["islands"].values():
        for bis in (False, True):
            wanted[bis].add(kmer_of(mer, bis))
        for c, o in places:
            planted[c][o] = True
            inside[c][o:o + 16] = True
    for _ in range(20):
        changed = 0
        for bis in (False, True):
            want = np.array(sorted(wanted[bis]), np.int64)
            for ci, c in enumerate(contigs):
                if len(c) < 16:
                    continue
                hit = np.nonzero(np.isin(_keys(c, bis), want) & ~planted[ci][:len(c) - 15])[0]
                last = -16
                for w in hit:
                    if w < last + 16:       # (the windows of one chance copy overlap: one change per pass clears them)
                        continue
                    last = w
                    free = np.nonzero(~inside[ci][w:w + 16])[0]
                    assert len(free), "a planted unit repeats one of its own 16-mers"
                    c[w + free[len(free) // 2]] = swap[c[w + free[len(free) // 2]]]
                    changed += 1
        if not changed:
            return
    raise AssertionError("the planted buckets could not be cleared of chance copies")


def real_starts(contigs):
    return np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def index(bisulfite=False, trunc=False, seed=SEED):
    g = genome(seed)
    cs = g["contigs"][:g["n_trunc"]] if trunc else g["contigs"]
    mers, ukmer, ustart, st = refio.kmer_index(cs, bisulfite=bisulfite)
    return dict(mers=mers, ukmer=ukmer, ustart=ustart, genome=np.concatenate(cs), contig_starts=st,
                contig_len=np.array([len(c) for c in cs], dtype=np.uint32))


def kmer_of(letters, bisulfite=False):
    """the 32-bit code of 16 letters as the index builder forms it (index_genome_whole.c:169-177, 263-267)"""
    code = {ord("A"): 0, ord("C"): 3 if bisulfite else 1, ord("G"): 2, ord("T"): 3}
    k = 0
    for x in bytes(letters):
        k = (k << 2) | code.get(x, 0)
    return k


def bucket_len(ix, k):
    i = int(np.searchsorted(ix["ukmer"], k))
    if i < len(ix["ukmer"]) and int(ix["ukmer"][i]) == k:
        return int(ix["ustart"][i + 1]) - int(ix["ustart"][i])
    return 0


def sdx_text(names, contigs):
    """the .sdx of the reference builder (index_genome_whole.c:347-350)"""
    return "%d\n" % len(contigs) + "".join("%d\t%s\n" % (len(c) - 15, n) for n, c in zip(names, contigs)) + "16\n"


def write_untidy_fasta(path, g, seed=7):
    """the contigs as a FASTA file that needs the reader's toupper, its isalpha filter and its 255-byte pieces
    (index_genome_whole.c:192-312): lower-case letters, digits, '*' and '-' and blanks inside the lines, CRLF on some lines, lines of
    every length up to 300 and one of 700 and one of 5,000 letters, headers with a description and trailing punctuation (the
    builder turns white space into '_' and drops what follows the last letter or digit)"""
    rng = np.random.default_rng(seed)
    junk = b"0123456789*- "
    with open(path, "wb") as f:
        for i, (name, c) in enumerate(zip(g["names"], g["contigs"])):
            head = _header(i)
            f.write(head + (b"\r\n" if i % 2 else b"\n"))
            low = rng.random(len(c)) < (0.3 if i % 4 else 1.0 if i == 4 else 0.0)
            x = np.where(low, c | 0x20, c).astype(np.uint8).tobytes()
            o, line = 0, 0
            while o < len(x):
                w = 700 if (i, line) == (1, 3) else 5000 if (i, line) == (2, 5) else int(rng.integers(1, 301))
                piece = bytearray(x[o:o + w])
                for _ in range(int(rng.integers(0, 3))):
                    piece.insert(int(rng.integers(0, len(piece) + 1)), junk[int(rng.integers(0, len(junk)))])
                f.write(bytes(piece) + (b"\r\n" if rng.random() < 0.2 else b"\n"))
                o += w
                line += 1


# --------------------------------------------------------------------------------------------------------------------
# reads
# --------------------------------------------------------------------------------------------------------------------
def offsets(L):
    """the segment offsets of initial_map (pemapper.c:1569-1583): every 16 bases, the last one at L - 16"""
    cuts = L // 16 - (1 if L % 16 == 0 else 0)
    return [16 * i for i in range(cuts)] + [L - 16]


def _substitute(x, n, rng):
    for q in rng.choice(len(x), size=n, replace=False):
        o = ACGT[ACGT != x[q]]
        x[q] = o[int(rng.integers(0, len(o)))]


@functools.lru_cache(maxsize=None)
def read_plan(L, seed=READ_SEED):
    """-> list of dict(kind, sib, contig, start (of the designed end in its contig), target (start of the copy or stretch), strand,
    subs, flen, broken): what reads() builds, without the letters.  The designed end starts at target - L + 16 ... target + length of the
    unit or stretch, so that the planted k-mers land on every segment offset, the last overlapping segment included.  A read of 100
    bases or more has so many segments outside a 60-base unit that it finds its place with or without the unit's; the `broken`
    reads (a second pass over the families) therefore carry two substitutions in every segment outside the unit but one, which
    leaves the place found only if the unit's segments count."""
    g = genome()
    rng = np.random.default_rng(seed + L)
    lens = [len(c) for c in g["contigs"]]
    plan = []

    def tile(kind, sib, places, length, broken=False):
        ok = [(c, o) for c, o in places if o >= L + 330 and o + length + L + 330 <= lens[c]]
        pick = [ok[int(i)] for i in rng.choice(len(ok), size=min(3, len(ok)), replace=False)]
        for ph, start_off in enumerate(range(-L + 16, length + 1)):
            c, o = pick[ph % len(pick)]
            plan.append(dict(kind=kind, sib=sib, contig=c, start=o + start_off, target=o, strand=int(rng.integers(0, 2)),
                             subs=(0, 0, 1, 2, 1, 0)[int(rng.integers(0, 6))], flen=L + int(rng.integers(100, 300)), broken=broken))

    for name, group in g["families"].items():
        for sib, (_, places) in enumerate(group):
            tile(name, sib, places, UNIT)
            if L >= 100:
                tile(name, sib, places, UNIT, broken=True)
    for name, (c, o, n) in g["homopolymers"].items():
        tile(name, 0, [(c, o)], n)
    big = [c for c in range(len(lens)) if lens[c] > 4 * L + 1300]
    for _ in range(400):
        c = big[int(rng.integers(0, len(big)))]
        fl = L + int(rng.integers(20, 300))
        plan.append(dict(kind="ordinary", sib=0, contig=c, start=int(rng.integers(L + 300, lens[c] - fl - L - 300)), target=-1,
                         strand=int(rng.integers(0, 2)), subs=int(rng.integers(0, 3)), flen=fl, broken=False))
    return plan


def _break_flank(d, p, L, rng):
    """two substitutions in every segment that is not wholly inside the unit, outside the unit and outside the one segment that is
    kept whole (the first, or the last where the unit lies in the read's first half)"""
    t = p["target"] - p["start"]
    offs = offsets(L)
    flank = [o for o in offs if not (t <= o and o + 16 <= t + UNIT)]
    if len(flank) < 2:
        return
    kept = flank[0] if t + UNIT // 2 > L // 2 else flank[-1]
    taken = np.zeros(L, bool)
    taken[max(t, 0):max(t + UNIT, 0)] = True
    taken[kept:kept + 16] = True
    for o in flank:
        if o == kept:
            continue
        free = o + np.nonzero(~taken[o:o + 16])[0]
        for q in (rng.choice(free, size=2, replace=False) if len(free) >= 2 else ()):
            other = AG if d[q] in b"CT" else ACGT[ACGT != d[q]]         # (C against T is no mismatch under bisulfite conversion)
            d[q] = other[int(rng.integers(0, len(other)))]
            taken[q] = True


@functools.lru_cache(maxsize=None)
def read_ends(L, bisulfite=False, seed=READ_SEED):
    """-> (reads of file 1, reads of file 2, which file holds the designed end of every pair).  strand 0: the designed end reads
    the genome forward and its mate the other strand `flen` downstream; strand 1: the designed end is the reverse complement and
    its mate lies upstream.  Bisulfite: 95 % of the C of both ends read as T, as _edge_reads of test_gpu_edge.py does."""
    g = genome()
    rng = np.random.default_rng(seed + 7 * L + int(bisulfite))
    r1, r2, where = [], [], []
    for p in read_plan(L, seed):
        c = g["contigs"][p["contig"]]
        s, fl = p["start"], p["flen"]
        d = c[s:s + L].copy()
        if p["strand"] == 0:
            m = COMP[c[s + fl - L:s + fl]][::-1].copy()
        else:
            m = c[s + L - fl:s + 2 * L - fl].copy()
        assert len(d) == L and len(m) == L, p
        if p["broken"]:
            _break_flank(d, p, L, rng)
        else:
            _substitute(d, p["subs"], rng)
        _substitute(m, int(rng.integers(0, 3)), rng)
        if p["strand"] == 1:
            d = COMP[d][::-1].copy()
        if bisulfite:
            for x in (d, m):
                conv = (x == ord("C")) & (rng.random(L) < 0.95)
                x[conv] = ord("T")
        w = int(rng.integers(0, 2))
        a, b = (d, m) if w == 0 else (m, d)
        r1.append(a.tobytes())
        r2.append(b.tobytes())
        where.append(w)
    return r1, r2, np.array(where)


@functools.lru_cache(maxsize=None)
def reads(L, bisulfite=False):
    """-> (buf1, len1, buf2, len2) as the mappers take them"""
    r1, r2, _ = read_ends(L, bisulfite)
    return refio.pack_reads(r1) + refio.pack_reads(r2)


@functools.lru_cache(maxsize=None)
def expected(L, bisulfite=False):
    """the oracle's results on an empty pileup"""
    b1, l1, b2, l2 = reads(L, bisulfite)
    o = oracle_py.Oracle(index(bisulfite), paired=True, min_dist=0, max_dist=500, min_align=0.85, bisulfite=bisulfite)
    m1, m2, mt, d1, d2 = o.map_batch(b1, l1, b2, l2, debug=True, threads=8)
    return dict(m1=m1, m2=m2, mt=mt, d=(d1, d2), counts=o.counts().copy(), ins=sorted(o.insertions()), summary=o.summary().copy())


def designed_hits(L, bisulfite=False):
    """-> n_hits of the designed end of every pair, and per pair whether its true place is in the hit list"""
    e = expected(L, bisulfite)
    _, _, where = read_ends(L, bisulfite)
    cst = index(bisulfite)["contig_starts"].astype(np.int64)
    n = len(where)
    nh = np.where(where == 0, e["d"][0]["n_hits"], e["d"][1]["n_hits"])
    found = np.zeros(n, bool)
    for i, p in enumerate(read_plan(L)):
        d = e["d"][int(where[i])][i]
        spot = cst[p["contig"]] + p["start"]
        found[i] = spot in d["spot"][:d["n_hits"]].astype(np.int64)
    return nh, found


def segments_inside(p, L, length=UNIT):
    """how many of the designed end's segments lie wholly inside the planted unit or stretch"""
    return sum(1 for o in offsets(L) if p["target"] <= p["start"] + o and p["start"] + o + 16 <= p["target"] + length)
