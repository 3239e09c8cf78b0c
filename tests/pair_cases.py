"""Inputs and a plain reference for the pair / single-end selection (pm_select_kernel, "K4" in DESIGN.md; find_mate_pairs and the
single-end rule of the reference, pemapper.c:1084-1185 and 1313-1536).  Shared by test_pair_select_cpu.py, test_gpu_pair_select.py
and tests/golden/make_golden_pair.py; a plain module like multi_object_common.py.

  genome(seed)     8 contigs of 24 kb of random letters (8: the reference's contig search is only defined for 1 or >= 8 contigs, see
                   find_chrom in oracle/pemap_oracle.c) with planted repeats: far copies of 600-base blocks on other contigs (one
                   to four copies, each with its own divergence), 130-base blocks repeated 140..400 bases downstream, and one
                   family of 32 copies of a 500-base block
  reads(...)       read pairs of the kinds listed in KINDS, mixed in one batch and swapped between the two files at random
  select_py(...)   the selection, restated in plain Python over the oracle's debug records; `variant` names one deliberate error
  SETS             the parameter sets; expected(name) runs the oracle once per set and keeps the result
"""
import functools

import numpy as np

import oracle_py
import refio

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[:] = ord("N")
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b

SEED = 20261
READ_SEED = 77
PAIRS = 3000
NC, CL = 8, 24000
BLOCK, NEAR, FAM, FAM_COPIES = 600, 130, 500, 32
COPIES = (1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 4)          # far copies of block k beside its source
DIVERGENCE = (0.0, 0.01, 0.02, 0.03, 0.05)
NARROW = (150, 300)                                 # the limits that the reads of kind "limits" are built around ...
OTHER_LIMITS = ((0, 500), (0, 0), (0, 5000))        # ... and the limits of the other sets, which get a share of them
# the deliberate errors select_py knows.  "clamp": the second end's ties measured against its LAST score where the first end's best
# index is past its list (a 0.0 fill in place of -1.0 could never differ, scores are never negative); it can only decide where
# the second end has three hits or more, since two hits cannot make two ties
VARIANTS = ("best2", "max_lt", "min_gt", "no_orient", "no_slip", "good_gt", "clamp")
# one entry per 15 pairs
KINDS = ("in_block", "in_block", "same_strand", "unrelated", "other_block", "other_block", "fill", "fill", "fill", "near_left",
         "near_right", "limits", "family", "ordinary", "ordinary")


def _mutate(x, rate, rng):
    m = rng.random(len(x)) < rate
    x[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
    return x


@functools.lru_cache(maxsize=None)
def genome(seed=SEED):
    """-> dict(names, contigs, blocks, near, family, fam_seq)
    blocks[k] = list of (contig, start) of the places of far block k, the source first; near[k] = (contig, start, shift);
    family = list of (contig, start) of the family's copies, fam_seq = the sequence they were all diverged from"""
    rng = np.random.default_rng(seed)
    cs = [ACGT[rng.integers(0, 4, CL)].copy() for _ in range(NC)]
    blocks = []
    for k in range(16):         # sources at 1000 and 2600, copies at 4000 + 700 k on the following contigs
        c, s = k % NC, 1000 + 1600 * (k // NC)
        src = cs[c][s:s + BLOCK].copy()
        places = [(c, s)]
        for j in range(COPIES[k]):
            d, t = (c + 1 + j) % NC, 4000 + 700 * k
            cs[d][t:t + BLOCK] = _mutate(src.copy(), float(rng.choice(DIVERGENCE)), rng)
            places.append((d, t))
        blocks.append(places)
    near = []
    for k in range(12):         # a 130-base block again 140 .. 382 bases downstream
        c, s, d = k % NC, 16000 + 1500 * (k // NC), 140 + 22 * k
        cs[c][s + d:s + d + NEAR] = cs[c][s:s + NEAR]
        near.append((c, s, d))
    fam_seq = ACGT[rng.integers(0, 4, FAM)].copy()
    family = []
    for k in range(FAM_COPIES):  # four copies per contig, 1200 bases apart, each 1 .. 3 % from the common sequence
        c, s = k % NC, 19000 + 1200 * (k // NC)
        cs[c][s:s + FAM] = _mutate(fam_seq.copy(), float(rng.uniform(0.01, 0.03)), rng)
        family.append((c, s))
    return dict(names=["pc%d" % i for i in range(NC)], contigs=cs, blocks=blocks, near=near, family=family, fam_seq=fam_seq)


@functools.lru_cache(maxsize=None)
def index(seed=SEED):
    cs = genome(seed)["contigs"]
    mers, ukmer, ustart, st = refio.kmer_index(cs)
    return dict(mers=mers, ukmer=ukmer, ustart=ustart, genome=np.concatenate(cs), contig_starts=st,
                contig_len=np.array([len(c) for c in cs], dtype=np.uint32))


def limit_distances(min_dist=NARROW[0], max_dist=NARROW[1]):
    """the spot distances that kind "limits" uses: one below, on, on and one above the limits of every set"""
    out = []
    for lo, hi in ((min_dist, max_dist),) + OTHER_LIMITS:
        out += [lo - 1, lo, hi, hi + 1]
    return sorted(set(d for d in out if d >= 0))


def _substitute(x, n, rng):
    for q in rng.choice(len(x), size=n, replace=False):
        o = ACGT[ACGT != x[q]]
        x[q] = o[int(rng.integers(0, 3))]


def read_ends(g, seed, n, L, min_dist=NARROW[0], max_dist=NARROW[1]):
    """-> two lists of n reads (bytes), and the kind of every pair.  A fragment is `fl` bases from `s` on one contig: the first
    mate reads its first L bases, the second the reverse complement of its last L bases, so the spot distance of a pair that maps
    where it was taken is fl - L."""
    rng = np.random.default_rng(seed)
    cs, blocks, near, family = g["contigs"], g["blocks"], g["near"], g["family"]
    limits = limit_distances(min_dist, max_dist)
    narrow = [min_dist - 1, min_dist, max_dist, max_dist + 1]
    r1, r2, kinds = [], [], []
    n_lim = 0

    def rc(x):
        return COMP[x][::-1].copy()

    def place(k=None, first=False, last=False):
        """a place of far block k (any block without k); first, last: the one that lies first or last in the genome"""
        places = blocks[int(rng.integers(0, len(blocks))) if k is None else k]
        if first or last:
            return min(places) if first else max(places)
        return places[int(rng.integers(0, len(places)))]

    for k in range(n):
        kind = KINDS[k % len(KINDS)]
        if kind == "same_strand" and rng.random() < 0.5:
            kind_pos = "ordinary_short"
        else:
            kind_pos = kind
        b = None
        if kind_pos in ("in_block", "same_strand", "other_block"):
            c, s0 = place()
            fl = int(rng.integers(L + 20, BLOCK - 40))
            s = s0 + int(rng.integers(0, BLOCK - fl))
        elif kind_pos == "fill":
            # first mate where its best hit comes late in a long list: in one copy of the family, or in the last place of a block
            # with four copies; the second in a block with two copies, mostly in its first place.  The first end's best hit then
            # has an index that the second end's list of three does not reach, and the second end's first score leads its list
            if rng.random() < 0.7:
                c, s0 = family[int(rng.integers(0, len(family)))]
                s = s0 + int(rng.integers(0, FAM - L))
            else:
                c, s0 = place(int(rng.integers(11, 16)), last=rng.random() < 0.8)
                s = s0 + int(rng.integers(0, BLOCK - L))
            fl = L
            c2, s2 = place(int(rng.integers(3, 8)), first=rng.random() < 0.8)
            s2 += int(rng.integers(0, BLOCK - L))
            b = rc(cs[c2][s2:s2 + L])
        elif kind_pos in ("near_left", "near_right"):
            c, s0, d = near[int(rng.integers(0, len(near)))]
            inside = s0 + int(rng.integers(min(0, NEAR - L), max(0, NEAR - L) + 1))     # where the mate in the copy starts
            if kind_pos == "near_left":     # the other mate lies to the left of both copies
                s = s0 - int(rng.integers(L + 50, L + 200))
                fl = inside + L - s
            else:                           # ... to the right of both
                s = inside
                fl = int(rng.integers(d + NEAR + 20, d + 400)) + L
        elif kind_pos == "limits":
            dist = narrow[n_lim % 4] if (n_lim // 4) % 2 == 0 else limits[(n_lim // 8) % len(limits)]
            n_lim += 1
            c, fl = int(rng.integers(0, NC)), L + dist
            s = int(rng.integers(50, 900 if fl > 2000 else CL - fl - 50))
        elif kind_pos == "family":
            c, s0 = family[int(rng.integers(0, len(family)))]
            fl = int(rng.integers(L + 20, FAM - 20))
            s = s0 + int(rng.integers(0, FAM - fl))
        elif kind_pos == "ordinary_short":
            c, fl = int(rng.integers(0, NC)), int(rng.integers(L + 20, L + max_dist))
            s = int(rng.integers(50, CL - fl - 50))
        else:                               # unrelated, ordinary: spot distances up to about max_dist + 400
            c, fl = int(rng.integers(0, NC)), int(rng.integers(L + 20, L + max_dist + 400))
            s = int(rng.integers(50, CL - fl - 50))
        gseq = cs[c]
        if kind_pos == "family" and rng.random() < 0.5:
            # read the common sequence, not one copy of it: every copy is then equally far from the read
            gseq, s = g["fam_seq"], s - s0
        a = gseq[s:s + L].copy()
        if b is None:
            b = rc(gseq[s + fl - L:s + fl])
        if kind == "same_strand":
            b = rc(b)
        elif kind == "unrelated":
            c2, s2 = int(rng.integers(0, NC)), int(rng.integers(50, CL - L - 50))
            b = rc(cs[c2][s2:s2 + L])
        elif kind == "other_block":
            c2, s2 = place()
            s2 += int(rng.integers(0, BLOCK - L))
            b = rc(cs[c2][s2:s2 + L])
        assert len(a) == L and len(b) == L, (kind, len(a), len(b))
        if kind != "limits":
            for x in (a, b):
                _substitute(x, int(rng.integers(0, 9)), rng)
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a.tobytes())
        r2.append(b.tobytes())
        kinds.append(kind)
    return r1, r2, kinds


@functools.lru_cache(maxsize=None)
def reads(L=100, seed=READ_SEED, n=PAIRS):
    """-> (buf1, len1, buf2, len2) as the mappers take them"""
    r1, r2, _ = read_ends(genome(), seed + L, n, L)
    return refio.pack_reads(r1) + refio.pack_reads(r2)


# --------------------------------------------------------------------------------------------------------------------
# the selection, restated
# --------------------------------------------------------------------------------------------------------------------
# mapping classes (the reference's enum, pemapper.c:44-52)
UNIQUE_MATE, UNIQUE_SLIP, UNIQUE_SINGLE, UNIQUE_MIS, NON_MATE, NON_MIS, FRAG_MIS, NON_NO, NEITHER_MAP = range(9)
GAP_OPEN = 2.0         # gopen_penalty, pemapper.c:2039


def _hits(d):
    """one end's debug record -> plain lists (spot, orient, score, coordinate a traced hit would report)"""
    if d is None:
        return [], [], [], []
    n = int(d["n_hits"])
    coord = (d["win_start"][:n].astype(np.int64) + d["start"][:n, 1] + 1) & 0xFFFFFFFF
    return d["spot"][:n].tolist(), d["orient"][:n].tolist(), d["score"][:n].tolist(), coord.tolist()


def _reaches(score, good, variant):
    return score > good if variant == "good_gt" else score >= good


def _alone(scores, length, min_align, variant):
    """an end whose mate has no hit at all: the best score that reaches the threshold wins if no later hit ties with it"""
    good = length * min_align * 1.0
    top, ties, best = -GAP_OPEN * length, 0, None
    for i, s in enumerate(scores):
        if s > top and _reaches(s, good, variant):
            top, ties, best = s, 1, i
        elif abs(s - top) < 0.0001 and ties > 0:
            ties += 1
    if ties == 0:
        return NEITHER_MAP, None
    return (UNIQUE_SINGLE, best) if ties == 1 else (NON_NO, None)


def _first_best(scores):
    """index of the first maximum, as a scan that only moves on a strictly greater score finds it"""
    return max(range(len(scores)), key=lambda i: (scores[i], -i))


def _tie_count(scores, against):
    """the reference's running count beside its scan for the best: reset to 1 whenever the scan moves, and raised by every other hit
    that comes within 0.0001 of against(best so far) -- 0 or 1 therefore means that the best stands alone"""
    best, count = 0, 0
    for i in range(1, len(scores)):
        if scores[i] > scores[best]:
            best, count = i, 1
        elif scores[i] - against(best) > -0.0001:
            count += 1
    return count


def select_py(d1, d2, l1, l2, params, variant=None):
    """d1, d2: the oracle's debug records of the two ends (d2 None when unpaired), l1, l2 their lengths,
    params = (min_dist, max_dist, min_align) -> (class, m1, m2)"""
    return _select(_hits(d1), _hits(d2), l1, l2, params, variant)


def _select(h1, h2, l1, l2, params, variant):
    min_dist, max_dist, min_align = params
    sp1, or1, sc1, co1 = h1
    sp2, or2, sc2, co2 = h2
    if not sc1 and not sc2:
        return NEITHER_MAP, 0, 0
    if not sc2:
        cls, w = _alone(sc1, l1, min_align, variant)
        return cls, (0 if w is None else co1[w]), 0
    if not sc1:
        cls, w = _alone(sc2, l2, min_align, variant)
        return cls, 0, (0 if w is None else co2[w])
    good1, good2 = l1 * min_align * 1.0, l2 * min_align * 1.0

    # proper pairs: both scores reach the threshold, opposite strands, spot distance inside the limits
    def proper(i, j):
        dist = abs(sp1[i] - sp2[j])
        lo = dist > min_dist if variant == "min_gt" else dist >= min_dist
        hi = dist < max_dist if variant == "max_lt" else dist <= max_dist
        return lo and hi and (variant == "no_orient" or or1[i] != or2[j])
    cand = [(i, j) for i in range(len(sc1)) if _reaches(sc1[i], good1, variant)
            for j in range(len(sc2)) if _reaches(sc2[j], good2, variant) if proper(i, j)]
    if cand:
        # in list order: a pair more than 0.001 better starts again; one within 0.001 counts, and counts as a slip of the leading
        # pair when it shares a hit with it
        lead, total, count, slips = None, -1e5, 0, 0
        for i, j in cand:
            gain = sc1[i] + sc2[j] - total
            if gain > 0.001:
                lead, total, count, slips = (i, j), sc1[i] + sc2[j], 1, 1
            elif gain > -0.001:
                count += 1
                if variant != "no_slip" and (i == lead[0] or j == lead[1]):
                    slips += 1
        if count == 1:
            return UNIQUE_MATE, co1[lead[0]], co2[lead[1]]
        if slips == count:
            return UNIQUE_SLIP, co1[lead[0]], co2[lead[1]]
        return NON_MATE, 0, 0

    # no proper pair: each end on its own merits
    b1, b2 = _first_best(sc1), _first_best(sc2)
    alone1 = _tie_count(sc1, lambda best: sc1[best]) < 2
    # the second end's ties are measured against ITS score at the FIRST end's best index (the reference's quirk), and a list that
    # is too short for that index answers -1.0 there
    if variant == "best2":
        against = lambda best: sc2[best]
    elif variant == "clamp":
        against = lambda best: sc2[min(b1, len(sc2) - 1)]
    else:
        against = lambda best: sc2[b1] if b1 < len(sc2) else -1.0
    ok1 = _reaches(sc1[b1], good1, variant)
    ok2 = _reaches(sc2[b2], good2, variant) and _tie_count(sc2, against) < 2
    if ok1 and alone1:
        return (UNIQUE_MIS, co1[b1], co2[b2]) if ok2 else (UNIQUE_SINGLE, co1[b1], 0)
    return (UNIQUE_SINGLE, 0, co2[b2]) if ok2 else (NON_MIS, 0, 0)


# --------------------------------------------------------------------------------------------------------------------
# parameter sets and the oracle's results for them
# --------------------------------------------------------------------------------------------------------------------
def threshold_pair(L, score):
    """-> (a, b): a = the largest double with L * a * 1.0 == score (None if there is none), b = the smallest double above a for
    which L * b * 1.0 exceeds score"""
    a = score / L
    on = [x for x in (np.nextafter(a, 0.0), a, np.nextafter(a, 1.0)) if L * float(x) * 1.0 == score]
    if not on:
        return None, None
    a = float(on[-1])
    while L * float(np.nextafter(a, 1.0)) * 1.0 == score:
        a = float(np.nextafter(a, 1.0))
    return a, float(np.nextafter(a, 1.0))


@functools.lru_cache(maxsize=None)
def score_on_threshold(L):
    """the most frequent score between 0.9 L and L in the oracle's hit lists of the narrow run that some min_align hits exactly
    -> (score, min_align on it, min_align one double above)"""
    import collections
    base = _run(L, True, NARROW[0], NARROW[1], 0.85)
    tally = collections.Counter()
    for d in base["d"]:
        nh = d["n_hits"]
        for i in np.nonzero(nh)[0]:
            for s in d["score"][i, :nh[i]].tolist():
                if 0.9 * L < s < L:
                    tally[s] += 1
    for s, _ in tally.most_common():
        a, b = threshold_pair(L, s)
        if a is not None:
            return s, a, b
    raise AssertionError("no score that a threshold can hit")


def set_params(name):
    """-> dict(L, paired, min_dist, max_dist, min_align)"""
    L = 150 if name.endswith("150") else 100
    p = dict(L=L, paired=not name.startswith("single"), min_dist=NARROW[0], max_dist=NARROW[1], min_align=0.85)
    key = name[:-3] if name.endswith("150") else name
    if key == "baseline":
        p.update(min_dist=0, max_dist=500)
    elif key == "empty":
        p.update(min_dist=301, max_dist=300)
    elif key == "zero":
        p.update(min_dist=0, max_dist=0)
    elif key == "wide":
        p.update(min_dist=0, max_dist=5000)
    elif key in ("on_score", "single_on"):
        p.update(min_align=score_on_threshold(L)[1])
    elif key in ("above_score", "single_above"):
        p.update(min_align=score_on_threshold(L)[2])
    else:
        assert key == "narrow", name
    return p


PAIRED_SETS = ("baseline", "narrow", "on_score", "above_score", "empty", "zero", "wide", "on_score150")
SINGLE_SETS = ("single_on", "single_above")
SETS = PAIRED_SETS + SINGLE_SETS


def _run(L, paired, min_dist, max_dist, min_align):
    b1, l1, b2, l2 = reads(L)
    o = oracle_py.Oracle(index(), paired=paired, min_dist=min_dist, max_dist=max_dist, min_align=min_align)
    m1, m2, mt, d1, d2 = o.map_batch(b1, l1, b2 if paired else None, l2 if paired else None, debug=True, threads=8)
    return dict(m1=m1, m2=m2, mt=mt, d=(d1, d2) if paired else (d1,), counts=o.counts().copy(), ins=sorted(o.insertions()),
                summary=o.summary().copy())


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's results for one set on an empty pileup (computed once, shared by the tests, never modified)"""
    p = set_params(name)
    return _run(p["L"], p["paired"], p["min_dist"], p["max_dist"], p["min_align"])


@functools.lru_cache(maxsize=None)
def _hit_lists(name):
    e = expected(name)
    d1 = e["d"][0]
    d2 = e["d"][1] if len(e["d"]) == 2 else [None] * len(d1)
    return [(_hits(a), _hits(b)) for a, b in zip(d1, d2)]


@functools.lru_cache(maxsize=None)
def restated(name, variant=None):
    """select_py over every read of a set -> rows (class, m1, m2); kept, not to be modified"""
    p = set_params(name)
    _, l1, _, l2 = reads(p["L"])
    prm = (p["min_dist"], p["max_dist"], p["min_align"])
    out = np.zeros((len(l1), 3), np.int64)
    for i, (h1, h2) in enumerate(_hit_lists(name)):
        out[i] = _select(h1, h2, int(l1[i]), int(l2[i]), prm, variant)
    return out
