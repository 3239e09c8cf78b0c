"""Planted pileup columns for the per-site caller (pecall_site.hip.h; call_single_base of the reference, pecaller.c:1207-1691).  Shared by
test_site_cases_cpu.py, test_gpu_site_cases.py and tests/golden/make_golden_pecall_edges.py; a plain module like pair_cases.py.

  cases(N, dom)    the families below for N samples, each a list of (name, reads [N][6] uint16, chrom byte); exact counts, no draws.
                   dom = the reference base of every family, or None: family k gets base k % 4
  arrays(N)        all families of N in one array, every planted column followed by two plain reference columns (a wave's piece of eight
                   columns then mixes kinds), -> dict(reads, dom, chrom, family, name, planted)
  expected(N, run) the oracle on arrays(N) under RUNS[run] (three (threshold, theta) pairs, haploid, chromosome bytes), computed once and kept
  reference(N)     the unmodified reference's printed rows for the planted columns of 8 and 129 samples (tests/golden/pecall_edges*)
  hand_off(...)    which columns the small beam hands to the beam search, from the oracle's pass-1 statistics

Sample counts (SIZES): 3 takes the single-pass rule N < 4; 8, 64 one chunk; 128 two chunks and the last size of the small beam's first
form (4 unsettled samples); 129 the first of its second form (16 unsettled samples); 257 five chunks' worth in the eight-chunk kernel.
Carriers go to lanes(N): the first lane, the last one and both sides of every boundary between chunks of 64 samples; a family's
columns take these lanes in turn, and the column "all_lanes" of the family "types" has a carrier in every one of them.

A plain sample has DEPTH reads of the reference base.  An insertion read (allele 5) is counted on top of the base it follows, so a
sample with an insertion keeps its reference reads.

Families, and what each is for:

  depth_floor   samples of min_depth and min_depth + 1 reads for both floors (diploid: a sample is called from 3 reads, haploid from 2),
                reference and carrying an alternative base: `tot > min_depth` in the set-up, in every kernel's `deep` mask and in the
                fallback configuration.
  site_filters  every sample 8 reads but one with 7 (total depth 8 N - 1: average_depth < 8 drops the column) and all with 8 (kept);
                h samples with 12 reads and the others with 7 for h on both sides of N / 2 (sample_count < 0.5 N drops the column);
                each with chromosome bytes 0, 2 (chrY: exempt from the second filter), 16 and 18 (HAPLOID forced for the column).
  scale         samples of 9, 10, 11, 99, 100 and 101 reads, reference and heterozygous: the clamp of the Dirichlet scale to 10 .. 100
                (the row of the ta table in pcs_fast_kernel).
  indel         2 and 3 reads of a deletion and of an insertion in a reference sample (an indel genotype needs three), heterozygous and
                homozygous deletions and insertions, and a column in which all samples but one are homozygous deletions: the
                fallback's best_hom > 3 -> reference base.
  table_edges   a sample of 1,446 / 1,447 reads (the head of the ln n! table: tot + 601 >= 2048 sends the column to the deep list, or
                beyond 128 samples to the beam search), 9,999 / 10,000 / 10,001 (the table's end: the log formula above it), 65,535 on one
                allele and on two; each alone in its column and beside a heterozygous carrier.
  types         SNP, DEL, INS; LOW with low_base = max (8, 0.4 average_depth) decided by either argument and the carrier's depth on
                both sides of it; MULTIALLELIC with two and three alternative alleles in different chunks; MESS with the off-target
                share of the reads at 0.15 exactly (not MESS) and one read above: the reductions of pcs_write_site over the chunks.
  small_beam    what pcs_mini_core hands off and what it keeps: MAXU and MAXU + 1 unsettled samples (25 + 5 reads: the reference
                homozygote is best by less than 2.31 nats), a heterozygous carrier whose margin is above a shallow settled sample's
                ("early"), carriers of 7 reads in 30 (they come last in the order, and the list grows), shallow carriers, and sixteen
                samples of 4 + 2 reads, which under the weak prior take the list to the cut at 514 configurations.
                What these reach depends on threshold and theta; test_site_cases_cpu.py asserts it from the oracle's statistics.
  ties          identical read vectors in several samples (equal margins: the order is by sample index) and two or four identical
                heterozygous carriers (configurations with equal posteriors: the sort must be stable).
"""
import functools

import numpy as np

import oracle_py

SIZES = (3, 8, 64, 128, 129, 257)
DEPTH = 30
FAMILIES = ("depth_floor", "site_filters", "scale", "indel", "table_edges", "types", "small_beam", "ties")
# (threshold, theta) of the runs: the defaults; a weak prior and a low threshold (long lists, one pass); the strictest pair
PARAMS = ((0.95, 0.001), (0.5, 0.5), (0.999999, 1e-10))
WEAK = 5                        # reads off the reference base, of DEPTH, that leave the reference homozygote best by less than 2.31 nats
SOFT = 7                        # ... that make the heterozygote best, by less than a plain sample's margin


def maxu(N):
    """unsettled samples the small beam takes (PCS_MINI_U; PcsMini::MAXU beyond 128 samples)"""
    return 4 if N <= 128 else 16


def lanes(N):
    s = {0, N - 1}
    for b in range(64, N + 1, 64):
        s.add(b - 1)
        if b < N:
            s.add(b)
    return sorted(s)


class _Family:
    def __init__(self, N, dom):
        self.N, self.dom, self.cols, self.turn = N, dom, [], 0
        self.alt = [(dom + k) % 4 for k in (1, 2, 3)]
        self.lanes = lanes(N)

    def lane(self, skip=()):
        """the next lane of lanes(N) in turn (not one of `skip`)"""
        for _ in range(len(self.lanes) + 1):
            v = self.lanes[self.turn % len(self.lanes)]
            self.turn += 1
            if v not in skip:
                return v
        return next(i for i in range(self.N) if i not in skip)

    def plain(self, depth=DEPTH):
        r = np.zeros((self.N, 6), np.int64)
        r[:, self.dom] = depth
        return r

    def put(self, r, i, ref=0, **alleles):
        """sample i: `ref` reads of the reference base and a1 / a2 / a3 / dele / ins reads of the alternatives"""
        r[i] = 0
        r[i, self.dom] = ref
        for k, v in alleles.items():
            r[i, {"a1": self.alt[0], "a2": self.alt[1], "a3": self.alt[2], "dele": 4, "ins": 5}[k]] += v

    def add(self, name, r, chrom=0):
        assert r.min() >= 0 and r.max() <= 65535
        self.cols.append((name, r.astype(np.uint16), chrom))


def _depth_floor(f):
    for kind, alleles in (("ref", {}), ("alt", {"a1": 1})):
        # samples of 1, 2, 3 reads (and 0) in one column, in the lanes in turn; the carrier's reads are all the alternative base
        r = f.plain()
        used = []
        for d in (0, 1, 2, 3):
            if len(used) + 1 >= f.N:
                break
            i = f.lane(used)
            used.append(i)
            f.put(r, i, ref=0 if alleles else d, **{k: d for k in alleles})
        f.add("mixed_%s" % kind, r)
        for d in (1, 2, 3):
            r = f.plain()
            i = f.lane()
            f.put(r, i, ref=0 if alleles else d, **{k: d for k in alleles})
            f.add("%s_%d" % (kind, d), r)
    # every sample at the floor but one / every sample one above it
    for d in (2, 3):
        r = f.plain(d)
        f.put(r, f.lane(), ref=9 * f.N)         # (the average depth stays above 8)
        f.add("all_%d" % d, r)


def _site_filters(f):
    N = f.N
    for chrom in (0, 2, 16, 18):
        for short in (1, 0):
            r = f.plain(8)
            if short:
                f.put(r, f.lane(), ref=7)
            f.add("total_%s_c%d" % ("8n-1" if short else "8n", chrom), r, chrom)
        for h in sorted({N // 2 - 1, N // 2, (N + 1) // 2, (N + 1) // 2 + 1}):
            if h < 1 or h > N:
                continue
            # h samples of 12 reads, the last of them a homozygous carrier, the others 7; from the last lane down when chrom has bit 1
            r = f.plain(7)
            who = list(range(h)) if not (chrom & 2) else list(range(N - h, N))
            for i in who:
                f.put(r, i, ref=12)
            f.put(r, who[-1], a1=12)
            f.add("count_%d_c%d" % (h, chrom), r, chrom)


def _scale(f):
    for d in (9, 10, 11, 99, 100, 101):
        r = f.plain()
        f.put(r, f.lane(), ref=d)
        f.add("ref_%d" % d, r)
        r = f.plain()
        f.put(r, f.lane(), ref=d - d // 2, a1=d // 2)
        f.add("het_%d" % d, r)
    r = f.plain()
    used = []
    for d in (9, 10, 11, 99, 100, 101):
        if len(used) + 1 >= f.N:
            break
        i = f.lane(used)
        used.append(i)
        f.put(r, i, ref=d - 3, a2=3)
    f.add("all_depths", r)


def _indel(f):
    for k in (2, 3):
        r = f.plain()
        f.put(r, f.lane(), ref=DEPTH, dele=k)
        f.add("del_reads_%d" % k, r)
        r = f.plain()
        f.put(r, f.lane(), ref=DEPTH, ins=k)
        f.add("ins_reads_%d" % k, r)
        # nothing but the indel reads beside a shallow reference: the genotype would be best, were it allowed
        r = f.plain()
        f.put(r, f.lane(), ref=1, dele=k)
        f.add("del_only_%d" % k, r)
        r = f.plain()
        f.put(r, f.lane(), ref=3, ins=k)
        f.add("ins_only_%d" % k, r)
    for name, kw in (("het_del", dict(ref=15, dele=15)), ("hom_del", dict(ref=0, dele=30)), ("het_ins", dict(ref=30, ins=15)),
                     ("hom_ins", dict(ref=30, ins=30))):
        r = f.plain()
        f.put(r, f.lane(), **kw)
        f.add(name, r)
    # two heterozygous insertions: configurations with equal posteriors (the crude families of the issue found them here)
    if f.N >= 4:
        r = f.plain()
        a = f.lane()
        f.put(r, a, ref=30, ins=15)
        f.put(r, f.lane((a,)), ref=30, ins=15)
        f.add("het_ins_pair", r)
    # nearly every sample a homozygous deletion
    r = f.plain()
    keep = f.lane()
    for i in range(f.N):
        if i != keep:
            f.put(r, i, ref=0, dele=30)
    f.add("all_hom_del", r)
    if f.N >= 8:
        r = f.plain()
        for i in range(f.N):
            if i % 8:
                f.put(r, i, ref=0 if i % 3 else 15, dele=30 if i % 3 else 15)
        f.add("most_del", r)


def _table_edges(f):
    for d in (1446, 1447, 9999, 10000, 10001, 65535, (65535, 65535)):
        for beside in (0, 1):
            r = f.plain()
            i = f.lane()
            if isinstance(d, tuple):
                f.put(r, i, ref=d[0], a1=d[1])
            else:
                f.put(r, i, ref=d)
            if beside and f.N > 1:
                f.put(r, f.lane((i,)), ref=15, a2=15)
            f.add("%s_%s" % ("x".join(map(str, d)) if isinstance(d, tuple) else d, "carrier" if beside else "alone"), r)


def _low_edge(N, base):
    """the deepest carrier that is still at or below low_base = 0.4 average_depth, the others at `base` reads: c <= 0.4 (base (N - 1) + c) / N"""
    c = 0
    while 5 * (c + 1) * N <= 2 * (base * (N - 1) + c + 1):
        c += 1
    return c


def _types(f):
    N = f.N
    for name, kw in (("snp", dict(ref=15, a1=15)), ("del", dict(ref=15, dele=15)), ("ins", dict(ref=30, ins=12)), ("hom_snp", dict(a3=30))):
        r = f.plain()
        f.put(r, f.lane(), **kw)
        f.add(name, r)
    r = f.plain()
    for i in f.lanes:
        f.put(r, i, ref=15, a1=15)
    f.add("all_lanes", r)
    # LOW: low_base = 8 (0.4 x 12 < 8), carrier of 8 and of 9 reads; low_base = 0.4 average_depth (samples of 50 reads), carrier at and above it
    for c in (8, 9):
        r = f.plain(12)
        f.put(r, f.lane(), a1=c)
        f.add("low8_%d" % c, r)
    c = _low_edge(N, 50)
    for k in (0, 1):
        r = f.plain(50)
        f.put(r, f.lane(), a1=c + k)
        f.add("low_avg_%s" % ("at" if k == 0 else "above"), r)
    # MULTIALLELIC: two and three alternative alleles, the carriers as far apart as the lanes allow
    far = [0, N - 1, N // 2] if N >= 3 else [0]
    for n_alt in (2, 3):
        r = f.plain()
        for k in range(min(n_alt, len(far))):
            f.put(r, far[k], ref=15, **{"a%d" % (k + 1): 15})
        f.add("multi_%d" % n_alt, r)
    r = f.plain()
    f.put(r, far[0], ref=15, a1=15)
    f.put(r, far[1], ref=15, dele=15)
    f.add("multi_snp_del", r)
    # MESS: samples of 40 reads, a homozygous carrier, error reads of the two other bases dealt round the reference samples until the
    # off-target share is 6 N / 40 N = 0.15 (not above: no MESS), and one more
    for extra in (0, 1):
        r = f.plain(40)
        who = f.lane()
        f.put(r, who, a1=40)
        others = [i for i in range(N) if i != who]
        for k in range(6 * N + extra):
            i = others[k % len(others)]
            a = f.alt[1 + (k // len(others)) % 2]
            r[i, f.dom] -= 1
            r[i, a] += 1
        f.add("mess_%s" % ("at" if extra == 0 else "over"), r)


def _small_beam(f):
    N = f.N
    U = maxu(N)
    # unsettled by error reads: 1, MAXU - 1, MAXU, MAXU + 1 samples (as many as there are)
    for n in (1, U - 1, U, U + 1):
        if n >= N:
            continue
        r = f.plain()
        used = []
        for _ in range(n):
            i = f.lane(used)
            used.append(i)
            f.put(r, i, ref=DEPTH - WEAK, a1=WEAK)
        f.add("weak_%d" % n, r)
    # carriers that come last in the order (SOFT reads of 30): 1 .. 3 of them, the list grows; and beside weak samples
    for n in (1, 2, 3):
        if n >= N:
            continue
        r = f.plain()
        used = []
        for _ in range(n):
            i = f.lane(used)
            used.append(i)
            f.put(r, i, ref=DEPTH - SOFT, a1=SOFT)
        f.add("soft_%d" % n, r)
        if n + 2 < N:
            r = r.copy()
            for _ in range(2):
                i = f.lane(used)
                used.append(i)
                f.put(r, i, ref=DEPTH - WEAK, a2=WEAK)
            f.add("soft_%d_weak_2" % n, r)
    # different alternatives in the soft carriers: more alleles, more configurations
    if N >= 4:
        r = f.plain()
        used = []
        for k in range(3):
            i = f.lane(used)
            used.append(i)
            f.put(r, i, ref=DEPTH - SOFT, **{"a%d" % (k + 1): SOFT})
        f.add("soft_3_alleles", r)
        # ... and a shallow reference sample, unsettled and last in the order: its expansion starts from more than four configurations
        r = r.copy()
        f.put(r, f.lane(used), ref=8)
        f.add("soft_3_alleles_ref_8", r)
    # a carrier whose margin is above a settled sample's: a clear heterozygote beside a sample of 4 reads
    r = f.plain()
    a = f.lane()
    f.put(r, a, ref=15, a1=15)
    if N > 2:
        f.put(r, f.lane((a,)), ref=4)
    f.add("early_het", r)
    # the same with a carrier of SOFT + 1 reads beside a settled sample of 19: the all-reference configuration stays in the list
    if N > 2:
        r = f.plain()
        a = f.lane()
        f.put(r, a, ref=DEPTH - SOFT - 1, a1=SOFT + 1)
        f.put(r, f.lane((a,)), ref=19)
        f.add("early_soft", r)
    # shallow carriers: 4 .. 8 reads, half of them the alternative base
    for d in (4, 6, 8):
        r = f.plain()
        f.put(r, f.lane(), ref=d - d // 2, a1=d // 2)
        f.add("shallow_het_%d" % d, r)
    # sixteen shallow samples with 2 of 6 reads off the reference base: under the weak prior every one of them doubles the list, up to the
    # cut at max_configs = 514
    if N >= 64:
        r = f.plain()
        for k in range(16):
            f.put(r, (k * 37) % N, ref=4, a1=2)
        f.add("shallow_x16", r)
    # a homozygous carrier: the cut leaves its configuration alone, which has two alleles (the fallback adds the homozygous one)
    r = f.plain()
    f.put(r, f.lane(), a1=DEPTH)
    f.add("hom_alt", r)
    r = f.plain()
    f.put(r, f.lane(), a1=5)
    f.add("hom_alt_5", r)


def _ties(f):
    N = f.N
    # every sample the same (all margins equal); the same with two depths alternating
    f.add("all_equal", f.plain())
    r = f.plain()
    r[1::2, f.dom] = 12
    f.add("two_depths", r)
    # identical weak samples and identical carriers in all the lanes
    for name, kw in (("weak", dict(ref=DEPTH - WEAK, a1=WEAK)), ("het", dict(ref=15, a1=15)), ("soft", dict(ref=DEPTH - SOFT, a1=SOFT))):
        for n in (2, 4):
            if n >= N:
                continue
            r = f.plain()
            used = []
            for _ in range(n):
                i = f.lane(used)
                used.append(i)
                f.put(r, i, **kw)
            f.add("%s_x%d" % (name, n), r)
    # symmetric carriers of different alleles
    if N >= 3:
        r = f.plain()
        f.put(r, 0, ref=15, a1=15)
        f.put(r, N - 1, ref=15, a2=15)
        f.add("het_a1_a2", r)


_BUILD = dict(depth_floor=_depth_floor, site_filters=_site_filters, scale=_scale, indel=_indel, table_edges=_table_edges, types=_types,
              small_beam=_small_beam, ties=_ties)


def cases(N, dom=None):
    """-> {family: [(name, reads [N][6] uint16, chrom byte), ...]} (module docstring); dom = every family's reference base, None = family k's is k % 4"""
    out = {}
    for k, fam in enumerate(FAMILIES):
        f = _Family(N, k % 4 if dom is None else dom)
        _BUILD[fam](f)
        out[fam] = f.cols
    return out


def family_dom(k_or_name, dom=None):
    k = FAMILIES.index(k_or_name) if isinstance(k_or_name, str) else k_or_name
    return k % 4 if dom is None else dom


@functools.lru_cache(maxsize=None)
def arrays(N):
    """all families in one array: planted column, two plain reference columns, planted column, ... and a column with a reference N every
    37th (more than 256 columns at every N: two chunks under PECALL_CHUNK_LOG2=8)"""
    cs = cases(N)
    reads, dom, chrom, family, name, planted = [], [], [], [], [], []
    for fam in FAMILIES:
        d = family_dom(fam)
        for nm, r, ch in cs[fam]:
            for kind in (1, 0, 0):
                if len(reads) % 37 == 36:
                    reads.append(np.full((N, 6), 3, np.uint16))
                    dom.append(14)
                    chrom.append(0)
                    family.append("")
                    name.append("ref_n")
                    planted.append(False)
                if kind:
                    reads.append(r)
                else:
                    p = np.zeros((N, 6), np.uint16)
                    p[:, d] = DEPTH
                    reads.append(p)
                dom.append(d)
                chrom.append(ch if kind else 0)
                family.append(fam)
                name.append(nm if kind else "plain")
                planted.append(bool(kind))
    out = dict(reads=np.array(reads, np.uint16), dom=np.array(dom, np.uint8), chrom=np.array(chrom, np.uint8), family=np.array(family),
               name=np.array(name), planted=np.array(planted))
    for v in out.values():
        v.setflags(write=False)
    return out


# the runs of expected(): (threshold, theta) of PARAMS by index, then haploid and every chromosome byte in turn at the defaults
RUNS = dict(default=dict(), weak_prior=dict(threshold=PARAMS[1][0], theta=PARAMS[1][1]), strict=dict(threshold=PARAMS[2][0], theta=PARAMS[2][1]),
            haploid=dict(haploid=True), chrom_turn=dict(chrom="turn"))


def run_chrom(N, run):
    """the chromosome bytes of a run: the planted ones, or (run "chrom_turn") 0-3 with and without bit 4 in turn over them"""
    a = arrays(N)
    if RUNS[run].get("chrom") != "turn":
        return a["chrom"]
    turn = np.array([0, 1, 2, 3, 16, 17, 18, 19], np.uint8)
    return (a["chrom"] | turn[np.arange(len(a["dom"])) // 3 % 8]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def expected(N, run="default"):
    """the oracle on arrays(N) under RUNS[run] -> dict(call, p, type, ac, passes, stats); computed once per (N, run), read-only"""
    a = arrays(N)
    kw = {k: v for k, v in RUNS[run].items() if k != "chrom"}
    call, p, typ, ac, npass = oracle_py.call_sites(a["reads"], a["dom"], chrom=run_chrom(N, run), **kw)
    out = dict(call=call, p=p, type=typ, ac=ac, passes=npass, stats=dict(oracle_py.call_sites.stats))
    for v in list(out.values())[:5] + list(out["stats"].values()):
        v.setflags(write=False)
    return out


def hand_off(N, stats):
    """pcs_mini_core's hand-off rules (the comment above PCS_MINI_U) on the oracle's pass-1 statistics -> dict of boolean arrays, one per
    rule, over the columns that reach the small beam at all (a pass was run and a sample is unsettled); "changed" = more than one pass"""
    live = (stats["passes"] >= 1) & (stats["unset"] > 0)
    return dict(live=live, many=live & (stats["unset"] > maxu(N)), early=live & (stats["early"] > 0), long=live & (stats["pre_list"] > 4),
                no_hom=live & (stats["no_hom"] > 0), changed=live & (stats["passes"] > 1))


# the reference's own rows for the planted columns of 8 and 129 samples (tests/golden/make_golden_pecall_edges.py): run -> call_sites' arguments
REFERENCE_RUNS = {"": dict(threshold=0.95, theta=0.001), "_t99": dict(threshold=0.99, theta=0.01), "_hap": dict(threshold=0.95, theta=0.001, haploid=True)}


@functools.lru_cache(maxsize=None)
def reference(N):
    """-> dict(reads, dom, ref, pos, family, name, rows = {run: (base rows, snp rows) by 1-based position}); the samples are in the order of
    the reference's columns (its directory order), so the planted lanes are permuted: columns of their own, not those of arrays(N)"""
    import gzip
    import os
    import refio
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    z = np.load(os.path.join(gold, "pecall_edges%d.npz" % N))
    names = [str(x) for x in z["names"]]
    perm = [names.index(str(c)) for c in z["columns"]]
    _, seqs = refio.read_fasta(os.path.join(gold, "g1.fa.gz"))
    ref = np.concatenate(seqs)[z["pos"]]
    dom = np.array([b"ACGT".index(bytes([c])) for c in ref], np.uint8)
    rows = {}
    for run in REFERENCE_RUNS:
        base = gzip.open(os.path.join(gold, "pecall_edges%d%s.base.txt.gz" % (N, run)), "rt").read().split("\n")
        snp = open(os.path.join(gold, "pecall_edges%d%s.snp.txt" % (N, run))).read().split("\n")
        rows[run] = ({int(r.split("\t")[1]): r for r in base[1:] if r}, {int(r.split("\t")[1]): r for r in snp[1:] if r})
    return dict(reads=np.ascontiguousarray(z["reads"][:, perm, :]), dom=dom, ref=ref, pos=z["pos"], family=z["family"], name=z["name"], rows=rows)


def reference_mismatches(N, run, call, p, typ, ac):
    """the rows of the reference's .base and .snp text that (call, p, typ, ac) of reference(N)["reads"] would not print the same -> list"""
    import pecall_sites_fixture as fx
    f = reference(N)
    base_rows, snp_rows = f["rows"][run]
    bad = []
    assert len(base_rows) == len(f["pos"])
    for i, pos in enumerate(f["pos"]):
        pos1 = int(pos) + 1
        got = fx.base_row("chr1", pos1, chr(f["ref"][i]), call[i], p[i])
        if got != base_rows[pos1]:
            bad.append((str(f["name"][i]), base_rows[pos1], got))
        got_s = fx.snp_row("chr1", pos1, chr(f["ref"][i]), call[i], p[i], typ[i], ac[i]) if typ[i] > 0 else None
        if got_s != snp_rows.get(pos1):
            bad.append((str(f["name"][i]), snp_rows.get(pos1), got_s))
    return bad
