"""The second way into the banded DP (pm_band_kernel; the bound is derived at PM_BAND_MAXX_ in pecaller_amd/csrc/pemap_sw.hip.h, K3b
in DESIGN.md), restated in Python from the rule and held against the oracle's full DP.  The band is exact when the optimum is at
least mm - 8.  One proof of that is a single diagonal with at most six mismatches; the other is an explicit alignment with ONE gap:
a prefix of the read on diagonal d1 with at most i mismatches, the gap, the rest on diagonal d2 with at most j, both diagonals among
those that hold the whole read (0 .. D = nn - mm).  With p_i[d] / s_j[d] the longest prefix / suffix of diagonal d with at most
i / j mismatches:
  deletion of b = d2 - d1 >= 1 reference bases:       exists iff p_i[d1] + s_j[d2] >= mm,      loss36 = 72 + (b-1) + 48 (i+j)
  insertion of b = d1 - d2, 1 <= b <= 5, read bases:  exists iff p_i[d1] + s_j[d2] >= mm - b,  loss36 = 36 b + 72 + (b-1) + 48 (i+j)
(match +1, mismatch -1/3, gap open 2, gap extend 1/36, in units of 1/36) and the window is admitted iff some loss36 <= 288.  The
kernel knows three mismatches from each end of a diagonal (KNOWN = 2: i, j <= 2).

Asserted: (a) whenever a window is admitted the full DP scores at least mm - loss36 / 36, hence at least mm - 8; (b) each limit is
needed; (c) one diagonal alone never admits; (d) the share of the bench's one-indel reads that the bound admits.  CPU only: this
pins the rule, tests/test_gpu_band_gate.py pins the kernel."""
import functools

import numpy as np
import oracle_py
from test_gapless_rule_cpu import match, edge_windows
from test_gapless_rule3_cpu import stress_windows, two_skips

K = 5                   # the band's half-width beside the diagonals 0 .. D (PM_BAND_K)
LOSS36 = 288            # 8, the margin of the x <= 6 rule
KNOWN = 2               # the kernel's PM_GATE_Y: mismatches known per side beyond the first
MAXX = 6                # PM_BAND_MAXX_
ACGT = np.frombuffer(b"ACGT", np.uint8)
_NEVER = 1 << 20


@functools.lru_cache(maxsize=None)
def _tables(nd, known):
    """-> loss36[i, j, d1, d2] (_NEVER where (d1, d2) is no case) and the read bases the gap takes, ins[d1, d2]"""
    d1, d2 = np.meshgrid(np.arange(nd), np.arange(nd), indexing="ij")
    ij = np.arange(known + 1)[:, None] + np.arange(known + 1)[None, :]
    b_del, b_ins = d2 - d1, d1 - d2
    loss = np.full((known + 1, known + 1, nd, nd), _NEVER, np.int64)
    dele = b_del >= 1
    inse = (b_ins >= 1) & (b_ins <= K)
    loss[:, :, dele] = (72 + (b_del[dele] - 1))[None, None, :] + 48 * ij[:, :, None]
    loss[:, :, inse] = (36 * b_ins[inse] + 72 + (b_ins[inse] - 1))[None, None, :] + 48 * ij[:, :, None]
    return loss, np.where(inse, b_ins, 0)


def mismatches(ref, read, bis=False):
    """[diagonal 0 .. D][read base]: does it mismatch the window there?  (None: no diagonal holds the whole read)"""
    nd = len(ref) - len(read) + 1
    if nd <= 0:
        return None
    idx = np.arange(nd)[:, None] + np.arange(len(read))[None, :]
    return ~match(ref[idx], read[None, :], bis)


def band_gate(ref, read, bis=False, known=KNOWN):
    """-> (admitted, loss36 of the cheapest explicit one-gap alignment that admits, or None)"""
    ne = mismatches(ref, read, bis)
    if ne is None or len(ne) < 2:
        return False, None
    mm = len(read)
    front, back = ne.cumsum(axis=1), ne[:, ::-1].cumsum(axis=1)
    p = np.stack([np.where(front[:, -1] > i, (front > i).argmax(axis=1), mm) for i in range(known + 1)])
    s = np.stack([np.where(back[:, -1] > j, (back > j).argmax(axis=1), mm) for j in range(known + 1)])
    loss, ins = _tables(len(ne), known)
    ok = (p[:, None, :, None] + s[None, :, None, :] >= mm - ins[None, None]) & (loss <= LOSS36)
    if not ok.any():
        return False, None
    return True, int(loss[ok].min())


def xmin(ref, read, bis=False):
    ne = mismatches(ref, read, bis)
    return 99 if ne is None else int(ne.sum(axis=1).min())


def _other(b, rng):
    o = ACGT[ACGT != (b & 0xDF)]
    return o[int(rng.integers(0, len(o)))]


def one_gap_windows(seed, n, bis):
    """reads of 40 .. 71 bases with one gap: a deletion of 1 .. 21 reference bases or an insertion of 1 .. 8 read bases; the gap 9 to
    20 bases from either end or in the middle, every fourth one inside a planted homopolymer or tandem repeat; 0 .. 3 substitutions on
    each side, some directly beside the gap and at the read's first and last base; N and lower case in read and window; every third
    window clipped (1 .. 21 diagonals); bisulfite conversion of the read when asked"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        mm = int(rng.integers(40, 72))
        slack = 21 if k % 3 else int(rng.integers(0, 21))
        alpha = ACGT if k % 5 else ACGT[:2]
        ref = alpha[rng.integers(0, len(alpha), mm + slack + 8)].copy()
        p = (int(rng.integers(9, 21)), mm - int(rng.integers(9, 21)), mm // 2 + int(rng.integers(-3, 4)))[k % 3]
        dele = (k // 3) % 2 == 0
        if dele:
            b = min(1 + (k // 6) % 21, slack)
            d = int(rng.integers(0, slack - b + 1))
        else:
            b = 1 + (k // 6) % 8
            d = int(rng.integers(min(b, slack), slack + 1))       # (a window too narrow for the suffix's diagonal: to be refused)
        if k % 4 == 0:
            unit = alpha[rng.integers(0, len(alpha), int(rng.integers(1, 5)))]
            m = int(rng.integers(8, 17))
            at = max(d + p - int(rng.integers(2, m - 1)), 0)
            ref[at:at + m] = np.tile(unit, m)[:m]
        if dele:
            read = np.concatenate([ref[d:d + p], ref[d + p + b:d + mm + b]]).copy()
            right = p
        else:
            read = np.concatenate([ref[d:d + p], alpha[rng.integers(0, len(alpha), b)], ref[d + p:d + mm - b]]).copy()[:mm]
            right = min(p + b, mm - 1)
        ref = ref[:mm + slack]
        assert len(read) == mm
        for side in (0, 1):
            lo, hi = (0, p) if side == 0 else (right, mm)
            special = ((0, p - 1), (right, mm - 1))[side]
            for t in range(int(rng.integers(0, 4))):
                q = special[t] if t < 2 and rng.random() < 0.4 else int(rng.integers(lo, hi))
                read[q] = _other(read[q], rng)
        if bis:
            conv = (read == ord("C")) & (rng.random(mm) < 0.9)
            read[conv] = ord("T")
        if k % 7 == 0:
            q = int(rng.integers(0, mm))
            read[q] = (ord("N"), ord("n"), read[q] | 0x20)[(k // 7) % 3]
        if k % 9 == 0:
            q = int(rng.integers(0, len(ref)))
            ref[q] = (ord("N"), ref[q] | 0x20, ord("n"))[(k // 9) % 3]
        yield ref, read


def _premise_holds(it, bis, known=KNOWN):
    """(a) on every window of a generator -> windows, admitted, admitted with no diagonal of at most MAXX mismatches"""
    n = adm = fresh = 0
    for ref, read in it:
        n += 1
        ok, loss = band_gate(ref, read, bis, known)
        if not ok:
            assert loss is None
            continue
        assert 72 <= loss <= LOSS36
        mm = len(read)
        score = oracle_py.sw(ref, read, bisulfite=bis)[0]
        assert score >= mm - loss / 36.0 - 1e-9, (ref.tobytes(), read.tobytes(), score, loss)
        assert score >= mm - 8 - 1e-9
        adm += 1
        fresh += xmin(ref, read, bis) > MAXX
    return n, adm, fresh


def test_admitted_windows_score_what_the_explicit_alignment_promises():
    r = _premise_holds(one_gap_windows(20261001, 6000, False), False)
    print("one gap", r)
    assert r[1] > 2500 and r[2] > 1000, r
    # ... and with every mismatch known per side that the bound can use (i + j <= 4), the rule as the issue states it
    r4 = _premise_holds(one_gap_windows(20261001, 3000, False), False, known=4)
    print("one gap, four known", r4)
    assert r4[1] > 1250, r4


def test_admitted_windows_in_bisulfite_mode():
    r = _premise_holds(one_gap_windows(20261002, 6000, True), True)
    print("one gap, bisulfite", r)
    assert r[1] > 2500 and r[2] > 1000, r


def test_premise_on_the_rule_tests_windows():
    for name, it, bis in (("stress", stress_windows(20260301, 8000), False), ("two_skips", two_skips(7, 3000), False),
                          ("edge", edge_windows(77, 8000, False), False), ("edge_bis", edge_windows(78, 8000, True), True)):
        r = _premise_holds(it, bis)
        print(name, r)
        assert r[1] > 100, (name, r)


def _planted(rng, mm, kind):
    """a random window of full width and a read with exactly the gap and the substitutions of `kind`, far from each other"""
    ref = ACGT[rng.integers(0, 4, mm + 21)].copy()
    p = mm // 2
    if kind == "ins6":
        read = np.concatenate([ref[10:10 + p], ACGT[rng.integers(0, 4, 6)], ref[10 + p:10 + mm - 6]]).copy()
        subs = []
    elif kind == "ins5+1":
        read = np.concatenate([ref[10:10 + p], ACGT[rng.integers(0, 4, 5)], ref[10 + p:10 + mm - 5]]).copy()
        subs = [p // 2]
    else:                   # "del+5": one skipped reference base, two substitutions before it and three behind
        read = np.concatenate([ref[10:10 + p], ref[10 + p + 1:10 + mm + 1]]).copy()
        subs = [p // 3, 2 * p // 3, p + (mm - p) // 4, p + (mm - p) // 2, p + 3 * (mm - p) // 4]
    for q in subs:
        read[q] = _other(read[q], rng)
    return ref, read


def test_each_limit_is_needed():
    """(b) a 6-base insertion, an insertion of 5 with one mismatch and a deletion with 5 mismatches are refused, with three mismatches
    known per side and with all of them; and each limit matters: there is such a window whose optimum is below mm - 8"""
    rng = np.random.default_rng(5)
    for kind in ("ins6", "ins5+1", "del+5"):
        below = 0
        for _ in range(60):
            mm = int(rng.integers(60, 90))
            ref, read = _planted(rng, mm, kind)
            for known in (KNOWN, 5):
                assert band_gate(ref, read, False, known) == (False, None), (kind, known, ref.tobytes(), read.tobytes())
            below += oracle_py.sw(ref, read)[0] < mm - 8
        print(kind, "windows with an optimum below mm - 8:", below, "of 60")
        assert below >= 1, kind
    # one step inside each limit the same windows are admitted: 5 inserted bases, 4 with one mismatch, a deletion with 2 + 2
    for kind, drop, loss in (("ins5+1", "sub", 36 * 5 + 72 + 4), ("del+5", "sub", 72 + 48 * 4)):
        mm = 80
        ref, read = _planted(rng, mm, kind)
        p = mm // 2
        q = p // 2 if kind == "ins5+1" else p + 3 * (mm - p) // 4
        read[q] = ref[10 + q] if q < p else ref[10 + q + 1]        # (the substitution put back; behind the deletion the diagonal is 11)
        assert band_gate(ref, read) == (True, loss), kind


def test_one_diagonal_alone_never_admits():
    """(c) d1 = d2 is no case: a read that lies on one diagonal with a short-mismatch prefix and suffix that cover it is not admitted
    by that diagonal -- not in a window with a single diagonal, and not among random ones"""
    rng = np.random.default_rng(8)
    for _ in range(300):
        mm = int(rng.integers(40, 80))
        for slack in (0, 21):
            ref = ACGT[rng.integers(0, 4, mm + slack)].copy()
            d = slack // 2
            read = ref[d:d + mm].copy()
            for q in (mm // 5, 2 * mm // 5, 3 * mm // 5, 4 * mm // 5):          # p_2 + s_2 = 3 mm / 5 + (mm - 1 - 2 mm / 5) >= mm
                read[q] = _other(read[q], rng)
            ne = mismatches(ref, read)[d]
            assert ne.sum() == 4
            assert band_gate(ref, read, False, KNOWN) == (False, None)
            # (with all four known, p_4 = mm on this diagonal: "the whole read, then a gap, then nothing" on a LATER diagonal is a
            # case of the rule and a true, if weak, bound; a window with one diagonal has no later one)
            if slack == 0:
                assert band_gate(ref, read, False, 4) == (False, None)


def test_share_of_the_bench_reads_with_one_indel():
    """(d) 150 bases, 1 % substitutions, one 1-base indel at a uniform position, random reference, full-width windows: of the reads
    without a diagonal of at most six mismatches the bound admits more than half (the model: 0.64 with two mismatches known per
    side, 0.88 with three)"""
    rng = np.random.default_rng(20261020)
    n = 20000
    mm = 150
    already = open_ = adm = adm1 = 0
    for k in range(n):
        ref = ACGT[rng.integers(0, 4, mm + 21)].copy()
        p = int(rng.integers(1, mm))
        if k % 2:
            read = np.concatenate([ref[10:10 + p], ref[11 + p:11 + mm]]).copy()
        else:
            read = np.concatenate([ref[10:10 + p], ACGT[rng.integers(0, 4, 1)], ref[10 + p:10 + mm - 1]]).copy()
        for q in np.nonzero(rng.random(mm) < 0.01)[0]:
            read[q] = _other(read[q], rng)
        if xmin(ref, read) <= MAXX:
            already += 1
            continue
        open_ += 1
        adm += band_gate(ref, read)[0]
        adm1 += band_gate(ref, read, False, 1)[0]
    print("banded by x <= 6: %.3f of %d; of the other %d the bound admits %.3f (three mismatches known per side), %.3f (two)"
          % (already / n, n, open_, adm / open_, adm1 / open_))
    assert open_ > n // 2
    assert adm >= open_ / 2, (adm, open_)
