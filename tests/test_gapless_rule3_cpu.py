"""Case (3) of the gapless rule of pm_gapless_kernel (pecaller_amd/csrc/pemap_sw.hip.h, K3a in DESIGN.md) -- the best diagonal has
three mismatches -- restated in Python with the facts the kernel keeps per diagonal (the first two and the last two mismatches, the
two edge diagonals -1 and D + 1) and its three tests, and checked against the oracle's full DP exactly as test_gapless_rule_cpu.py
checks cases (1) and (2): whenever the rule decides, the DP gives the same double, the same start cell and planes in which the
traceback never leaves plane 0.  Each of the three exclusions must also be SEEN to matter: among the windows it alone refuses there
is one whose DP result is not the diagonal's.  CPU only: this pins the rule, the GPU tests pin the kernel."""
import numpy as np
import oracle_py
from test_gapless_rule_cpu import MISS, match, edge_windows, _add_ones


def _mism(ref, read, d, bis):
    """positions of the read's bases that lie inside the window on diagonal d (-1 .. D + 1) and mismatch it"""
    mm = len(read)
    j = np.arange(mm)
    j = j[(j + d >= 0) & (j + d < len(ref))]
    return j[~match(ref[j + d], read[j], bis)]


def rule3(ref, read, bis=False):
    """-> None (case (3) does not apply: the best diagonal has not three mismatches), or (refusals, score, row of the start cell):
    refusals is the set of the classes 'a', 'b', 'c' that send the window to the DP (empty: decided), score and row the answer of
    the diagonals alone"""
    nn, mm = len(ref), len(read)
    D = nn - mm
    if D < 0:
        return None
    pos = [_mism(ref, read, d, bis) for d in range(D + 1)]
    x = np.array([len(p) for p in pos])
    if x.min() != 3:
        return None
    m1 = np.array([p[0] for p in pos])
    m2 = np.array([p[1] for p in pos])
    l1 = np.array([p[-1] for p in pos])
    l2 = np.array([p[-2] for p in pos])
    p0, p1, s0, s1 = m1, m2, mm - 1 - l1, mm - 1 - l2
    # the edge diagonals: D + 1 holds read bases 0 .. mm - 2, -1 holds 1 .. mm - 1
    e_hi, e_lo = _mism(ref, read, D + 1, bis), _mism(ref, read, -1, bis)
    p0_hi = min(int(e_hi[0]), mm - 1) if len(e_hi) else mm - 1
    s0_lo = mm - 1 - int(e_lo[-1]) if len(e_lo) else mm - 1
    why = set()
    # (a) one deletion, at most one mismatch
    for d2 in range(1, D + 1):
        if p0[:d2].max() + s1[d2] >= mm or p1[:d2].max() + s0[d2] >= mm:
            why.add("a")
    # (b) one inserted read base, no mismatch
    pre = list(p0) + [p0_hi]
    suf = [s0_lo] + list(s0)
    for d1 in range(D + 2):
        if pre[d1] + suf[d1] >= mm - 1:
            why.add("b")
    # (c) two one-base deletions, no mismatch: diagonal l between the prefix of l - 1 and the suffix of l + 1
    for l in range(1, D):
        lo, hi = int(p0[l - 1]), int(l1[l + 1]) + 1
        dirty = False
        if lo < hi:
            dirty = any(lo <= int(q) < hi for q in (m1[l], m2[l], l2[l], l1[l]))
            if not dirty and lo > m2[l] and hi <= l2[l]:
                dirty = bool(((pos[l] >= lo) & (pos[l] < hi)).any())          # (the kernel looks at the pieces of [lo, hi))
        if not dirty:
            why.add("c")
    best, bd = None, -1
    for d in np.nonzero(x == 3)[0]:             # ascending rows, strict '>'; the fold as the kernel takes it
        a, b, c = (int(q) for q in pos[d])
        s = float(a) + MISS
        s = _add_ones(s, b - a - 1) + MISS
        s = _add_ones(s, c - b - 1) + MISS
        s = _add_ones(s, mm - c - 1)
        if best is None or s > best:
            best, bd = s, int(d)
    return why, np.float64(best), bd + mm


def _dp_is_diagonal(ref, read, score, row, bis):
    """is the full DP's answer (score bits, start cell, plane 0 along the whole diagonal) the diagonals' answer?"""
    sc, st, pl = oracle_py.sw(ref, read, bisulfite=bis, planes=True)
    mm = len(read)
    if np.float64(sc).view(np.uint64) != np.float64(score).view(np.uint64):
        return False
    if (int(st[0]), int(st[1]), int(st[2])) != (0, row, mm):
        return False
    i = row
    for j in range(mm, 1, -1):
        a, b, c = pl[0, i - 1, j - 1], pl[1, i - 1, j - 1], pl[2, i - 1, j - 1]
        if b > a or c > max(a, b):
            return False
        i -= 1
    return True


def stress_windows(seed, n):
    """short reads on alphabets of 1 .. 4 letters, tandem repeats, reads that skip one or two reference stretches, an inserted base
    anywhere (the first and the last included), 0 .. 4 substitutions, N on either side"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        mm = int(rng.integers(16, 60))
        slack = int(rng.integers(0, 22))
        alpha = np.frombuffer((b"AC", b"ACGT", b"ACG", b"ACGT", b"A")[k % 5 if k % 50 else 4], np.uint8)
        ref = alpha[rng.integers(0, len(alpha), mm + slack + 4)].copy()
        if k % 4 == 0:
            per = int(rng.integers(1, 7))
            ref = np.tile(ref[:per], len(ref) // per + 1)[:len(ref)].copy()
            for q in rng.integers(0, len(ref), int(rng.integers(0, 3))):          # a blemished repeat
                ref[q] = alpha[int(rng.integers(0, len(alpha)))]
        d = int(rng.integers(0, slack + 1))
        kind = k % 8
        src = list(range(d, d + mm + 4))
        if kind == 6 and slack - d >= 1:                        # the read skips b reference bases
            b = int(rng.integers(1, slack - d + 1))
            p = int(rng.integers(1, mm))
            src = src[:p] + list(range(d + p + b, d + mm + b + 4))
        if kind in (2, 3) and slack - d >= 2:                   # the read skips one base at each of two places
            for p in sorted(rng.integers(1, mm - 1, 2).tolist(), reverse=True):
                src = src[:p] + [s + 1 for s in src[p:]]
        src = [s for s in src if s < len(ref)]
        read = ref[src[:mm]].copy()
        if kind in (5, 7):                                     # an inserted base, anywhere
            p = int(rng.integers(0, mm))
            read = np.concatenate([read[:p], alpha[rng.integers(0, len(alpha), 1)], read[p:mm - 1]]).copy()
        ref = ref[:mm + slack]
        if len(read) < mm or len(alpha) == 1 and kind == 0:
            read = np.resize(read, mm).copy()
        for q in rng.choice(mm, size=(3, 3, 0, 0, 3, 2, 1, 3)[kind] + int(rng.integers(0, 2)) * (k % 3 == 0), replace=False):
            if len(alpha) > 1:
                read[q] = alpha[(int(np.nonzero(alpha == read[q])[0][0]) + int(rng.integers(1, len(alpha)))) % len(alpha)]
            else:
                read[q] = ord("C")
        if k % 11 == 0:
            read[int(rng.integers(0, mm))] = ord("N")
        if k % 13 == 0:
            ref[int(rng.integers(0, len(ref)))] = ord("N")
        yield ref, read


def two_skips(seed, n):
    """reads that skip one reference base at each of two places, without a substitution, on two letters: the tie of class (c)"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"AC", np.uint8)
    for k in range(n):
        mm = int(rng.integers(16, 40))
        slack = int(rng.integers(2, 8))
        ref = alpha[(rng.random(mm + slack) < 0.25).astype(int)].copy()
        d = int(rng.integers(0, slack - 1))
        p, q = sorted(rng.choice(np.arange(2, mm - 2), 2, replace=False).tolist())
        read = np.concatenate([ref[d:d + p], ref[d + p + 1:d + q + 1], ref[d + q + 2:d + mm + 2]]).copy()
        yield ref, read


_seen = {}


def _run(name, it, bis):
    """-> counts of one generator's run: decided, refused by class, and per class the windows it ALONE refused whose DP result
    is not the diagonals' answer.  Every decision is checked against the DP here."""
    if name in _seen:
        return _seen[name]
    r = dict(n=0, applies=0, decided=0, narrow=0, refused=dict(a=0, b=0, c=0), needed=dict(a=0, b=0, c=0))
    for ref, read in it:
        r["n"] += 1
        got = rule3(ref, read, bis)
        if got is None:
            continue
        r["applies"] += 1
        why, score, row = got
        if not why:
            assert _dp_is_diagonal(ref, read, score, row, bis), (ref.tobytes(), read.tobytes(), score, row)
            r["decided"] += 1
            r["narrow"] += len(ref) - len(read) < 21
            continue
        for w in why:
            r["refused"][w] += 1
        if len(why) == 1 and r["needed"][min(why)] < 40:         # (enough to show the class matters; the DP is the test's cost)
            r["needed"][min(why)] += not _dp_is_diagonal(ref, read, score, row, bis)
    _seen[name] = r
    return r


def test_case3_agrees_with_the_full_dp():
    r = _run("stress", stress_windows(20260301, 30000), False)
    print(r)
    assert r["decided"] > 5000, r
    assert all(v >= 1 for v in r["refused"].values()), r
    assert r["needed"]["a"] >= 1 and r["needed"]["b"] >= 1, r


def test_each_exclusion_is_needed():
    """a window that only (c) refuses and on which the DP does not give the diagonals' answer is scarce: the tie of two one-base
    deletions against three mismatches, decided by rounding"""
    r = _run("stress", stress_windows(20260301, 30000), False)
    t = _run("two_skips", two_skips(7, 6000), False)
    print(t)
    assert t["refused"]["c"] >= 1, t
    for w in "abc":
        assert r["needed"][w] + t["needed"][w] >= 1, (w, r, t)


def test_case3_on_clipped_windows_and_odd_letters():
    r = _run("edge", edge_windows(77, 20000, False), False)
    print(r)
    assert r["decided"] > 1000 and r["narrow"] > 500, r


def test_case3_in_bisulfite_mode():
    r = _run("edge_bis", edge_windows(78, 20000, True), True)
    print(r)
    assert r["decided"] > 1000 and r["narrow"] > 500, r


def test_random_reads_with_three_substitutions_are_decided():
    """150 bases, full-width windows (21 spare bases), four letters: the exact rule refuses about one read in a thousand"""
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    n = decided = 0
    for _ in range(1000):
        ref = acgt[rng.integers(0, 4, 171)].copy()
        read = ref[10:160].copy()
        for q in rng.choice(150, 3, replace=False):
            read[q] = acgt[(int(np.searchsorted(acgt, read[q])) + int(rng.integers(1, 4))) % 4]
        got = rule3(ref, read)
        if got is not None:
            n += 1
            decided += not got[0]
    assert n >= 990 and decided >= 0.98 * n, (n, decided)


def test_fold_by_binades_with_three_mismatches():
    """pemapper.c:2062-2081 adds the bonus one read base at a time; the kernel takes the steps of a binade at once, now with three
    -1/3 steps between them"""
    rng = np.random.default_rng(6)
    miss = float(MISS)
    for _ in range(4000):
        mm = int(rng.integers(16, 512))
        a, b, c = sorted(rng.choice(mm, 3, replace=False).tolist())
        if _ % 4 == 0:
            a, b, c = ((0, 1, 2), (mm - 3, mm - 2, mm - 1), (0, 7, 8), (0, mm // 2, mm - 1))[(_ // 4) % 4]
        y = 0.0
        for j in range(mm):
            y = y + (miss if j in (a, b, c) else 1.0)
        z = float(a) + miss
        z = _add_ones(z, b - a - 1) + miss
        z = _add_ones(z, c - b - 1) + miss
        z = _add_ones(z, mm - c - 1)
        assert z == y, (mm, a, b, c)
