"""The two row forms of pm_gapless_kernel (short rows for reads of up to 160 bases: 160 + 208 bytes of LDS per problem and queues
of 24 entries; the long form for everything longer) against the oracle, exactly: coordinates, classes, per-hit fp64 score bits and
start cells, pileup, insertions -- and run_stats' account of who decided each problem.

The contigs and the read makers are those of test_gpu_gapless3.py, the comparisons those of test_gpu_traceback.py.  Batches of 300
pairs:
  ends    one end of every pair starts 0..12 bases from its contig's first base or ends 0..12 bases from its last one (clipped
          windows: every window length from the read's length up to the full one, length + 21), the other lies inside; 0..2
          substitutions anywhere in the read, the last base included; both strands, as in every paired batch
  last3   exactly three substitutions, all in the read's last 8-base piece (a partial one unless the length is a multiple of 8):
          these go through the rule's second launch (case (3)), which decides them
  mixed   rows 160 wide holding reads of 40..160 bases
  band / dp / perfect   batches all of whose problems go to the banded DP / to the full DP / are decided at once: together with
          last3 (all to the second launch) every per-wave queue fills and is flushed many times, or never
The lengths: 150, 153 and 159 have a partial last piece, 160 is the largest short row (window 181), 161 and 168 take the long form.

run_stats: "sw_score" counts every problem, "sw_dirs" those the DP scored with directions -- the banded DP's ("banded") among them --
and "gapless" those the rule decided.  Every problem is counted once: gapless + sw_dirs - redo = the oracle's number of problems
where no end has several hits (such an end's problems are scored without directions and its winner is scored again: "redo").
"""
import functools

import numpy as np
import pytest

import oracle_py
import refio
from test_gapless_rule3_cpu import rule3
from test_gpu_gapless3 import PAIRS, SLOP, _contigs, _device, _index, _other
from test_gpu_gapless3 import _reads as _reads3
from test_gpu_traceback import COMP, PARAMS, _check_hits, _check_outputs, _indel, _mapped_ends, _substitute

pytestmark = pytest.mark.gpu
LENGTHS = (150, 153, 159, 160, 161, 168)


def _pair_up(ends, rng, r1, r2):
    a, b = ends
    if rng.random() < 0.5:
        a, b = b, a
    r1.append(a.tobytes())
    r2.append(b.tobytes())


def _last3(c, lo, L, rng):
    """c[lo:lo + L] with three substitutions in the last piece (where that has fewer than three bases: on the last three bases, which
    end in it) that the rule, as restated in tests/test_gapless_rule3_cpu.py, decides on the full-width window"""
    last = 8 * ((L - 1) // 8)
    first = last if L - last >= 3 else L - 3
    for attempt in range(60):
        if attempt == 30:
            first = L - 8         # (the last three bases alone leave no choice of positions)
        x = c[lo:lo + L].copy()
        for q in rng.choice(np.arange(first, L), 3, replace=False):
            x[q] = _other(x[q], rng)
        got = rule3(c[lo - SLOP:lo + L + SLOP + 1], x, False)
        if got is not None and not got[0]:
            return x
    raise AssertionError("no decidable read at %d" % lo)


def _make(kind, L, seed):
    """(r1, r2): lists of reads; L is the length of all reads but "mixed"'s"""
    rng = np.random.default_rng(seed)
    contigs = _contigs()
    r1, r2 = [], []
    for k in range(PAIRS):
        c = contigs[int(rng.integers(0, len(contigs)))]
        if kind == "mixed":
            L = 160 if k == 0 else 40 if k == 1 else int(rng.integers(40, 161))
        fl = int(rng.integers(L + 20, L + 200))
        s = int(rng.integers(30, len(c) - fl - 30))
        if kind == "ends":
            e = (k // 2) % 13
            s = e if k % 2 == 0 else len(c) - fl - e
        ends = []
        for which in (0, 1):
            lo = s if which == 0 else s + fl - L
            if kind == "last3":
                x = _last3(c, lo, L, rng)
            elif kind == "band":
                x = c[lo:lo + L].copy()
                _substitute(x, rng, int(rng.integers(4, 7)), L)     # 4..6 substitutions at least 20 bases apart
            elif kind == "dp":
                x = _indel(c, lo, L, int(rng.integers(40 * L // 150, 110 * L // 150 + 1)), rng)
            else:
                x = c[lo:lo + L].copy()
                if kind != "perfect":
                    for q in rng.choice(L, int(rng.integers(0, 3)), replace=False):
                        x[q] = _other(x[q], rng)
                    if k % 5 == 0:
                        x[L - 1] = _other(x[L - 1], rng)
            assert len(x) == L
            if which == 1:
                x = COMP[x][::-1].copy()
            ends.append(x)
        _pair_up(ends, rng, r1, r2)
    return r1, r2


@functools.lru_cache(maxsize=None)
def _batch(kind, L, bis):
    if bis:
        return _reads3("three", L, True, 77000 + L)
    r1, r2 = _make(kind, L, 5000 * L + sum(kind.encode()))
    stride = 160 if kind == "mixed" else 304
    return refio.pack_reads(r1, stride) + refio.pack_reads(r2, stride)


@functools.lru_cache(maxsize=None)
def _expected(kind, L, bis):
    """the oracle's results for one batch on an empty pileup (computed once, shared, never modified)"""
    b1, l1, b2, l2 = _batch(kind, L, bis)
    o = oracle_py.Oracle(_index(bis), paired=True, bisulfite=bis, **PARAMS)
    m1, m2, mt, d1, d2 = o.map_batch(b1, l1, b2, l2, debug=True, threads=8)
    return dict(m1=m1, m2=m2, mt=mt, d=(d1, d2), counts=o.counts().copy(), ins=sorted(o.insertions()))


def _map(dev, kind, L, bis):
    b1, l1, b2, l2 = _batch(kind, L, bis)
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(b1, l1, b2, l2)
    stats, _ = dev.run_stats()
    dbg = dev.debug_hits(2 * len(l1))
    counts, ins = dev.fetch_pileup()
    return dict(m1=m1, m2=m2, mt=mt, stats=stats, dbg=dbg, counts=counts, ins=sorted(ins))


def _problems(exp):
    """(the oracle's alignment problems, those of ends with several hits)"""
    nh = np.concatenate([exp["d"][0]["n_hits"], exp["d"][1]["n_hits"]]).astype(np.int64)
    return int(nh.sum()), int(nh[nh > 1].sum())


def _run(kinds, L, bis):
    dev = _device(bis)
    got = {kind: _map(dev, kind, L, bis) for kind in kinds}
    dev.close()
    out = {}
    for kind in kinds:
        exp = _expected(kind, L, bis)
        st = got[kind]["stats"]
        n, multi = _problems(exp)
        print(kind, L, "bis" if bis else "", "problems", n, "in multi-hit ends", multi, "mapped ends", _mapped_ends(got[kind]),
              {k: st[k] for k in ("sw_score", "walks", "walked", "banded", "gapless", "sw_dirs", "redo")})
        _check_outputs(got[kind], exp, (kind, L))
        _check_hits(got[kind]["dbg"], exp, (kind, L))
        assert st["sw_score"] == n, (kind, L, st)
        assert st["banded"] <= st["sw_dirs"], (kind, L, st)
        if multi == 0:
            assert st["gapless"] + st["sw_dirs"] - st["redo"] == n, (kind, L, st)
        out[kind] = (st, n, multi, exp)
    return out


@pytest.mark.parametrize("L", LENGTHS)
def test_row_forms_at_the_edges(L):
    r = _run(("ends", "last3"), L, False)
    st, n, multi, exp = r["ends"]
    assert n >= 19 * PAIRS // 10, (n, st)
    # the clipped windows are there: at a contig's first bases each length from L + 11 up to the full L + 21; at its last bases (the
    # index's coordinates stop 15 bases short of a contig's end) each length from L up to L + 8, and a few below L
    wl = set(int(v) for w in (0, 1) for v in exp["d"][w]["win_len"][:, 0][exp["d"][w]["n_hits"] > 0])
    assert set(range(L + 11, L + 22)) | set(range(L, L + 9)) <= wl, sorted(wl)
    # at most three substitutions: the rule's, but for the quarter of the ends whose window is cut short at the contig's last bases
    assert st["gapless"] >= n // 2, st
    st, n, multi, exp = r["last3"]
    assert n >= 19 * PAIRS // 10 and int(exp["counts"][:, 4:6].sum()) == 0 and exp["ins"] == [], (n, st)
    assert st["banded"] == 0 and st["walked"] == 0 and st["sw_dirs"] == st["redo"], st


def test_mixed_lengths_in_rows_160_wide():
    b1, l1, b2, l2 = _batch("mixed", 160, False)
    assert b1.shape[1] == 160 and max(l1.max(), l2.max()) == 160 and min(l1.min(), l2.min()) == 40
    st, n, multi, exp = _run(("mixed",), 160, False)["mixed"]
    assert n >= 18 * PAIRS // 10 and st["gapless"] >= 9 * n // 10, (n, st)


def test_bisulfite_at_160():
    st, n, multi, exp = _run(("three",), 160, True)["three"]
    assert n >= PAIRS // 2 and st["banded"] == 0 and st["walked"] == 0, (n, st)


@pytest.mark.parametrize("L", (150, 160))
def test_queues_fill_and_flush_or_never(L):
    """At least 200 consecutive problems (here: all of a batch, so whichever order the task list has) take the same way out of the
    rule's kernel: its queue is flushed a dozen times by the waves that hold them while the other queues stay empty."""
    r = _run(("band", "dp", "last3", "perfect"), L, False)
    # (the few problems of an end with several hits -- a fragment beside a planted repeat -- are other windows: they may go any way)
    for kind in r:
        assert r[kind][1] >= 19 * PAIRS // 10 and r[kind][2] <= PAIRS // 20, (kind, r[kind][:3])
    st, n, multi = r["band"][:3]
    assert st["banded"] >= n - multi and st["gapless"] <= multi and st["sw_dirs"] - st["banded"] <= multi, st
    st, n, multi = r["dp"][:3]
    assert st["banded"] <= multi and st["gapless"] <= multi and st["sw_dirs"] >= n - multi, st
    for kind in ("last3", "perfect"):
        st, n, multi = r[kind][:3]
        assert st["banded"] <= multi and st["sw_dirs"] <= multi + st["redo"] and st["gapless"] >= n - multi, (kind, st)
