"""The band's second way in on the device (PEMAP_BAND_GATE; the bound at PM_BAND_MAXX_ in pecaller_amd/csrc/pemap_sw.hip.h, restated in
tests/test_band_gate_cpu.py): a problem without a diagonal of at most six mismatches goes to the banded DP when a prefix on one
diagonal, one gap and a suffix on another prove that the optimum is at least mm - 8.  Against the oracle, exactly: coordinates,
classes, per-hit fp64 score bits and start cells, pileup, insertions; with the gate and without it (PEMAP_BAND_GATE=0, the routing
before it), each on a device object of its own (the knobs are read when the object is made); and run_stats' account: "gated" is the
number of problems the Python restatement admits on the oracle's windows, and "banded" rises by exactly that.

Two batches per read length on a dozen contigs of 5 kb with planted homopolymers and tandem repeats:
  mix   every end carries one gap -- a deletion of 1, 2, 5, 10 or 21 reference bases or an insertion of 1, 2, 3, 5 or 6 read bases,
        20 bases from the read's start, in its middle or 20 bases from its end -- and 0 .. 3 substitutions on each side of it (all
        sixteen pairs of counts for every gap: both sides of the bound's limits i + j <= 4 | 3 | 2 | 0); a tenth of the fragments
        lies at a contig end (clipped windows), a few reads hold an N
  ins6  6-base insertions alone: none is admitted
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import oracle_py
import refio
from test_band_gate_cpu import MAXX, band_gate, xmin
from test_gpu_gapless3 import _contigs, _index, _other
from test_gpu_traceback import ACGT, COMP, PARAMS, _check_outputs, _check_hits, _mapped_ends

pytestmark = pytest.mark.gpu
KINDS = ("mix", "ins6")
PAIRS = 2000
GAPS = [("del", b) for b in (1, 2, 5, 10, 21)] + [("ins", b) for b in (1, 2, 3, 5, 6)]


def _planted(c, lo, L, combo, rng):
    """L read bases from reference position lo with the gap and the substitutions that `combo` numbers"""
    kind, b = GAPS[combo % 10]
    p = (20, L // 2, L - 20)[(combo // 10) % 3]
    nl, nr = (combo // 30) % 4, (combo // 120) % 4
    if kind == "del":
        x = np.concatenate([c[lo:lo + p], c[lo + p + b:lo + L + b]]).copy()
        right = p
    else:
        if p + b > L - 8:
            p = L - 8 - b
        x = np.concatenate([c[lo:lo + p], ACGT[rng.integers(0, 4, b)], c[lo + p:lo + L - b]]).copy()
        right = p + b
    assert len(x) == L
    for n, a, e in ((nl, 0, p - 3), (nr, right + 3, L)):
        for q in rng.choice(np.arange(a, e), min(n, e - a), replace=False):
            x[q] = _other(x[q], rng)
    return x


def _reads(kind, L, bis, seed):
    rng = np.random.default_rng(seed)
    contigs = _contigs()
    r1, r2 = [], []
    for k in range(PAIRS):
        c = contigs[int(rng.integers(0, len(contigs)))]
        fl = int(rng.integers(L + 40, L + 200))
        s = int(rng.integers(30, len(c) - fl - 60))
        if k % 10 == 0:         # at a contig end: the window of the end that lies there is clipped
            s = int(rng.integers(0, 9)) if k % 20 == 0 else len(c) - fl - 22 - int(rng.integers(0, 9))
        ends = []
        for which in (0, 1):
            lo = s if which == 0 else s + fl - L
            combo = 2 * k + which
            if kind == "ins6":
                combo = 10 * (combo // 10) + 9
            x = _planted(c, lo, L, combo, rng)
            if k % 97 == 0:
                x[int(rng.integers(0, L))] = ord("N")
            if which == 1:
                x = COMP[x][::-1].copy()
            if bis:
                x = x.copy()
                x[(x == ord("C")) & (rng.random(L) < 0.95)] = ord("T")
            ends.append(x)
        a, b = ends
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a.tobytes())
        r2.append(b.tobytes())
    return refio.pack_reads(r1) + refio.pack_reads(r2)


@functools.lru_cache(maxsize=None)
def _batch(kind, L, bis):
    return _reads(kind, L, bis, 2000 * L + 10 * KINDS.index(kind) + int(bis))


def _admitted_by_the_restatement(batch, dbg2, genome, bis):
    """problems (hits of either mate) without a diagonal of at most MAXX mismatches that band_gate admits on the oracle's windows"""
    b1, l1, b2, l2 = batch
    n = 0
    for which, (rows, lens, od) in enumerate(((b1, l1, dbg2[0]), (b2, l2, dbg2[1]))):
        for i in np.nonzero(od["n_hits"])[0]:
            read = np.asarray(rows[i][:lens[i]], np.uint8)
            rc = COMP[read][::-1]
            for h in range(int(od["n_hits"][i])):
                ws, wl = int(od["win_start"][i, h]) & 0xFFFFFFFF, int(od["win_len"][i, h])
                ref = genome[ws:ws + wl]
                y = rc if od["orient"][i, h] else read
                if xmin(ref, y, bis) > MAXX and band_gate(ref, y, bis)[0]:
                    n += 1
    return n


@functools.lru_cache(maxsize=None)
def _expected(kind, L, bis):
    """the oracle's results for one batch on an empty pileup, and the restatement's count (computed once, never modified)"""
    b1, l1, b2, l2 = _batch(kind, L, bis)
    ix = _index(bis)
    o = oracle_py.Oracle(ix, paired=True, bisulfite=bis, **PARAMS)
    m1, m2, mt, d1, d2 = o.map_batch(b1, l1, b2, l2, debug=True, threads=8)
    return dict(m1=m1, m2=m2, mt=mt, d=(d1, d2), counts=o.counts().copy(), ins=sorted(o.insertions()),
                admitted=_admitted_by_the_restatement((b1, l1, b2, l2), (d1, d2), ix["genome"], bis))


@contextlib.contextmanager
def _knob(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _map_all(gate, L, bis):
    from pecaller_amd import PemapDev
    with _knob("PEMAP_BAND_GATE", str(gate)):
        dev = PemapDev(0)
    ix = _index(bis)
    dev.build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
    dev.set_params(paired=True, bisulfite=bis, **PARAMS)
    out = {}
    for kind in KINDS:
        b1, l1, b2, l2 = _batch(kind, L, bis)
        dev.reset_pileup()
        m1, m2, mt = dev.map_batch(b1, l1, b2, l2)
        stats, _ = dev.run_stats()
        dbg = dev.debug_hits(2 * len(l1))
        counts, ins = dev.fetch_pileup()
        out[kind] = dict(m1=m1, m2=m2, mt=mt, stats=stats, dbg=dbg, counts=counts, ins=sorted(ins))
    dev.close()
    return out


# (64: 8 pieces and the 8-lane DP; 100: a last piece of four bases, bisulfite; 150: the headline; 245: long rows, two pieces per lane)
@pytest.mark.parametrize("L,bis", [(64, False), (100, True), (150, False), (245, False)])
def test_one_gap_reads_through_the_band(L, bis):
    on, off = _map_all(1, L, bis), _map_all(0, L, bis)
    same = ("walks", "gapless", "sw_dirs", "redo", "pile_incs", "big_ends", "positions", "sw_score", "walked")
    for kind in KINDS:
        exp = _expected(kind, L, bis)
        a, b = on[kind], off[kind]
        sa, sb = a["stats"], b["stats"]
        print(kind, "mapped ends", _mapped_ends(a), "oracle", _mapped_ends(exp), "restatement admits", exp["admitted"],
              {k: (sa[k], sb[k]) for k in ("gated", "banded", "sw_dirs", "gapless", "walks", "walked", "redo", "sw_score")})
        for got, tag in ((a, (kind, "gate")), (b, (kind, "no gate"))):
            _check_outputs(got, exp, tag)
            _check_hits(got["dbg"], exp, tag)
        for k in ("m1", "m2", "mt", "counts"):
            assert np.array_equal(a[k], b[k]), (kind, k)
        assert a["ins"] == b["ins"], kind
        # (the per-hit records of both equal the oracle's in every slot that holds a hit: _check_hits above)
        assert np.array_equal(a["dbg"]["n_hits"], b["dbg"]["n_hits"]), kind
        assert sb["gated"] == 0, sb
        assert sa["gated"] == exp["admitted"], (kind, sa, exp["admitted"])
        assert sa["banded"] - sb["banded"] == sa["gated"], (kind, sa, sb)
        for k in same:
            assert sa[k] == sb[k], (kind, k, sa, sb)
    assert on["mix"]["stats"]["gated"] > 0
    assert on["ins6"]["stats"]["gated"] == 0
    # gaps were found, and the reads mapped
    exp = _expected("mix", L, bis)
    assert int(exp["counts"][:, 4:6].sum()) + len(exp["ins"]) > PAIRS // 8


def test_unset_the_gate_follows_the_chunk_size():
    """Without PEMAP_BAND_GATE the bound is tested in the chunks that hold more read-ends than one pass of the full DP's grid takes
    problems (CUs x PEMAP_SW_WAVES_PER_CU waves, four 150-base problems each): with one wave per CU that is 4 x CUs ends.  The
    first 2 x CUs pairs of the mix are routed as before, one pair more and the bound is tested; same outputs on the shared pairs."""
    from pecaller_amd import PemapDev
    if "PEMAP_BAND_GATE" in os.environ:
        pytest.skip("PEMAP_BAND_GATE is set: this test is about the default")
    L, bis = 150, False
    with _knob("PEMAP_SW_WAVES_PER_CU", "1"):
        dev = PemapDev(0)
    n = 2 * dev.sw_grid()           # pairs: 2 n ends = four problems for each of the grid's waves
    assert 16 <= n < PAIRS, n
    ix = _index(bis)
    dev.build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
    dev.set_params(paired=True, bisulfite=bis, **PARAMS)
    b1, l1, b2, l2 = _batch("mix", L, bis)
    exp = _expected("mix", L, bis)
    got = {}
    for k in (n, n + 1):
        dev.reset_pileup()
        m1, m2, mt = dev.map_batch(b1[:k], l1[:k], b2[:k], l2[:k])
        got[k] = (m1, m2, mt, dev.run_stats()[0])
        for a, e in zip((m1, m2, mt), (exp["m1"], exp["m2"], exp["mt"])):
            assert np.array_equal(a, e[:k]), k
    dev.close()
    lo, hi = got[n][3], got[n + 1][3]
    print(n, {k: (lo[k], hi[k]) for k in ("gated", "banded", "sw_dirs", "gapless")})
    assert lo["gated"] == 0 and hi["gated"] > n // 8, (lo, hi)
    assert hi["banded"] - hi["gated"] <= lo["banded"] + 1, (lo, hi)
