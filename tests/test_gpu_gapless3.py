"""Case (3) of the gapless rule in pm_gapless_kernel (a best diagonal with three mismatches is decided without the banded DP unless
one of three kinds of gapped alignment could beat or tie it; K3a in DESIGN.md) against the oracle, exactly: coordinates, classes,
per-hit fp64 score bits and start cells, pileup, insertions -- and run_stats' "banded" and "walked", which say who decided.

Two batches per read length on a dozen contigs of 5 kb (random letters with homopolymers and short tandem repeats planted in them):
  three   exactly three substitutions, placed where the kernel's 8-base pieces meet (bases 0, 7, 8, 15, 16, L - 9, L - 8, L - 1),
          on neighbouring bases and all in the read's last piece; the reads lie at least 30 bases inside their contig (full-width
          windows) and are those that the rule as restated in tests/test_gapless_rule3_cpu.py decides: none may reach the banded DP
  gaps    gapped reads whose best diagonal has about three mismatches: an indel a few bases from a read end, a one-base insertion
          at the first, the last and a middle base beside substitutions, two one-base deletions, the same inside the planted
          repeats: the rule must leave some of them to the banded DP, and all outputs are the oracle's
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py
import refio
from test_gapless_rule3_cpu import rule3
from test_gpu_traceback import ACGT, COMP, PARAMS, _check_outputs, _check_hits, _mapped_ends

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("three", "gaps")
PAIRS = 300
SLOP = 10               # window bases on either side of the read (MISALIGN_SLOP)


@functools.lru_cache(maxsize=None)
def _contigs():
    rng = np.random.default_rng(3003)
    out = []
    for _ in range(12):
        c = ACGT[rng.integers(0, 4, 5000)].copy()
        for p in range(150, 4800, 300):         # a homopolymer or a short tandem repeat every 300 bases
            unit = ACGT[rng.integers(0, 4, int(rng.integers(1, 4)))]
            n = int(rng.integers(8, 15))
            c[p:p + n] = np.tile(unit, n)[:n]
        out.append(c)
    return out


def _other(b, rng):
    o = ACGT[ACGT != b]
    return o[int(rng.integers(0, 3))]


def _patterns(L, rng):
    last = 8 * ((L - 1) // 8)
    q = int(rng.integers(20, L - 30))
    return [(0, 7, 8), (15, 16, L - 1), (L - 9, L - 8, L - 1), (0, 8, 16), (7, 15, L - 8), (0, L - 9, L - 1), (q, q + 1, q + 2),
            (q, q + 1, q + 6), tuple(sorted(rng.choice(np.arange(last, L), 3, replace=False).tolist())),
            tuple(sorted(rng.choice(L, 3, replace=False).tolist()))]


def _convert(x, rng):
    x = x.copy()
    x[(x == ord("C")) & (rng.random(len(x)) < 0.95)] = ord("T")
    return x


def _three(c, lo, L, k, bis, check, rng):
    """the fragment's strand of one end: c[lo:lo + L] with three substitutions that the rule decides on the full-width window"""
    for attempt in range(40):
        pats = _patterns(L, rng)
        pos = pats[k % len(pats)] if attempt < 4 else pats[-1]
        x = c[lo:lo + L].copy()
        for q in pos:
            x[q] = _other(x[q], rng)
        if not check:
            return x
        y = _convert(x, rng) if bis else x
        got = rule3(c[lo - SLOP:lo + L + SLOP + 1], y, bis)
        if got is not None and not got[0]:
            return y
    raise AssertionError("no decidable read at %d" % lo)


def _gapped(c, lo, L, k, rng):
    """one end with a gap that competes with a diagonal of about three mismatches"""
    kind = k % 8
    t = int(rng.integers(3, 6))
    if kind == 0:         # the read skips 1..3 reference bases t bases from its end
        g = int(rng.integers(1, 4))
        x = np.concatenate([c[lo:lo + L - t], c[lo + L - t + g:lo + L + g]])
    elif kind == 1:       # ... from its start (the window starts where the long part says)
        g = int(rng.integers(1, 4))
        x = np.concatenate([c[lo - g:lo - g + t], c[lo + t:lo + L]])
    elif kind == 2:       # 1..3 inserted bases t bases from an end
        g = int(rng.integers(1, 4))
        p = t if rng.random() < 0.5 else L - t - g
        x = np.concatenate([c[lo:lo + p], ACGT[rng.integers(0, 4, g)], c[lo + p:lo + L - g]])
    elif kind == 3:       # one inserted base at the first, the last or a middle base, and two or three substitutions elsewhere
        p = (0, L - 1, L // 2)[int(rng.integers(0, 3))]
        x = np.concatenate([c[lo:lo + p], ACGT[rng.integers(0, 4, 1)], c[lo + p:lo + L - 1]])
        for q in rng.choice(np.arange(20, L - 20), int(rng.integers(2, 4)), replace=False):
            if abs(int(q) - p) > 2:
                x[q] = _other(x[q], rng)
    elif kind == 4:       # two one-base deletions near an end
        a = L - int(rng.integers(4, 8))
        b = a + int(rng.integers(1, 3))
        x = np.concatenate([c[lo:lo + a], c[lo + a + 1:lo + b + 1], c[lo + b + 2:lo + L + 2]])
    else:                 # the same with the gap inside a planted repeat that lies a few bases from the read's end
        want = lo + t if kind == 6 else lo + L - t          # the planted repeat nearest to where the fragment puts this end
        rep = 150 + 300 * min(max(int(round((want - 150) / 300.0)), 1), 14)
        into = int(rng.integers(2, 8))
        if kind == 5:     # a skipped base, the repeat near the read's end
            lo = rep + into + t - L
            x = np.concatenate([c[lo:rep + into], c[rep + into + 1:rep + into + 1 + t]])
        elif kind == 6:   # an inserted copy of the repeat's base, the repeat near the read's start
            lo = rep + into - t
            x = np.concatenate([c[lo:rep + into], c[rep + into - 1:rep + into], c[rep + into:lo + L - 1]])
        else:             # two skipped bases, one in the repeat and one two bases on
            lo = rep + into + t - L
            x = np.concatenate([c[lo:rep + into], c[rep + into + 1:rep + into + 3], c[rep + into + 4:rep + into + 2 + t]])
    assert len(x) == L, (kind, len(x))
    return x.copy(), lo


def _reads(kind, L, bis, seed):
    rng = np.random.default_rng(seed)
    contigs = _contigs()
    r1, r2 = [], []
    for k in range(PAIRS):
        c = contigs[int(rng.integers(0, len(contigs)))]
        fl = int(rng.integers(L + 20, L + 200))
        s = int(rng.integers(30, len(c) - fl - 30))
        ends = []
        for which in (0, 1):
            lo = s if which == 0 else s + fl - L
            if kind == "three":
                # (bisulfite: the end that reads the converted strand in reverse does not map: nothing to demand of it)
                x = _three(c, lo, L, 2 * k + which, bis, not (bis and which == 1), rng)
                done = bis and which == 0
            else:
                done = False
                if which == k % 2:
                    x, _ = _gapped(c, lo, L, k // 2, rng)
                else:
                    x = c[lo:lo + L].copy()
            if which == 1:
                x = COMP[x][::-1].copy()
            if bis and not done:
                x = _convert(x, rng)
            ends.append(x)
        a, b = ends
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a.tobytes())
        r2.append(b.tobytes())
    return refio.pack_reads(r1) + refio.pack_reads(r2)


@functools.lru_cache(maxsize=None)
def _index(bis):
    contigs = _contigs()
    mers, ukmer, ustart, cs = refio.kmer_index(contigs, bisulfite=bis)
    return dict(mers=mers, ukmer=ukmer, ustart=ustart, genome=np.concatenate(contigs), contig_starts=cs,
                contig_len=np.array([len(c) for c in contigs], dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def _batch(kind, L, bis):
    return _reads(kind, L, bis, 1000 * L + 10 * KINDS.index(kind) + int(bis))


@functools.lru_cache(maxsize=None)
def _expected(kind, L, bis):
    """the oracle's results for one batch on an empty pileup (computed once, shared by the tests, never modified)"""
    b1, l1, b2, l2 = _batch(kind, L, bis)
    o = oracle_py.Oracle(_index(bis), paired=True, bisulfite=bis, **PARAMS)
    m1, m2, mt, d1, d2 = o.map_batch(b1, l1, b2, l2, debug=True, threads=8)
    return dict(m1=m1, m2=m2, mt=mt, d=(d1, d2), counts=o.counts().copy(), ins=sorted(o.insertions()))


def _map_kind(dev, kind, L, bis):
    b1, l1, b2, l2 = _batch(kind, L, bis)
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(b1, l1, b2, l2)
    stats, _ = dev.run_stats()
    dbg = dev.debug_hits(2 * len(l1))
    counts, ins = dev.fetch_pileup()
    return dict(m1=m1, m2=m2, mt=mt, stats=stats, dbg=dbg, counts=counts, ins=sorted(ins))


def _device(bis):
    from pecaller_amd import PemapDev
    dev = PemapDev(0)
    ix = _index(bis)
    dev.build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
    dev.set_params(paired=True, bisulfite=bis, **PARAMS)
    return dev


# (64: 8 pieces, 100: a last piece of four bases, 150: the headline, 245: two pieces per lane in the kernel's loads)
@pytest.mark.parametrize("L,bis", [(150, False), (64, False), (100, True), (245, False)])
def test_three_mismatches_without_the_dp(L, bis):
    dev = _device(bis)
    got = {kind: _map_kind(dev, kind, L, bis) for kind in KINDS}
    dev.close()
    for kind in KINDS:
        exp = _expected(kind, L, bis)
        st = got[kind]["stats"]
        print(kind, "mapped ends", _mapped_ends(got[kind]), "oracle", _mapped_ends(exp),
              {k: st[k] for k in ("walks", "walked", "banded", "gapless", "sw_dirs", "redo")})
        _check_outputs(got[kind], exp, kind)
        _check_hits(got[kind]["dbg"], exp, kind)
        assert st["walks"] == _mapped_ends(got[kind]), (kind, st)
    # nearly every end with three substitutions maps (of 64 bases with three of them gone the seeds can miss one; bisulfite: only
    # the end that reads the converted strand forward maps)
    floor = PAIRS // 2 if bis else 19 * PAIRS // 10
    exp = _expected("three", L, bis)
    assert _mapped_ends(exp) >= floor and int(exp["counts"][:, 4:6].sum()) == 0 and exp["ins"] == []
    st = got["three"]["stats"]
    assert _mapped_ends(got["three"]) >= floor, st
    assert st["banded"] == 0 and st["walked"] == 0, st
    # gaps beside a diagonal with three mismatches: some are left to the banded DP, and gaps were found
    exp = _expected("gaps", L, bis)
    assert int(exp["counts"][:, 4:6].sum()) + len(exp["ins"]) > PAIRS // 8
    st = got["gaps"]["stats"]
    assert st["banded"] > 0 and st["walked"] > 0, st


def _worker(out_path, L, bis):
    """maps the two batches with whatever knobs the environment sets and saves the outputs"""
    sys.path.insert(0, ROOT)
    dev = _device(bis)
    out = {}
    for kind in KINDS:
        r = _map_kind(dev, kind, L, bis)
        for k in ("m1", "m2", "mt", "counts"):
            out[kind + "_" + k] = r[k]
        out[kind + "_ins"] = np.frombuffer(json.dumps([[p, s.decode("latin1")] for p, s in r["ins"]]).encode(), np.uint8)
        out[kind + "_stats"] = np.frombuffer(json.dumps(r["stats"]).encode(), np.uint8)
    dev.close()
    np.savez(out_path, **out)


def test_the_previous_rule_gives_the_same_outputs_through_the_band(tmp_path):
    """PEMAP_GAPLESS=2 (cases (1) and (2) only; a process of its own, the setting is read once): the same outputs, and the ends
    with three mismatches back in the banded DP"""
    L, bis = 150, False
    dev = _device(bis)
    default = {kind: _map_kind(dev, kind, L, bis) for kind in KINDS}
    dev.close()
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out, str(L), str(int(bis))], env=dict(os.environ, PEMAP_GAPLESS="2"),
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    z = np.load(out)
    for kind in KINDS:
        exp = _expected(kind, L, bis)
        got = {k: z[kind + "_" + k] for k in ("m1", "m2", "mt", "counts")}
        got["ins"] = sorted((p, s.encode("latin1")) for p, s in json.loads(z[kind + "_ins"].tobytes().decode()))
        _check_outputs(got, exp, (kind, "PEMAP_GAPLESS=2"))
        _check_outputs(default[kind], exp, (kind, "default"))
        st = json.loads(z[kind + "_stats"].tobytes().decode())
        print(kind, "banded", default[kind]["stats"]["banded"], "with PEMAP_GAPLESS=2", st["banded"])
        assert st["banded"] > default[kind]["stats"]["banded"], (kind, st, default[kind]["stats"])
    st = json.loads(z["three_stats"].tobytes().decode())
    assert st["banded"] >= 19 * PAIRS // 10 and st["walked"] == 0, st


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    _worker(sys.argv[1], int(sys.argv[2]), bool(int(sys.argv[3])))
