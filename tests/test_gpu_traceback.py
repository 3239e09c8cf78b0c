"""The traceback stage's short cut for banded alignments: pm_band_kernel flags an alignment whose traceback never leaves the
start cell's diagonal (PM_GAPLESS beside PM_BANDED), pm_select_kernel lists only the other winners for pm_walk_kernel, and
pm_pile_kernel applies a flagged one as mm diagonal steps.  Against the oracle, exactly: coordinates, classes, per-hit fp64
score bits and start cells, pileup, insertions -- and the number of alignments that were walked (run_stats' "walked").

Read-ends of four kinds on a genome of uniform random letters (12 contigs, 60 kb), each kind mapped as a batch of its own so
that the counters can be told apart:
  subs      3..6 substitutions at least 20 bases apart, no indel: banded, and none may be walked
  mid       one insertion or deletion of 1..6 bases in the middle of the read: every mapped end is walked
  near_end  an indel within 5 bases of a read end
  clipped   reads at a contig's first or last bases or hanging over them: clipped windows, start rows below the read length
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[:] = ord("N")
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
KINDS = ("subs", "mid", "near_end", "clipped")
PAIRS_PER_KIND = 600
PARAMS = dict(min_dist=0, max_dist=500, min_align=0.85)


def _contigs():
    rng = np.random.default_rng(2024)
    return [ACGT[rng.integers(0, 4, 5000)].copy() for _ in range(12)]


def _substitute(x, rng, nsub, L):
    """nsub substitutions at least 20 bases apart (as many as fit into L bases)"""
    nsub = min(nsub, (L - 1) // 20 + 1)
    base = np.sort(rng.integers(0, L - 20 * (nsub - 1), nsub))
    for q in base + 20 * np.arange(nsub):
        other = ACGT[ACGT != x[q]]
        x[q] = other[int(rng.integers(0, 3))]


def _span(c, lo, n, rng):
    """c[lo:lo + n], with random letters where the span leaves the contig"""
    out = ACGT[rng.integers(0, 4, n)].copy()
    a, b = max(lo, 0), min(lo + n, len(c))
    out[a - lo:b - lo] = c[a:b]
    return out


def _indel(c, lo, L, p, rng):
    """L read bases from reference position lo with one insertion or deletion of 1..6 bases after read offset p"""
    g = int(rng.integers(1, 7))
    if rng.random() < 0.5:      # the read skips g reference bases
        return np.concatenate([c[lo:lo + p], c[lo + p + g:lo + L + g]]).copy()
    return np.concatenate([c[lo:lo + p], ACGT[rng.integers(0, 4, g)], c[lo + p:lo + max(p, L - g)]])[:L].copy()


def _reads(contigs, kind, L, bis, seed):
    rng = np.random.default_rng(seed)
    r1, r2 = [], []
    for _ in range(PAIRS_PER_KIND):
        c = contigs[int(rng.integers(0, len(contigs)))]
        fl = int(rng.integers(L + 20, L + 200))
        s = int(rng.integers(10, len(c) - fl - 20))
        if kind == "clipped":
            # one end starts 0..4 bases inside the contig's end or hangs 1..8 bases over it; the other lies inside
            h = int(rng.integers(-4, 9))
            if rng.random() < 0.5:
                s = -h
            else:
                s = len(c) - fl + h
        ends = []
        for which in (0, 1):
            lo = s if which == 0 else s + fl - L
            if kind == "subs":
                x = c[lo:lo + L].copy()
                _substitute(x, rng, int(rng.integers(3, 7)), L)
            elif kind == "mid":
                x = _indel(c, lo, L, int(rng.integers(40 * L // 150, 110 * L // 150 + 1)), rng)
            elif kind == "near_end":
                t = int(rng.integers(1, 6))
                x = _indel(c, lo, L, t if rng.random() < 0.5 else L - t, rng)
            else:
                x = _span(c, lo, L, rng)
                _substitute(x, rng, 3, L)
            assert len(x) == L
            if which == 1:
                x = COMP[x][::-1].copy()
            if bis:
                conv = (x == ord("C")) & (rng.random(L) < 0.95)
                x[conv] = ord("T")
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
    return _reads(_contigs(), kind, L, bis, 100 * L + 10 * KINDS.index(kind) + int(bis))


@functools.lru_cache(maxsize=None)
def _expected(kind, L, bis):
    """the oracle's results for one kind's batch on an empty pileup (computed once, shared by the tests, never modified)"""
    b1, l1, b2, l2 = _batch(kind, L, bis)
    o = oracle_py.Oracle(_index(bis), paired=True, bisulfite=bis, **PARAMS)
    m1, m2, mt, d1, d2 = o.map_batch(b1, l1, b2, l2, debug=True, threads=8)
    return dict(m1=m1, m2=m2, mt=mt, d=(d1, d2), counts=o.counts().copy(), ins=sorted(o.insertions()))


def _map_kind(dev, kind, L, bis):
    """one kind's batch on the device, on an empty pileup"""
    b1, l1, b2, l2 = _batch(kind, L, bis)
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(b1, l1, b2, l2)
    stats, _ = dev.run_stats()
    dbg = dev.debug_hits(2 * len(l1))
    counts, ins = dev.fetch_pileup()
    return dict(m1=m1, m2=m2, mt=mt, stats=stats, dbg=dbg, counts=counts, ins=sorted(ins))


def _check_outputs(got, exp, tag):
    assert np.array_equal(got["m1"], exp["m1"]), (tag, np.nonzero(got["m1"] != exp["m1"])[0][:10])
    assert np.array_equal(got["m2"], exp["m2"]), (tag, np.nonzero(got["m2"] != exp["m2"])[0][:10])
    assert np.array_equal(got["mt"], exp["mt"]), tag
    assert np.array_equal(got["counts"], exp["counts"]), (tag, np.nonzero((got["counts"] != exp["counts"]).any(axis=1))[0][:10])
    assert got["ins"] == exp["ins"], tag


def _check_hits(dbg, exp, tag):
    for which, od in enumerate(exp["d"]):
        nh = dbg["n_hits"][which::2]
        assert np.array_equal(nh, od["n_hits"]), tag
        for i in np.nonzero(nh)[0]:
            k = nh[i]
            e = 2 * i + which
            assert np.array_equal(dbg["score"][e, :k].view(np.uint64), od["score"][i, :k].view(np.uint64)), (tag, e)
            assert np.array_equal(dbg["start_k"][e, :k], od["start"][i, :k, 0]), (tag, e)
            assert np.array_equal(dbg["start_i"][e, :k], od["start"][i, :k, 1]), (tag, e)


def _mapped_ends(r):
    return int((r["m1"] > 0).sum() + (r["m2"] > 0).sum())


# (150: 10 segments, 16 lanes x 10 columns; 100: 7 segments, 8 x 13; 245: 16 segments, 16 x 16)
@pytest.mark.parametrize("L,bis", [(150, False), (100, False), (100, True), (245, False), (245, True)])
def test_diagonal_flag(L, bis):
    from pecaller_amd import PemapDev
    # what makes "no substitution-only end is walked" a fair demand: the oracle's tracebacks of these ends hold no gap at all
    exp = _expected("subs", L, bis)
    assert int(exp["counts"][:, 4:6].sum()) == 0 and exp["ins"] == []
    dev = PemapDev(0)
    ix = _index(bis)
    dev.build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
    dev.set_params(paired=True, bisulfite=bis, **PARAMS)
    got = {}
    for kind in KINDS:
        got[kind] = _map_kind(dev, kind, L, bis)
    dev.close()
    for kind in KINDS:
        exp = _expected(kind, L, bis)
        _check_outputs(got[kind], exp, kind)
        _check_hits(got[kind]["dbg"], exp, kind)
        st = got[kind]["stats"]
        print(kind, "mapped ends", _mapped_ends(got[kind]), {k: st[k] for k in ("walks", "walked", "banded", "gapless", "sw_dirs", "redo")})
        assert st["walks"] == _mapped_ends(got[kind]), (kind, st)
        assert st["walked"] <= st["walks"], (kind, st)
    floor = PAIRS_PER_KIND // 4 if bis else PAIRS_PER_KIND      # (bisulfite: only the end that reads the converted strand forward maps)
    st = got["subs"]["stats"]
    assert _mapped_ends(got["subs"]) >= floor and st["banded"] >= floor, st
    assert st["walked"] == 0, st
    st = got["mid"]["stats"]
    assert _mapped_ends(got["mid"]) >= floor, st
    assert int(_expected("mid", L, bis)["counts"][:, 4:6].sum()) >= floor
    assert st["walked"] == st["walks"], st
    # the other two kinds contribute what they contribute: gaps were found, and flagged alignments occurred beside them
    for kind in ("near_end", "clipped"):
        st = got[kind]["stats"]
        assert _mapped_ends(got[kind]) >= floor // 2 and st["banded"] > 0, (kind, st)
    assert got["near_end"]["stats"]["walked"] > 0
    starts = np.concatenate([_expected("clipped", L, bis)["d"][w]["start"][:, 0, 1] for w in (0, 1)])
    nh = np.concatenate([_expected("clipped", L, bis)["d"][w]["n_hits"] for w in (0, 1)])
    assert int(((starts < L) & (nh > 0)).sum()) > 20         # start rows below the read length: the diagonal meets the top border


def _worker(out_path, L, bis):
    """maps the four batches with whatever knobs the environment sets and saves the outputs"""
    sys.path.insert(0, ROOT)
    from pecaller_amd import PemapDev
    dev = PemapDev(0)
    ix = _index(bis)
    dev.build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
    dev.set_params(paired=True, bisulfite=bis, **PARAMS)
    out = {}
    for kind in KINDS:
        r = _map_kind(dev, kind, L, bis)
        for k in ("m1", "m2", "mt", "counts"):
            out[kind + "_" + k] = r[k]
        out[kind + "_ins"] = np.frombuffer(json.dumps([[p, s.decode("latin1")] for p, s in r["ins"]]).encode(), np.uint8)
        out[kind + "_stats"] = np.frombuffer(json.dumps(r["stats"]).encode(), np.uint8)
    dev.close()
    np.savez(out_path, **out)


@pytest.mark.parametrize("knobs", [dict(PEMAP_BAND="0"), dict(PEMAP_BAND="0", PEMAP_GAPLESS="0")])
def test_knobs_that_walk_everything_give_the_same_outputs(knobs, tmp_path):
    """without the banded DP nothing is flagged, and without the gapless rule every winner is walked: same outputs"""
    L, bis = 150, False
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out, str(L), str(int(bis))], env=dict(os.environ, **knobs),
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    z = np.load(out)
    for kind in KINDS:
        exp = _expected(kind, L, bis)
        got = {k: z[kind + "_" + k] for k in ("m1", "m2", "mt", "counts")}
        got["ins"] = sorted((p, s.encode("latin1")) for p, s in json.loads(z[kind + "_ins"].tobytes().decode()))
        _check_outputs(got, exp, (kind, knobs))
        st = json.loads(z[kind + "_stats"].tobytes().decode())
        assert st["banded"] == 0 and st["walks"] == _mapped_ends(got), (kind, st)
        if "PEMAP_GAPLESS" in knobs:
            assert st["gapless"] == 0 and st["walked"] == st["walks"], (kind, st)
        else:
            assert st["walked"] <= st["walks"] and (kind != "mid" or st["walked"] == st["walks"]), (kind, st)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    _worker(sys.argv[1], int(sys.argv[2]), bool(int(sys.argv[3])))
