"""The seed kernel's k-mers from bit planes (pemap_seed4.hip.h, stage_p): reads of the ladder genome of index_cases.py at the lengths
where the planes' words, the byte registers (lanes 64 and 128), the last cut (len - 16, and len % 16 == 0) and the segment templates
change, on both strands, with N on either side of the N filter (len / 10 and 1 + len / 10 of them), with lower-case and IUPAC
letters, plain and bisulfite -- through the first tier, and with PEMAP_FIRST_TIER=0 through the second.  Expectation: the oracle,
compared as test_gpu_index_cases.py compares (hit lists, window geometry, scores, coordinates, classes, pileup, summary)."""
import functools

import numpy as np
import pytest

import index_cases as ic
import oracle_py
import refio
from test_gpu_index_cases import _compare_with_oracle

pytestmark = pytest.mark.gpu
LENGTHS = (16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 127, 128, 129, 150, 159, 160, 161, 245)
KINDS = ("plain", "n_kept", "n_dropped", "lower", "iupac")
PER_KIND = 6                    # pairs per kind and length: both strands, three places
IUPAC = np.frombuffer(b"RYKMSWBDHVU", np.uint8)


def _spoil(x, kind, rng):
    L = len(x)
    if kind == "n_kept":
        x[rng.choice(L, size=L // 10, replace=False)] = ord("N")
    elif kind == "n_dropped":
        x[rng.choice(L, size=1 + L // 10, replace=False)] = ord("N")
    elif kind == "lower":
        low = rng.random(L) < 0.25
        low[int(rng.integers(0, L))] = True
        x[low] |= 0x20
    elif kind == "iupac":
        q = rng.choice(L, size=min(2, max(1, L // 40)), replace=False)
        x[q] = IUPAC[rng.integers(0, len(IUPAC), len(q))]


@functools.lru_cache(maxsize=None)
def _reads(L, bis):
    """pairs from ordinary places of the large contigs; the kind's letters go into both ends"""
    g = ic.genome()
    rng = np.random.default_rng(977 + 13 * L + int(bis))
    lens = [len(c) for c in g["contigs"]]
    big = [c for c in range(len(lens)) if lens[c] > 4 * L + 1300]
    r1, r2 = [], []
    for kind in KINDS:
        for j in range(PER_KIND):
            c = g["contigs"][big[int(rng.integers(0, len(big)))]]
            fl = L + int(rng.integers(20, 300))
            s = int(rng.integers(L + 300, len(c) - fl - L - 300))
            d = c[s:s + L].copy()
            m = ic.COMP[c[s + fl - L:s + fl]][::-1].copy()
            if j % 2:
                d, m = m, d         # (file 1 holds the reverse strand's end)
            for x in (d, m):
                if bis:
                    conv = (x == ord("C")) & (rng.random(L) < 0.95)
                    x[conv] = ord("T")
                _spoil(x, kind, rng)
            r1.append(d.tobytes())
            r2.append(m.tobytes())
    return refio.pack_reads(r1) + refio.pack_reads(r2)


@functools.lru_cache(maxsize=None)
def _expected(L, bis):
    b1, l1, b2, l2 = _reads(L, bis)
    o = oracle_py.Oracle(ic.index(bis), paired=True, min_dist=0, max_dist=500, min_align=0.85, bisulfite=bis)
    m1, m2, mt, d1, d2 = o.map_batch(b1, l1, b2, l2, debug=True, threads=8)
    return dict(m1=m1, m2=m2, mt=mt, d=(d1, d2), counts=o.counts().copy(), ins=sorted(o.insertions()), summary=o.summary().copy())


@pytest.fixture(scope="module", params=[(False, 1), (False, 2), (True, 1), (True, 2)], ids=["plain-tier1", "plain-tier2", "bisulfite-tier1", "bisulfite-tier2"])
def dev_of(request):
    """one device object per mode and tier, one at a time (the knob is read when the object is made; the look-up replicas of two
    objects do not fit a device)"""
    from pecaller_amd import PemapDev
    bis, tier = request.param
    mp = pytest.MonkeyPatch()
    try:
        if tier == 2:
            mp.setenv("PEMAP_FIRST_TIER", "0")
        else:
            mp.delenv("PEMAP_FIRST_TIER", raising=False)
        dev = PemapDev(0)
    finally:
        mp.undo()
    try:
        ix = ic.index(bis)
        dev.build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
        assert dev.lookup_replicas()[0] == 8
        dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85, bisulfite=bis)
        yield dev, bis, tier
    finally:
        dev.close()


def test_the_oracle_keeps_and_drops_by_the_n_filter():
    """(what the cases rest on, no device: no end with 1 + len / 10 N has a hit, ends of every other kind have)"""
    for bis in (False, True):
        for L in LENGTHS:
            e = _expected(L, bis)
            for which in (0, 1):
                nh = e["d"][which]["n_hits"].reshape(len(KINDS), PER_KIND)
                assert not nh[KINDS.index("n_dropped")].any()
                for kind in ("plain", "n_kept", "lower", "iupac"):
                    assert nh[KINDS.index(kind)].any(), (L, bis, which, kind)


@pytest.mark.parametrize("L", LENGTHS)
def test_kmers_of_every_length_and_letter(L, dev_of):
    dev, bis, tier = dev_of
    b1, l1, b2, l2 = _reads(L, bis)
    e = _expected(L, bis)
    n = len(l1)
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(b1, l1, b2, l2)
    stats, _ = dev.run_stats()
    assert np.array_equal(m1, e["m1"]), np.nonzero(m1 != e["m1"])[0][:10]
    assert np.array_equal(m2, e["m2"]), np.nonzero(m2 != e["m2"])[0][:10]
    assert np.array_equal(mt, e["mt"])
    _compare_with_oracle(dev, e, n)
    assert stats["ends"] == 2 * n
    # which tier took them: every end with PEMAP_FIRST_TIER=0
    assert (stats["big_ends"] == 2 * n) == (tier == 2), stats
