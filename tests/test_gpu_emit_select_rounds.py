"""pm_emit_kernel and pm_select_kernel at the boundaries of their waves.  A wave of pm_emit_kernel takes 8 rounds of 64 consecutive
read-ends and reserves its ranges of both task lists with one 64-bit atomic; the slab of a single-hit end is its task number; a wave
of pm_select_kernel counts its winners by ballot and reserves their places in `wins` and `walks` with one 64-bit atomic.  The reads
of pair_cases.py (ends of 0, 1 and tens of hits, every mapping class) are mapped in slices that end one short of, on and one past a
round (64 ends) and a wave (512 ends), paired and single-ended, and once with PEMAP_GAPLESS=0, where the winners of the multi-hit
ends are scored again in slabs numbered behind the single hits'.

Against the oracle on the same slice, exactly: coordinates and classes, the hit lists with their fp64 score bits and start cells,
pileup, insertions, summary, and run_stats' "walks" against the mapped ends.
"""
import functools

import numpy as np
import pytest

import pair_cases as pc

pytestmark = pytest.mark.gpu

L = 100
PARAMS = dict(min_dist=0, max_dist=500, min_align=0.85)
PAIRED_N = (1, 31, 32, 33, 255, 256, 257, 3000)         # in pairs: the rounds' and the waves' boundaries of 64 and 512 ends
SINGLE_N = (63, 64, 65, 511, 512, 513)


def _slice(paired, n):
    b1, l1, b2, l2 = pc.reads(L)
    return (b1[:n], l1[:n], b2[:n], l2[:n]) if paired else (b1[:n], l1[:n], None, None)


@functools.lru_cache(maxsize=None)
def _expected(paired, n):
    """the oracle's results for the first n reads on an empty pileup (computed once, shared, never modified)"""
    b1, l1, b2, l2 = _slice(paired, n)
    o = pc.oracle_py.Oracle(pc.index(), paired=paired, **PARAMS)
    m1, m2, mt, d1, d2 = o.map_batch(b1, l1, b2, l2, debug=True, threads=8)
    return dict(m1=m1, m2=m2, mt=mt, d=(d1, d2) if paired else (d1,), counts=o.counts().copy(), ins=sorted(o.insertions()),
                summary=o.summary().copy())


def _make_dev():
    from pecaller_amd import PemapDev
    d = PemapDev(0)
    ix = pc.index()
    d.build_index(ix["genome"], ix["contig_len"])
    return d


@pytest.fixture(scope="module")
def dev():
    d = _make_dev()
    yield d
    d.close()


def _check(dev, paired, n, tag):
    exp = _expected(paired, n)
    dev.set_params(paired=paired, **PARAMS)
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(*_slice(paired, n))
    stats, _ = dev.run_stats()
    assert np.array_equal(mt, exp["mt"]), (tag, np.nonzero(mt != exp["mt"])[0][:10])
    assert np.array_equal(m1, exp["m1"]), (tag, np.nonzero(m1 != exp["m1"])[0][:10])
    if paired:
        assert np.array_equal(m2, exp["m2"]), (tag, np.nonzero(m2 != exp["m2"])[0][:10])
    ends = len(exp["d"])
    dbg = dev.debug_hits(ends * n)
    for which, od in enumerate(exp["d"]):
        nh = dbg["n_hits"][which::ends]
        assert np.array_equal(nh, od["n_hits"]), (tag, which)
        k = np.arange(pc.oracle_py.MAX_HITS)[None, :] < nh[:, None]         # the listed hits of every end
        for key in ("spot", "orient"):
            assert np.array_equal(dbg[key][which::ends][k], od[key][k]), (tag, which, key)
        assert np.array_equal(dbg["score"][which::ends][k].view(np.uint64), od["score"][k].view(np.uint64)), (tag, which)
        assert np.array_equal(dbg["start_k"][which::ends][k], od["start"][:, :, 0][k]), (tag, which)
        assert np.array_equal(dbg["start_i"][which::ends][k], od["start"][:, :, 1][k]), (tag, which)
    counts, ins = dev.fetch_pileup()
    assert np.array_equal(counts, exp["counts"]), (tag, np.nonzero((counts != exp["counts"]).any(axis=1))[0][:10])
    assert sorted(ins) == exp["ins"], tag
    assert dev.summary().tolist() == exp["summary"].tolist(), tag
    mapped = int((m1 > 0).sum()) + (int((m2 > 0).sum()) if paired else 0)
    assert stats["walks"] == mapped, (tag, stats)
    return stats, dbg


@pytest.mark.parametrize("n", PAIRED_N)
def test_paired_slices_equal_oracle(dev, n):
    _check(dev, True, n, ("paired", n))


@pytest.mark.parametrize("n", SINGLE_N)
def test_single_slices_equal_oracle(dev, n):
    _check(dev, False, n, ("single", n))


def test_the_reads_hold_every_kind_of_end():
    """what the slices are meant to put into one wave: ends without a hit, with one, and with tens"""
    nh = np.concatenate([d["n_hits"] for d in _expected(True, PAIRED_N[-1])["d"]])
    assert (nh == 0).sum() > 0 and (nh == 1).sum() > 100 and (nh >= 10).sum() > 100, np.bincount(nh)[:12]


def test_redo_slabs_behind_the_single_hits(monkeypatch):
    """PEMAP_GAPLESS=0: every winner of a multi-hit end is scored again, in a slab pm_select_kernel numbers from where
    pm_emit_kernel's single hits end (an object of its own: the knobs are read by pemap_dev_create)"""
    monkeypatch.setenv("PEMAP_GAPLESS", "0")
    d = _make_dev()
    try:
        n = PAIRED_N[-1]
        stats, dbg = _check(d, True, n, "gapless=0")
        print("redo", stats["redo"], "sw_dirs", stats["sw_dirs"], "walks", stats["walks"])
        assert stats["gapless"] == 0 and stats["redo"] > 0, stats
    finally:
        d.close()
