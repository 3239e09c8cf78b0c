"""pm_select_kernel ("K4" in DESIGN.md: which hit of each end is traced, the mapping class, m1 / m2) on the inputs of pair_cases.py,
which reach every class the reference assigns, put spot distances on both limits and scores on the threshold, and carry hit lists
of tens of entries (test_pair_select_cpu.py holds the floors).  One device object with the index of the small genome; the
parameters change between runs with set_params, so every run also says that a change takes effect on an object that has mapped.

Against the oracle, exactly, for every parameter set: coordinates and classes, pileup, insertions, the 13 summary entries, the hit
lists with their fp64 score bits (a class difference can then be told from a score difference), and run_stats' "walks".  Against
the committed reference outputs (rpair_*, make_golden_pair.py) for the two runs the reference mapped.
"""
import numpy as np
import pytest

import fixtures
import pair_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from pecaller_amd import PemapDev
    d = PemapDev(0)
    ix = pc.index()
    d.build_index(ix["genome"], ix["contig_len"])
    yield d
    d.close()


def _batch(name):
    p = pc.set_params(name)
    b1, l1, b2, l2 = pc.reads(p["L"])
    return p, ((b1, l1, b2, l2) if p["paired"] else (b1, l1, None, None))


def _set(dev, p):
    dev.set_params(paired=p["paired"], min_dist=p["min_dist"], max_dist=p["max_dist"], min_align=p["min_align"])
    dev.reset_pileup()


def _mapped_ends(m1, m2):
    return int((m1 > 0).sum()) + (int((m2 > 0).sum()) if m2 is not None else 0)


def _check_results(dev, got, exp, tag):
    """coordinates, classes, pileup, insertions and summary of the batch(es) the device mapped since its pileup was reset"""
    m1, m2, mt = got
    assert np.array_equal(mt, exp["mt"]), (tag, np.nonzero(mt != exp["mt"])[0][:10], mt[mt != exp["mt"]][:10], exp["mt"][mt != exp["mt"]][:10])
    assert np.array_equal(m1, exp["m1"]), (tag, np.nonzero(m1 != exp["m1"])[0][:10])
    if exp["m2"] is not None:
        assert np.array_equal(m2, exp["m2"]), (tag, np.nonzero(m2 != exp["m2"])[0][:10])
    counts, ins = dev.fetch_pileup()
    assert np.array_equal(counts, exp["counts"]), (tag, np.nonzero((counts != exp["counts"]).any(axis=1))[0][:10])
    assert sorted(ins) == exp["ins"], tag
    assert dev.summary().tolist() == exp["summary"].tolist(), tag


def _check_hits(dev, exp, n, tag):
    ends = len(exp["d"])
    dbg = dev.debug_hits(ends * n)
    for which, od in enumerate(exp["d"]):
        nh = dbg["n_hits"][which::ends]
        assert np.array_equal(nh, od["n_hits"]), (tag, which)
        k = np.arange(pc.oracle_py.MAX_HITS)[None, :] < nh[:, None]         # the listed hits of every end
        for key, okey in (("spot", "spot"), ("orient", "orient")):
            assert np.array_equal(dbg[key][which::ends][k], od[okey][k]), (tag, which, key)
        assert np.array_equal(dbg["score"][which::ends][k].view(np.uint64), od["score"][k].view(np.uint64)), (tag, which)
        assert np.array_equal(dbg["start_k"][which::ends][k], od["start"][:, :, 0][k]), (tag, which)
        assert np.array_equal(dbg["start_i"][which::ends][k], od["start"][:, :, 1][k]), (tag, which)


@pytest.mark.parametrize("name", pc.SETS)
def test_selection_equals_oracle(dev, name):
    p, batch = _batch(name)
    exp = pc.expected(name)
    _set(dev, p)
    got = dev.map_batch(*batch)
    stats, _ = dev.run_stats()
    print(name, "classes", np.bincount(got[2], minlength=9).tolist(), "oracle", np.bincount(exp["mt"], minlength=9).tolist())
    _check_hits(dev, exp, len(batch[1]), name)
    _check_results(dev, got, exp, name)
    assert stats["walks"] == _mapped_ends(got[0], got[1]), (name, stats)


def test_uneven_tickets_equal_one_call(dev):
    """the narrow set through submit_batch in uneven pieces, waited for out of order: what the single call gives"""
    p, (b1, l1, b2, l2) = _batch("narrow")
    exp = pc.expected("narrow")
    _set(dev, p)
    cuts = [0, 1, 700, 701, 1999, len(l1)]
    tickets = [(a, b, dev.submit_batch(b1[a:b], l1[a:b], b2[a:b], l2[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
    m1, m2, mt = np.zeros(len(l1), np.uint32), np.zeros(len(l1), np.uint32), np.zeros(len(l1), np.int32)
    for a, b, t in reversed(tickets):
        m1[a:b], m2[a:b], mt[a:b] = dev.wait_batch(t)
    _check_results(dev, (m1, m2, mt), exp, "tickets")


@pytest.mark.parametrize("name", ["rpair_narrow", "rpair_base"])
def test_selection_equals_reference(dev, name):
    """the two runs of the compiled reference on these reads: .mfile words, pileup, insertions, summary rows, the two averages"""
    s = fixtures.SETS[name]
    r1, l1, r2, l2 = fixtures.reads(name)
    dev.set_params(paired=True, **fixtures.params(name))
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(r1, l1, r2, l2)
    assert np.array_equal(m1, fixtures.golden_m(name, 1)) and np.array_equal(m2, fixtures.golden_m(name, 2))
    counts, ins = dev.fetch_pileup()
    fixtures.check_pileup_against_golden(name, counts)
    names, contigs = fixtures.genome(fixtures.genome_of(name))
    assert fixtures.ins_to_named(ins, names, contigs) == fixtures.golden_insertions(name)[0]
    tot, head, rows = fixtures.golden_summary(name)
    sm = dev.summary()
    assert sm[0] == tot
    cls = ["Unique Mate-Paired", "Unique Mate-Paired with slip", "Unique Single End", "Unique Mis-size", "Non-Unique Mate-Paired",
           "Non-Unique Mis-size", "Fragment Mismatch", "Non-unique with no map", "Neither Map"]
    for k, v in zip(cls, sm[4:]):
        assert rows[k] == v, k
    assert np.bincount(mt, minlength=9).tolist() == [rows[k] for k in cls] and rows["All"] == len(l1)
    assert head[3] == "%g" % (sm[1] / sm[0])
    assert head[7] == "%g" % ((sm[2] / sm[3]) if sm[3] else 0.0)
    # the classes this run was made for are there
    assert rows["Unique Mis-size"] >= 5 and rows["Non-Unique Mis-size"] >= 5 and rows["Non-Unique Mate-Paired"] >= 5
