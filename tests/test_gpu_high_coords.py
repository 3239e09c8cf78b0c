"""The mapper above position 2^31 and on the largest genome it accepts (high_cases.py: a small genome behind a filler contig of N).
hg38 has a third of its positions above 2^31, and until here no read of the suite was seeded, windowed, aligned, paired, walked or
piled at a coordinate with bit 31 set.  Every comparison is with the oracle on the same index and exact: m1, m2, mapping_type,
summary(), per end the hit list, per hit the fp64 score bits, the start plane and row, the orientation and the window (its start as
u32), the insertions, and the pileup as records -- fetch_records over the small genome's rows against the oracle's non-zero rows,
and no record anywhere in front of them.  (fetch_pileup() with counts would ask the host for 51 GB.)  test_high_coords_cpu.py
ties these expectations to the reference's printed results and holds the conditions on the read sets.

One device object per placement and genome, closed before the next is made: a genome of 4.29 G letters has a 51 GB pileup beside
the 137 GB of look-up replicas."""
import contextlib
import os
import time

import numpy as np
import pytest

import fixtures
import high_cases as hc
import oracle_py
import refio

pytestmark = pytest.mark.gpu
PARAMS = dict(min_dist=0, max_dist=500, min_align=0.85)


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@contextlib.contextmanager
def _device(ix, bis=False, **env):
    """a device object made under `env` (the knobs are read when it is made) with the index built from the genome's letters; the
    device's own position lists and contig starts are the expected ones; closed on the way out"""
    from pecaller_amd import PemapDev
    t = time.time()
    with _env(**env):
        dev = PemapDev(0)
    try:
        dev.build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
        print("object with its index: %.1f s" % (time.time() - t))
        assert dev.index_info() == (len(ix["mers"]), len(ix["genome"]), len(ix["contig_len"]), 16)
        assert np.array_equal(dev.read_buffer(1, np.uint32), ix["mers"])
        assert np.array_equal(dev.read_buffer(3, np.uint32), ix["contig_starts"])
        yield dev
    finally:
        dev.close()


def _expected(ix, paired, reads, bis=False):
    """the oracle on the same index, on an empty pileup; its array of 6 x gsize counters is freed before this returns"""
    o = oracle_py.Oracle(ix, paired=paired, bisulfite=bis, **PARAMS)
    m1, m2, mt, d1, d2 = o.map_batch(*reads, debug=True, threads=8)
    F, g = ix["F"], ix["g"]
    c = o.counts()[F:F + g]
    nz = np.nonzero(c.astype(np.int64).sum(axis=1))[0]
    rec = np.zeros(len(nz), refio.PILE_DT)
    rec["pos"] = (nz + F).astype(np.uint32)
    rec["c"] = c[nz]
    return dict(m1=m1, m2=m2, mt=mt, d=(d1, d2) if paired else (d1,), rec=rec, ins=o.insertions(), summary=np.array(o.summary()))


def _records_in_front(dev, F):
    """number of pileup records below position F, counted on the device in pieces of at most 2^31 sites"""
    return sum(len(dev.fetch_records(a, min(1 << 31, F - a))) for a in range(0, F, 1 << 31))


def _map_and_compare(dev, ix, name, paired, reads, bis=False, exp=None):
    exp = exp or _expected(ix, paired, reads, bis)
    F, g = ix["F"], ix["g"]
    n = len(reads[1])
    dev.reset_pileup()
    dev.set_params(paired=paired, bisulfite=bis, **PARAMS)
    m1, m2, mt = dev.map_batch(*reads)
    stats, _ = dev.run_stats()
    dbg = dev.debug_hits(2 * n if paired else n)
    _, ins = dev.fetch_pileup(want_counts=False)
    rec = dev.fetch_records(F, g)
    tag = (name, paired, bis)
    print(name, "mapped first ends", int((m1 > 0).sum()), "of", n, "records", len(rec), "insertions", len(ins))
    assert np.array_equal(m1, exp["m1"]), (tag, np.nonzero(m1 != exp["m1"])[0][:10])
    if paired:
        assert np.array_equal(m2, exp["m2"]), (tag, np.nonzero(m2 != exp["m2"])[0][:10])
    assert np.array_equal(mt, exp["mt"]), tag
    assert np.array_equal(np.array(dev.summary()), exp["summary"]), tag
    step = len(exp["d"])
    for which, od in enumerate(exp["d"]):
        nh = dbg["n_hits"][which::step]
        assert np.array_equal(nh, od["n_hits"]), (tag, which, np.nonzero(nh != od["n_hits"])[0][:10])
        for i in np.nonzero(nh)[0]:
            k = nh[i]
            e = step * i + which
            assert np.array_equal(dbg["spot"][e, :k], od["spot"][i, :k]), (tag, e)
            assert np.array_equal(dbg["orient"][e, :k], od["orient"][i, :k]), (tag, e)
            assert np.array_equal(dbg["win_start"][e, :k], od["win_start"][i, :k].astype(np.int64) & 0xFFFFFFFF), (tag, e)
            assert np.array_equal(dbg["win_len"][e, :k], od["win_len"][i, :k]), (tag, e)
            assert np.array_equal(dbg["score"][e, :k].view(np.uint64), od["score"][i, :k].view(np.uint64)), (tag, e, k)
            assert np.array_equal(dbg["start_k"][e, :k], od["start"][i, :k, 0]), (tag, e)
            assert np.array_equal(dbg["start_i"][e, :k], od["start"][i, :k, 1]), (tag, e)
    assert sorted(ins) == exp["ins"], tag
    assert np.array_equal(rec, exp["rec"]), (tag, len(rec), len(exp["rec"]))
    assert _records_in_front(dev, F) == 0, tag
    return dict(m1=m1, m2=m2, mt=mt, stats=stats, exp=exp)


def _golden_r150(F):
    return [np.where(m > 0, (m.astype(np.uint64) + F).astype(np.uint32), np.uint32(0))
            for m in (fixtures.golden_m("r150", k)[:3000] for k in (1, 2))]


@pytest.mark.parametrize("env,replicas", [({}, 8), ({"PEMAP_REPLICAS": "0"}, 0)], ids=["replicas", "no_replicas"])
def test_straddle_g1(env, replicas):
    """g1 with position 2^31 in the middle of contig 5: the golden r150 pairs (also against the reference's own .m1 / .m2 words plus
    F), r100 single-end, 400 + 400 pairs whose fragments cover position 2^31 (mates on two sides of it), the edge pairs; the records
    of [2^31 - 1000, 2^31 + 1000) on their own; through the fused seed kernel on the replicas and through the reference's table.
    (The small sets that follow a set with coverage at 2^31 on the same object are what found reset_pileup returning before its
    fill of the planes had run: the next batch's conversion of plane 0 read the old counts from byte 2^32 of the plane on.)"""
    _, contigs = fixtures.genome()
    F = hc.straddle(contigs)
    ix = hc.high_index(contigs, F)
    with _device(ix, **env) as dev:
        if replicas:
            dev.set_lookup_replicas(8)
        assert dev.lookup_replicas()[0] == replicas
        for name, paired, reads in hc.g1_sets(contigs):
            got = _map_and_compare(dev, ix, name, paired, reads)
            if name == "r150":
                g1, g2 = _golden_r150(F)
                assert np.array_equal(got["m1"], g1) and np.array_equal(got["m2"], g2)
            if name in ("b150", "b16_278"):
                part = dev.fetch_records(hc.HALF - 1000, 2000)
                rec = got["exp"]["rec"]
                assert np.array_equal(part, rec[(rec["pos"] >= hc.HALF - 1000) & (rec["pos"] < hc.HALF + 1000)])
                assert len(part) >= 600 and part["pos"].min() < hc.HALF <= part["pos"].max()


def test_straddle_g1_bisulfite():
    """the bisulfite index and mode: 2,000 ragged pairs of 90 .. 160 bases"""
    _, contigs = fixtures.genome()
    ix = hc.high_index(contigs, hc.straddle(contigs), bisulfite=True)
    with _device(ix, bis=True) as dev:
        for name, paired, reads in hc.bisulfite_sets():
            _map_and_compare(dev, ix, name, paired, reads, bis=True)


def test_straddle_adversarial_genome_every_dp_kernel():
    """the genome of tandem repeats, near-duplicates and planted Ns with the band's and the gapless rule's reads under
    PEMAP_BAND_GATE=1: the gapless rule, the banded DP by both ways in, the full DP, the walk and the insertion log all ran at
    coordinates around and above 2^31 (run_stats), a tenth of the fragments over 2^31 itself; and edge pairs, whose windows are
    clipped at the filler's end and at the genome's"""
    contigs = hc.adversarial_contigs()
    ix = hc.high_index(contigs, hc.straddle(contigs))
    with _device(ix, PEMAP_BAND_GATE="1") as dev:
        for name, paired, reads in hc.adversarial_sets(contigs):
            got = _map_and_compare(dev, ix, name, paired, reads)
            st = got["stats"]
            print(name, {k: st[k] for k in ("gapless", "banded", "gated", "sw_dirs", "walked", "n_ins", "big_ends")})
            if name != "edge":
                for k in ("gapless", "banded", "gated", "sw_dirs", "walked", "n_ins"):
                    assert st[k] > 0, (name, k, st)


@pytest.mark.parametrize("env", [{}, {"PEMAP_FIRST_TIER": "0"}], ids=["default", "no_first_tier"])
def test_straddle_repeat_family(env):
    """the repeat family (190 copies): read-ends of more than 1,024 positions, the seed stage's second tier and pm_seed_kernel's
    spill area"""
    from test_gpu_edge import _repeat_family_genome
    contigs, spots = _repeat_family_genome(4242)
    ix = hc.high_index(contigs, hc.straddle(contigs))
    with _device(ix, **env) as dev:
        for name, paired, reads in hc.family_sets(contigs, spots):
            got = _map_and_compare(dev, ix, name, paired, reads)
            st = got["stats"]
            print(name, {k: st[k] for k in ("big_ends", "mono_ends", "gapless", "banded", "sw_dirs", "walked", "n_ins")})
            assert st["big_ends"] > 0, st


def test_top_g1_without_room_for_the_records():
    """g1 as the last 1.9 M letters of the largest genome: its 36,762 record units do not fit the 398 codes, the replicas are not
    built and the kernels on the reference's table carry the load; requiring the replicas is an error and the object maps on"""
    from pecaller_amd import PemapError
    _, contigs = fixtures.genome()
    F = hc.top(contigs)
    ix = hc.high_index(contigs, F)
    assert len(ix["genome"]) == (1 << 32) - 401 and hc.units(ix) == 36762
    with _device(ix) as dev:
        assert dev.lookup_replicas()[0] == 0
        sets = hc.g1_sets(contigs, ("r150", "edge"))
        got = _map_and_compare(dev, ix, *sets[0])
        g1, g2 = _golden_r150(F)
        assert np.array_equal(got["m1"], g1) and np.array_equal(got["m2"], g2)
        assert int(got["m1"][got["m1"] > 0].min()) - 1 > (1 << 32) - ix["g"] - 401
        with pytest.raises(PemapError, match="36762 record units do not fit"):
            dev.set_lookup_replicas(8)
        assert dev.lookup_replicas()[0] == 0
        dev.set_lookup_replicas(-1)
        assert dev.lookup_replicas()[0] == 0
        _map_and_compare(dev, ix, *sets[0], exp=got["exp"])
        _map_and_compare(dev, ix, *sets[1])


@pytest.mark.parametrize("target", [398, 399], ids=["full", "one_over"])
def test_top_code_space_full_and_one_over(target):
    """ten contigs of 50 kb as the last letters of the largest genome, with copied 16-mers planted until the records take exactly
    the 398 units that fit between the genome's size and 0xFFFFFFFE -- every replica entry of a record is the expected code, the
    last record ends in code 0xFFFFFFFC, positions just below the first code and record numbers just below the marker are told
    apart -- and 399 units, one too many: no replicas, requiring them is an error.  Both map 2,000 pairs as the oracle does, half of
    them laid over the planted copies, a tenth at the genome's very end."""
    from pecaller_amd import PemapError
    contigs, sites = hc.code_space_genome(target)
    ix = hc.high_index(contigs, hc.top(contigs))
    assert hc.units(ix) == target and len(ix["genome"]) == hc.LARGEST
    with _device(ix) as dev:
        if target == 398:
            dev.set_lookup_replicas(8)
            assert dev.lookup_replicas() == (8, 398 * 16)
            kmers, codes, u = hc.record_codes(ix, hc.LARGEST)
            got = np.array([dev.read_buffer(5, np.uint32, 4 * int(k), 4)[0] for k in kmers])
            assert np.array_equal(got, codes)
            assert int(got.max()) + int(u[-1]) - 1 == 0xFFFFFFFC and got.max() == got[-1]
        else:
            assert dev.lookup_replicas()[0] == 0
            with pytest.raises(PemapError, match="399 record units do not fit"):
                dev.set_lookup_replicas(8)
            assert dev.lookup_replicas()[0] == 0
            dev.set_lookup_replicas(-1)
        for name, paired, reads in hc.code_space_sets(contigs, sites):
            got = _map_and_compare(dev, ix, name, paired, reads)
            assert int((got["m1"] > 0).sum()) > 1800


def test_argument_edges():
    """index_alloc refuses a genome of 2^32 - 400 letters and takes one of 2^32 - 401; fetch_records refuses a range that ends
    behind the genome and more than 2^31 sites; the object stays usable after each refusal"""
    from pecaller_amd import PemapDev, PemapError
    dev = PemapDev(0)
    try:
        with pytest.raises(PemapError, match="not supported"):
            dev.index_alloc(0, (1 << 32) - 400, 1)
        dev.index_alloc(0, (1 << 32) - 401, 1)
        g = (1 << 32) - 401
        assert len(dev.fetch_records(g - 1000, 1000)) == 0
        with pytest.raises(PemapError, match="beyond the genome"):
            dev.fetch_records(g - 1000, 1001)
        assert len(dev.fetch_records(g - 1000, 1000)) == 0
        with pytest.raises(PemapError, match="at most 2\\^31 sites"):
            dev.fetch_records(0, (1 << 31) + 1)
        assert len(dev.fetch_records(0, 1 << 31)) == 0
        assert len(dev.fetch_records(g - (1 << 31), 1 << 31)) == 0
        # and a small index built on the same object afterwards maps
        ix = fixtures.index()
        dev.build_index(ix["genome"], ix["contig_len"])
        r1, l1, r2, l2 = (x[:500] for x in fixtures.reads("r150"))
        dev.set_params(paired=True, **PARAMS)
        m1, m2, mt = dev.map_batch(r1, l1, r2, l2)
        assert np.array_equal(m1, fixtures.golden_m("r150", 1)[:500]) and np.array_equal(m2, fixtures.golden_m("r150", 2)[:500])
    finally:
        dev.close()
