"""One object taken through every way of staging reads in turn (pecaller_amd/csrc/pemap_capi.hip: ensure_reads, ring_setup, ring_leave
and the entries on top of them): a resident paired set, a resident single-end set with fewer rows and another stride (the mates' arrays
are made again), three batches in flight (the ring takes the arrays over), a resident set again (the ring is left), the same pairs as
fastq text staged and then submitted, and close().  Expected: every paired step returns the reference's golden positions for its pairs and
the oracle's mapping types, the single-end step what a fresh object returns (and the oracle), and pemap_dev_pipeline_stats [5] (set-ups of the ring)
moves by one at the first submit_batch and at the submit_fastq and nowhere else.  (The golden set holds positions only: its mapping types
exist as the summary's totals over all 20,000 pairs, which is how test_map_matches_reference_golden checks them.  For 64 pairs the
per-row reference is the CPU oracle, which the golden summary validates on the whole set.)"""
import numpy as np
import pytest
import fixtures
import oracle_py

pytestmark = pytest.mark.gpu
N, N_SINGLE, SETUPS = 64, 32, 5
PARAMS = dict(min_dist=0, max_dist=500, min_align=0.85)


def _text_of(rows, lens):
    flat, stride = rows.tobytes(), rows.shape[1]
    return b"".join(b"@g%d\n%s\n+\n%s\n" % (i, flat[i * stride:i * stride + int(n)], b"I" * int(n)) for i, n in enumerate(lens))


def _fresh_single(src, rows, lens):
    """the same single reads on an object of their own (src's index, no replicas: the results do not depend on the layout)"""
    from pecaller_amd import PemapDev
    d = PemapDev(0)
    try:
        d.set_lookup_replicas(0)
        d.index_share(src)
        d.set_params(paired=False, **PARAMS)
        d.stage_reads(rows, lens)
        d.run()
        m1, _, mt = d.collect()
    finally:
        d.close()
    return m1, mt


def test_one_object_through_every_staging_mode():
    from pecaller_amd import PemapDev
    ix = fixtures.index()
    r1, l1, r2, l2 = (np.ascontiguousarray(a[:N]) for a in fixtures.reads("r150"))
    assert max(l1.max(), l2.max()) <= 160
    r1, r2 = np.ascontiguousarray(r1[:, :160]), np.ascontiguousarray(r2[:, :160])
    g1, g2 = fixtures.golden_m("r150", 1)[:N], fixtures.golden_m("r150", 2)[:N]
    gt = oracle_py.Oracle(ix, paired=True, **PARAMS).map_batch(r1, l1, r2, l2, threads=4)[2]
    wide = np.zeros((N_SINGLE, 256), np.uint8)
    wide[:, :160] = r1[:N_SINGLE]
    lw = np.ascontiguousarray(l1[:N_SINGLE])
    o1, _, ot = oracle_py.Oracle(ix, paired=False, **PARAMS).map_batch(wide, lw, threads=4)[:3]
    text1, text2 = _text_of(r1, l1), _text_of(r2, l2)

    def check_pairs(step, got, lo=0, hi=N):
        m1, m2, mt = got
        assert np.array_equal(m1, g1[lo:hi]), (step, "m1 differs at", np.nonzero(m1 != g1[lo:hi])[0][:10])
        assert np.array_equal(m2, g2[lo:hi]), (step, "m2 differs at", np.nonzero(m2 != g2[lo:hi])[0][:10])
        assert np.array_equal(mt, gt[lo:hi]), (step, "mapping types differ at", np.nonzero(mt != gt[lo:hi])[0][:10])

    dev = PemapDev(0)
    setups = []
    try:
        dev.build_index(ix["genome"], ix["contig_len"])
        setups.append(dev.pipeline_stats()[SETUPS])
        # 1: a resident paired set at stride 160
        dev.set_params(paired=True, **PARAMS)
        dev.stage_reads(r1, l1, r2, l2)
        assert dev.staged_info() == (N, 160, 1)
        dev.run()
        check_pairs(1, dev.collect())
        setups.append(dev.pipeline_stats()[SETUPS])
        # 2: fewer rows, another stride, one mate
        dev.set_params(paired=False, **PARAMS)
        dev.stage_reads(wide, lw)
        assert dev.staged_info() == (N_SINGLE, 256, 0)
        dev.run()
        s1, _, st = dev.collect()
        f1, ft = _fresh_single(dev, wide, lw)
        assert np.array_equal(s1, f1) and np.array_equal(st, ft), (2, np.nonzero(s1 != f1)[0][:10])
        assert np.array_equal(s1, o1) and np.array_equal(st, ot), (2, "oracle", np.nonzero(s1 != o1)[0][:10])
        setups.append(dev.pipeline_stats()[SETUPS])
        # 3: the ring takes the arrays over; three batches in flight, then the waits
        dev.set_params(paired=True, **PARAMS)
        cuts = [(0, N), (0, 16), (0, N)]
        tickets = [dev.submit_batch(r1[a:b], l1[a:b], r2[a:b], l2[a:b]) for a, b in cuts]
        for (a, b), t in zip(cuts, tickets):
            check_pairs(3, dev.wait_batch(t), a, b)
        setups.append(dev.pipeline_stats()[SETUPS])
        # 4: a resident set again: the ring is left
        dev.stage_reads(r1, l1, r2, l2)
        assert dev.staged_info() == (N, 160, 1)
        dev.run()
        check_pairs(4, dev.collect())
        setups.append(dev.pipeline_stats()[SETUPS])
        # 5: the same pairs staged as text
        res = dev.stage_fastq(text1, text2, max_records=1 << 10, stride=288)
        assert res["n"] == N, res
        assert dev.staged_info() == (N, 288, 1)
        dev.run()
        check_pairs(5, dev.collect())
        setups.append(dev.pipeline_stats()[SETUPS])
        # 6: and submitted as text
        res, t = dev.submit_fastq(text1, text2, max_records=1 << 10, stride=288)
        assert res["n"] == N, res
        check_pairs(6, dev.wait_batch(t))
        setups.append(dev.pipeline_stats()[SETUPS])
    finally:
        dev.close()         # 7
    moved = [b - a for a, b in zip(setups, setups[1:])]
    print("ring set-ups per step", moved)
    assert moved == [0, 0, 1, 0, 0, 1], moved
