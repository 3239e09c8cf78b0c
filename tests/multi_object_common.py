"""Shared by tests/test_gpu_multi_object.py and the child process it starts (not a test module): two device objects of one process,
one mapping the first part of the golden r150 pairs and one the rest, and the byte-for-byte check of pemap_dev_absorb's counter sum."""
import numpy as np
import fixtures

CUT = 9001            # A maps pairs [0, CUT), B the rest: uneven on purpose
PAIRED_CLASSES = ["Unique Mate-Paired", "Unique Mate-Paired with slip", "Unique Single End", "Unique Mis-size", "Non-Unique Mate-Paired",
                  "Non-Unique Mis-size", "Fragment Mismatch", "Non-unique with no map", "Neither Map"]


def map_range(dev, lo, hi):
    r1, l1, r2, l2 = fixtures.reads("r150")
    dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
    return dev.map_batch(r1[lo:hi], l1[lo:hi], r2[lo:hi], l2[lo:hi])


def map_halves(A, B):
    n = len(fixtures.reads("r150")[1])
    ma, mb = map_range(A, 0, CUT), map_range(B, CUT, n)
    for k in (0, 1):
        assert np.array_equal(np.concatenate([ma[k], mb[k]]), fixtures.golden_m("r150", k + 1))
    return ma, mb


def absorb_checked(A, B):
    """A.absorb(B); A's whole buffer 4 (padding words too) must then be the element-wise sum modulo 2^16 of the two buffers as they
    were, and B's must be zero"""
    a, b = A.read_buffer(4, np.uint16), B.read_buffer(4, np.uint16)
    assert a.shape == b.shape and a.any() and b.any()
    A.absorb(B)
    want = a + b                # numpy's uint16 addition wraps
    assert want.dtype == np.uint16
    got = A.read_buffer(4, np.uint16)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
    assert not B.read_buffer(4, np.uint16).any()
    return a, b


def check_sum_is_the_whole_read_set(A, counts=None, ins=None):
    """A's pileup, insertions and summary are the reference's for all of r150"""
    if counts is None:
        counts, ins = A.fetch_pileup()
    fixtures.check_pileup_against_golden("r150", counts)
    names, contigs = fixtures.genome()
    assert fixtures.ins_to_named(ins, names, contigs) == fixtures.golden_insertions("r150")[0]
    tot, head, rows = fixtures.golden_summary("r150")
    sm = A.summary()
    assert sm[0] == tot
    assert head[3] == "%g" % (sm[1] / sm[0]) and head[7] == "%g" % (sm[2] / sm[3])
    assert [rows[c] for c in PAIRED_CLASSES] == [int(x) for x in sm[4:13]]
    assert rows["All"] == int(sm[4:13].sum())


def check_emptied(B):
    assert not B.summary().any()
    assert len(B.fetch_records()) == 0
    assert B.fetch_pileup(want_counts=False)[1] == []
