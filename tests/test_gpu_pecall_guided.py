"""Pileup columns at every position of a list of intervals, made on the device (pecall_dev_sites_stage_records_guided /
_call_records_guided: the guide-file loop of pecaller.c:941-1039): the columns against a numpy build, the rejection of bad streams
and of bad interval lists, and the caller behind it against the caller on host-built columns."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GEN = b"ACGTDIMRWSYKEHN"
LUT = np.full(256, 255, np.uint8)
for _k, _ch in enumerate(GEN):
    LUT[_ch] = _k
REC = np.dtype([("pos", "<u4"), ("counts", "<u2", (6,))])
BIG = (1 << 18) + 37     # 65 blocks of the scan: its second level has several block sums


@pytest.fixture(scope="module")
def dev():
    from pecaller_amd.pecall import PecallDev
    d = PecallDev(0)
    yield d
    d.close()


# slots every case's list is built around (spans are 1000 at least)
EMPTY_IV = (100, 10)            # an interval no sample has a record in
GAP = (110, 450)                # no interval in it, records of every sample, sample 0 in every slot


def intervals(span, seed):
    """-> first, count, chrom byte per interval: ascending, disjoint.  An interval at slot 0; single slots 5 and 7 (3, 4 and 6 are
    unmarked slots of the same run of 8); 12..19 crosses a multiple of 16; 40..46 and 47..49 are adjacent; 60..69 crosses slot 64, a
    run boundary at 8, 16 and 32 slots a run; 100..109 holds no record; nothing in 110..449; random ones from 460 on; at span
    4099 one over slot 4096; the last ends at span - 1"""
    rng = np.random.default_rng(seed)
    iv = [(0, 3), (5, 1), (7, 1), (12, 8), (40, 7), (47, 3), (60, 10), EMPTY_IV]
    stop = span - 20
    n_rand = (stop - 460) // 20 + 1
    at = 460 + np.cumsum(rng.integers(1, 41, n_rand) + rng.integers(1, 31, n_rand))      # ends, each a gap of 1..30 behind its predecessor
    ln = rng.integers(1, 41, n_rand)
    ok = np.ones(n_rand, bool)
    ok[1:] = at[1:] - ln[1:] > at[:-1]
    ok &= (at - ln >= 460) & (at <= stop)
    iv += [(int(e - l), int(l)) for e, l in zip(at[ok], ln[ok])]
    if span == 4099:
        iv = [x for x in iv if x[0] + x[1] <= 4080] + [(4090, 7)]
    iv.append((span - 2, 2))
    first = np.array([x[0] for x in iv], np.uint32)
    count = np.array([x[1] for x in iv], np.uint32)
    chrom = ((np.arange(len(iv)) * 7) % 4).astype(np.uint8)
    chrom[chrom >= 2] |= 16
    return first, count, chrom


def synth(indiv, span, p0, seed, real=False):
    """seeded records of a range: 35 % of the slots per sample (2 % for some), none in EMPTY_IV; sample 0 has a record in every slot
    of the gap and at the unmarked slots 3, 4 and 6; the last sample at slot 0 and span - 1.  With three samples or more sample 1 has no
    record at all.  real: depths on the reference allele, a second allele here and there (for the caller) -> per-sample arrays"""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(indiv):
        if indiv >= 3 and i == 1:
            slots = np.zeros(0, np.int64)
        else:
            slots = np.flatnonzero(rng.random(span) < (0.02 if i % 7 == 3 else 0.35))
            if i == 0:
                slots = np.union1d(slots, np.concatenate([np.arange(GAP[0] + 5, GAP[1] - 5), [3, 4, 6]]))
            if i == indiv - 1:
                slots = np.union1d(slots, [0, span - 1])
            slots = slots[(slots < EMPTY_IV[0]) | (slots >= EMPTY_IV[0] + EMPTY_IV[1])]
        r = np.zeros(len(slots), REC)
        r["pos"] = (p0 + slots).astype(np.uint32)
        if real:
            c = np.zeros((len(slots), 6), np.uint16)
            c[np.arange(len(slots)), slots % 4] = rng.integers(0, 45, len(slots))
            # every 11th slot is a variant position: half the samples carry a second allele there; a stray read elsewhere
            alt = ((slots % 11 == 5) & (rng.random(len(slots)) < 0.5)) | (rng.random(len(slots)) < 0.01)
            c[alt, (slots[alt] + 1 + (slots[alt] // 4) % 3) % 4] = rng.integers(1, 30, int(alt.sum()))
        else:
            c = rng.integers(0, 60, (len(slots), 6)).astype(np.uint16)
            c[rng.random((len(slots), 6)) < 0.01] = 65535
        r["counts"] = c
        recs.append(r)
    return recs


def numpy_columns(recs, span, p0, letters, first, count, chrom):
    indiv = len(recs)
    marks = np.zeros(span, bool)
    cy = np.zeros(span, np.uint8)
    for k in range(len(first)):
        marks[first[k]:first[k] + count[k]] = True
        if chrom is not None:
            cy[first[k]:first[k] + count[k]] = chrom[k]
    col_slot = np.flatnonzero(marks).astype(np.uint32)
    col_of = np.cumsum(marks) - 1
    reads = np.zeros((len(col_slot), indiv, 6), np.uint16)
    for i, r in enumerate(recs):
        slot = r["pos"].astype(np.int64) - p0
        at = marks[slot]
        reads[col_of[slot[at]], i] = r["counts"][at]
    lt = np.full(span, 255, np.uint8)
    lt[:len(letters)] = LUT[np.frombuffer(letters, np.uint8)]
    return col_slot, reads, lt[col_slot], cy[col_slot]


def letters_of(ref_len, seed, real=False):
    rng = np.random.default_rng(seed + 99)
    if real:
        a = np.frombuffer(b"ACGT", np.uint8)[np.arange(ref_len) % 4].copy()
        a[rng.random(ref_len) < 0.01] = ord("N")
        return a.tobytes()
    alphabet = np.frombuffer(b"ACGTACGTACGTNMa\0DIRWSYKEHcgtx", np.uint8)
    return alphabet[rng.integers(0, len(alphabet), ref_len)].tobytes()


def check_guided(dev, indiv, span, p0, seed, iv, short_ref):
    first, count, chrom = iv
    recs = synth(indiv, span, p0, seed)
    letters = letters_of(span - 7 if short_ref else span, seed)
    exp_slot, exp_reads, exp_ref, exp_cy = numpy_columns(recs, span, p0, letters, first, count, chrom)
    n_cols, col_slot = dev.sites_stage_records_guided(recs, p0, span, letters, first, count, chrom)
    assert n_cols == int(count.sum()) == len(exp_slot)
    assert np.array_equal(col_slot, exp_slot)
    reads, ref, cy = dev.sites_gather()
    assert reads.shape == exp_reads.shape and np.array_equal(reads, exp_reads)
    assert np.array_equal(ref, exp_ref)
    assert np.array_equal(cy, exp_cy)
    return recs, exp_reads


CASES = [(n, s) for n in (1, 3, 64, 65, 129, 512) for s in (1000, 4099)] + [(20, 4099), (20, BIG)]


@pytest.mark.parametrize("indiv,span", CASES)
def test_guided_columns_against_numpy(dev, indiv, span):
    seed = indiv * 7 + span
    # (the range of one case ends at the last 32-bit position)
    p0 = (1 << 32) - span if (indiv, span) == (20, 4099) else 1000003 + indiv
    first, count, chrom = intervals(span, seed)
    # what the list is said to hold
    assert first[0] == 0 and first[-1] + count[-1] == span and (count == 1).sum() >= 2
    assert np.any(first[1:] == first[:-1] + count[:-1])
    assert span != 4099 or np.any((first < 4096) & (first + count > 4096))
    recs, exp_reads = check_guided(dev, indiv, span, p0, seed, (first, count, chrom if (indiv + span) % 2 == 0 else None), short_ref=span != 1000)
    e0 = int(np.flatnonzero(first == EMPTY_IV[0])[0])
    c0 = int(count[:e0].sum())
    assert not exp_reads[c0:c0 + EMPTY_IV[1]].any()        # the interval nobody covers: columns of zeros
    slots0 = recs[0]["pos"].astype(np.int64) - p0
    assert {3, 4, 6} <= set(slots0.tolist()) and ((slots0 >= GAP[0]) & (slots0 < GAP[1])).sum() > 300


def test_one_interval_over_the_whole_span_and_none(dev):
    span = 4099
    whole = (np.array([0], np.uint32), np.array([span], np.uint32), np.array([3 | 16], np.uint8))
    check_guided(dev, 5, span, 777, 4, whole, short_ref=True)
    none = np.zeros(0, np.uint32)
    n_cols, col_slot = dev.sites_stage_records_guided(synth(5, span, 777, 4), 777, span, b"A" * span, none, none)
    assert n_cols == 0 and len(col_slot) == 0
    with pytest.raises(Exception):                # nothing is staged
        dev.sites_run()


def test_intervals_without_any_record(dev):
    span = 1000
    first, count, chrom = intervals(span, 1)
    letters = letters_of(span, 1)
    empty = [np.zeros(0, REC)] * 3
    exp_slot, exp_reads, exp_ref, exp_cy = numpy_columns(empty, span, 50, letters, first, count, chrom)
    n_cols, col_slot = dev.sites_stage_records_guided(empty, 50, span, letters, first, count, chrom)
    reads, ref, cy = dev.sites_gather()
    assert n_cols == len(exp_slot) and np.array_equal(col_slot, exp_slot) and not reads.any() and reads.shape == exp_reads.shape
    assert np.array_equal(ref, exp_ref) and np.array_equal(cy, exp_cy)


def test_small_after_large_on_one_object(dev):
    """a larger range, then a smaller one with fewer samples and intervals: nothing of the first shows in the second"""
    check_guided(dev, 64, 4099, 5000, 1, intervals(4099, 1), True)
    check_guided(dev, 3, 1000, 700, 2, intervals(1000, 2), False)
    check_guided(dev, 64, 4099, 5000, 1, intervals(4099, 1), True)


@pytest.mark.parametrize("what", ["equal", "descends", "below_p0", "at_end", "descends_in_the_gap"])
def test_rejects_bad_streams_without_a_fault(dev, what):
    from pecaller_amd.pecall import PecallUnordered, RC_UNORDERED
    p0, span, indiv = 4000, 1000, 6
    iv = intervals(span, 11)
    good = synth(indiv, span, p0, 11)
    bad = [r.copy() for r in good]
    if what == "equal":
        s, j = 3, 7
        bad[s]["pos"][j] = bad[s]["pos"][j - 1]
    elif what == "descends":
        s, j = 3, 7
        bad[s]["pos"][j] = bad[s]["pos"][j - 1] - 1
    elif what == "below_p0":
        s, j = 2, 0
        bad[s]["pos"][j] = p0 - 1
    elif what == "at_end":
        s, j = 4, len(bad[4]) - 1
        bad[s]["pos"][j] = p0 + span
    else:
        # two records of the gap, where no interval is: checked like the others
        s = 0
        j = int(np.flatnonzero(bad[0]["pos"] == p0 + 300)[0])
        bad[s]["pos"][j] = bad[s]["pos"][j - 1] - 1
    bad[5]["pos"][3] = bad[5]["pos"][2]          # (a later sample has one too: the lowest is named)
    with pytest.raises(PecallUnordered) as e:
        dev.sites_stage_records_guided(bad, p0, span, b"A" * span, *iv)
    assert e.value.rc == RC_UNORDERED
    assert "sample %d, record %d " % (s, j) in str(e.value), str(e.value)
    with pytest.raises(Exception):                # nothing is staged
        dev.sites_run()
    check_guided(dev, indiv, span, p0, 11, iv, False)


@pytest.mark.parametrize("what", ["overlap", "descends", "empty", "overlong", "beyond"])
def test_rejects_bad_intervals(dev, what):
    from pecaller_amd.pemap import PemapError
    from pecaller_amd.pecall import PecallUnordered, RC_UNORDERED
    p0, span, indiv = 4000, 1000, 4
    first, count, chrom = intervals(span, 12)
    first, count = first.copy(), count.copy()
    if what == "overlap":
        count[3] = first[4] - first[3] + 1
    elif what == "descends":
        first[[4, 5]] = first[[5, 4]]
        count[[4, 5]] = count[[5, 4]]
    elif what == "empty":
        count[2] = 0
    elif what == "overlong":
        count[-1] += 1
    else:
        first[-1] = 0xfffffff0
    recs = synth(indiv, span, p0, 12)
    with pytest.raises(PemapError) as e:
        dev.sites_stage_records_guided(recs, p0, span, b"A" * span, first, count, chrom)
    assert not isinstance(e.value, PecallUnordered)
    # the C entry itself: no arrays for a list that is not empty
    n = np.array([len(r) for r in recs], np.uint64)
    ptrs = (C.c_void_p * indiv)(*[r.ctypes.data if len(r) else None for r in recs])
    n_cols = C.c_long(0)
    rc = dev.L.pecall_dev_sites_stage_records_guided(dev.h, C.addressof(ptrs), n.ctypes.data, indiv, p0, span, None, 0, None, None, None, 3, C.byref(n_cols), None)
    assert rc not in (0, RC_UNORDERED)
    check_guided(dev, indiv, span, p0, 12, intervals(span, 12), False)   # the object is as usable as before


@pytest.mark.parametrize("indiv,span", [(64, 4099), (129, 1000)])
def test_call_records_guided_against_the_caller_on_host_columns(indiv, span):
    from pecaller_amd.pecall import PecallDev
    p0, seed = 70001, indiv + span
    first, count, chrom = intervals(span, seed)
    assert np.any(chrom == (2 | 16)) and np.any(chrom == (3 | 16)) and np.any(chrom == 0)
    recs = synth(indiv, span, p0, seed, real=True)
    letters = letters_of(span, seed, real=True)
    exp_slot, exp_reads, exp_ref, exp_cy = numpy_columns(recs, span, p0, letters, first, count, chrom)
    dev, host = PecallDev(0), PecallDev(0)
    call, sp, typ, ac, npass, col_slot = dev.call_records_guided(recs, p0, span, letters, first, count, chrom, cap=span)
    den = dev.denovo.copy()
    exp = host.call_sites_sparse(exp_reads, exp_ref, chrom=exp_cy, cap=span)
    assert np.array_equal(col_slot, exp_slot)
    assert np.array_equal(call, exp[0]) and np.array_equal(typ, exp[2]) and np.array_equal(ac, exp[3]) and np.array_equal(npass, exp[4])
    assert np.array_equal(den, host.denovo[:len(exp_slot)])
    assert np.array_equal(sp[0], exp[1][0]) and sp[1].tobytes() == exp[1][1].tobytes()
    assert (typ > 0).sum() >= 3 and len(sp[0]) >= 3         # (variant columns and posteriors below 1 among them: the CPU oracle finds 5 and 6 at the least)
    # the staged columns are still there behind the call
    reads, ref, cy = dev.sites_gather()
    assert np.array_equal(reads, exp_reads) and np.array_equal(ref, exp_ref) and np.array_equal(cy, exp_cy)
    dev.close()
    host.close()
