"""Pileup columns made on the device from per-sample record streams (pecall_dev_sites_stage_records / _sites_gather /
_call_records): the merge against a numpy build of the columns, the rejection of streams that do not ascend, and the caller
behind it against the caller on host-built columns and the reference's own text."""
import ctypes as C
import os
import numpy as np
import pytest
import oracle_py
import pecall_sites_fixture as fx
import refio

pytestmark = pytest.mark.gpu

GEN = b"ACGTDIMRWSYKEHN"
LUT = np.full(256, 255, np.uint8)
for _k, _ch in enumerate(GEN):
    LUT[_ch] = _k
REC = np.dtype([("pos", "<u4"), ("counts", "<u2", (6,))])


@pytest.fixture(scope="module")
def dev():
    from pecaller_amd.pecall import PecallDev
    d = PecallDev(0)
    yield d
    d.close()


def synth(indiv, span, p0, mode, seed):
    """seeded records of a range.  mode "full": sample 0 has a record in every slot (slots 0 and span - 1 with it); "gap": nobody
    has, a run of 300 slots (more than nine workgroups' runs of 32) holds one single record -- with six zero counts -- and the last sample has
    records at slot 0 and slot span - 1.  With three samples or more sample 1 has no record at all.  Some counts are 65,535; one
    record with six zero counts lies at a slot that no other sample has a record in.  -> per-sample structured arrays"""
    rng = np.random.default_rng(seed)
    gap0 = span // 3
    gap = (gap0, min(gap0 + 300, span - 1))
    zero_slot = 5 if mode == "full" else (gap[0] + gap[1]) // 2
    zero_sample = 0 if (mode == "full" or indiv < 3) else 2
    recs = []
    for i in range(indiv):
        if mode == "full" and i == 0:
            slots = np.arange(span)
        elif indiv >= 3 and i == 1:
            slots = np.zeros(0, np.int64)
        else:
            slots = np.flatnonzero(rng.random(span) < (0.02 if i % 7 == 3 else 0.35))
            if mode == "gap":
                slots = slots[(slots < gap[0]) | (slots >= gap[1])]
                if i == indiv - 1:
                    slots = np.union1d(slots, [0, span - 1])
        slots = slots[slots != zero_slot] if i != zero_sample else np.union1d(slots, [zero_slot])
        r = np.zeros(len(slots), REC)
        r["pos"] = (p0 + slots).astype(np.uint32)
        c = rng.integers(0, 60, (len(slots), 6)).astype(np.uint16)
        c[rng.random((len(slots), 6)) < 0.01] = 65535
        if i == zero_sample:
            c[slots == zero_slot] = 0
        r["counts"] = c
        recs.append(r)
    return recs


def numpy_columns(recs, span, p0, letters, chrom):
    indiv = len(recs)
    marks = np.zeros(span, bool)
    for r in recs:
        marks[r["pos"].astype(np.int64) - p0] = True
    col_slot = np.flatnonzero(marks).astype(np.uint32)
    col_of = np.cumsum(marks) - 1
    reads = np.zeros((len(col_slot), indiv, 6), np.uint16)
    for i, r in enumerate(recs):
        reads[col_of[r["pos"].astype(np.int64) - p0], i] = r["counts"]
    lt = np.full(span, 255, np.uint8)
    lt[:len(letters)] = LUT[np.frombuffer(letters, np.uint8)]
    cy = np.zeros(span, np.uint8) if chrom is None else chrom
    return col_slot, reads, lt[col_slot], cy[col_slot]


def letters_of(span, ref_len, seed):
    rng = np.random.default_rng(seed + 99)
    alphabet = np.frombuffer(b"ACGTACGTACGTNMa\0DIRWSYKEHcgtx", np.uint8)
    return alphabet[rng.integers(0, len(alphabet), ref_len)].tobytes()


def check_merge(dev, indiv, span, p0, mode, seed, with_chrom, short_ref):
    recs = synth(indiv, span, p0, mode, seed)
    letters = letters_of(span, span - 7 if short_ref else span, seed)
    chrom = None
    if with_chrom:
        chrom = np.zeros(span, np.uint8)
        chrom[span // 2:] = 2
    exp_slot, exp_reads, exp_ref, exp_cy = numpy_columns(recs, span, p0, letters, chrom)
    n_cols, col_slot = dev.sites_stage_records(recs, p0, span, letters, chrom=chrom)
    assert n_cols == len(exp_slot)
    assert np.array_equal(col_slot, exp_slot)
    reads, ref, cy = dev.sites_gather()
    assert reads.shape == exp_reads.shape and np.array_equal(reads, exp_reads)
    assert np.array_equal(ref, exp_ref)
    assert np.array_equal(cy, exp_cy)
    # a listed subset, in an order of its own
    pick = np.array([n_cols - 1, 0, n_cols // 2, n_cols // 2], np.uint32)
    r2, f2, c2 = dev.sites_gather(pick)
    assert np.array_equal(r2, exp_reads[pick]) and np.array_equal(f2, exp_ref[pick]) and np.array_equal(c2, exp_cy[pick])
    return recs, exp_slot


BIG = (1 << 18) + 37     # 65 blocks of the scan: its second level has several block sums
# every number of samples with spans that are no multiple of a tile (8 / 16 / 32 slots) or of a scan block (4,096); the span of
# 2^18 + 37 with 1, 20, 64 and 65 samples (with 100 and 512 its columns alone are 0.3 and 1.6 GB: not a test of seconds)
CASES = [(n, s, "full" if (k + j) % 2 == 0 else "gap") for k, n in enumerate((1, 20, 64, 65, 100, 512)) for j, s in enumerate((1000, 4099))]
CASES += [(1, BIG, "gap"), (20, BIG, "gap"), (64, BIG, "full"), (65, BIG, "gap")]


@pytest.mark.parametrize("indiv,span,mode", CASES)
def test_merge_against_numpy(dev, indiv, span, mode):
    seed = indiv * 7 + span
    # (the range of one case ends at the last 32-bit position)
    p0 = (1 << 32) - span if (indiv, span) == (20, 4099) else 1000003 + indiv
    check_merge(dev, indiv, span, p0, mode, seed, with_chrom=(indiv + span) % 2 == 0, short_ref=span != 1000)


def test_merge_small_after_large_on_one_object(dev):
    """a larger range, then a smaller one with fewer samples: nothing of the first shows in the second; then the larger again"""
    check_merge(dev, 64, 4099, 5000, "full", 1, True, True)
    check_merge(dev, 20, 1000, 700, "gap", 2, False, False)
    check_merge(dev, 64, 4099, 5000, "full", 1, True, True)


def test_no_records_at_all(dev):
    n_cols, col_slot = dev.sites_stage_records([np.zeros(0, REC)] * 3, 10, 100, b"A" * 100)
    assert n_cols == 0 and len(col_slot) == 0


@pytest.mark.parametrize("what", ["equal", "descends", "below_p0", "at_end"])
def test_rejects_unordered_streams_without_a_fault(dev, what):
    from pecaller_amd.pecall import PecallUnordered, RC_UNORDERED
    p0, span, indiv = 4000, 1000, 6
    good = synth(indiv, span, p0, "gap", 11)
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
    else:
        s, j = 4, len(bad[4]) - 1
        bad[s]["pos"][j] = p0 + span
    bad[5]["pos"][3] = bad[5]["pos"][2]          # (a later sample has one too: the lowest is named)
    with pytest.raises(PecallUnordered) as e:
        dev.sites_stage_records(bad, p0, span, b"A" * span)
    assert e.value.rc == RC_UNORDERED
    assert "sample %d, record %d " % (s, j) in str(e.value), str(e.value)
    with pytest.raises(Exception):                # nothing is staged
        dev.sites_run()
    letters = letters_of(span, span, 5)
    exp_slot, exp_reads, exp_ref, _ = numpy_columns(good, span, p0, letters, None)
    n_cols, col_slot = dev.sites_stage_records(good, p0, span, letters)
    reads, ref, _ = dev.sites_gather()
    assert n_cols == len(exp_slot) and np.array_equal(col_slot, exp_slot) and np.array_equal(reads, exp_reads) and np.array_equal(ref, exp_ref)


def test_argument_errors(dev):
    from pecaller_amd.pemap import PemapError
    from pecaller_amd.pecall import PecallUnordered, RC_UNORDERED
    good = synth(4, 100, 50, "gap", 3)
    for recs, span in ((good, 0), ([np.zeros(0, REC)] * 513, 100)):
        with pytest.raises(PemapError) as e:
            dev.sites_stage_records(recs, 50, span, b"")
        assert not isinstance(e.value, PecallUnordered)
    n = np.array([1, 1], np.uint64)
    n_cols = C.c_long(0)
    rc = dev.L.pecall_dev_sites_stage_records(dev.h, None, n.ctypes.data, 2, 50, 100, None, 0, None, C.byref(n_cols), None)
    assert rc not in (0, RC_UNORDERED)
    n_cols2, _ = dev.sites_stage_records(good, 50, 100, b"ACGT" * 25)   # the object is as usable as before
    assert n_cols2 > 0


# ---- end to end on the reference's fixtures

def fixture_records(f):
    """records where a sample's six counts are not all zero, as the CLI test writes its files"""
    out = []
    for s in range(f["reads"].shape[1]):
        keep = f["reads"][:, s].sum(1) > 0
        r = np.zeros(int(keep.sum()), REC)
        r["pos"] = f["pos"][keep].astype(np.uint32)
        r["counts"] = f["reads"][keep, s]
        out.append(r)
    return out


def dense(n, indiv, sparse):
    p = np.ones((n, indiv))
    p[sparse[0]] = sparse[1]
    return p


# (the last case: chunks of 256 columns, the lower clamp, so that the resident seam runs the fixture's columns as 24 chunks)
E2E = [pytest.param(tag, split, None, id="%s-%s" % (split, tag)) for split in (None, 1024) for tag in ("pecall_sites", "pecall_wide", "pecall_ped")]
E2E.append(pytest.param("pecall_sites", None, 8, id="None-pecall_sites-chunks_of_256"))


@pytest.mark.parametrize("tag,split,chunk_log2", E2E)
def test_call_records_end_to_end(tag, split, chunk_log2, monkeypatch):
    from pecaller_amd.pecall import PecallDev
    if chunk_log2 is not None:
        monkeypatch.setenv("PECALL_CHUNK_LOG2", str(chunk_log2))
    f = fx.load(tag)
    _, seqs = refio.read_fasta(os.path.join(fx.GOLD, "g1.fa.gz"))
    seq = np.concatenate(seqs)
    pos = f["pos"].astype(np.int64)
    recs = fixture_records(f)
    indiv = len(recs)
    dev, host = PecallDev(0), PecallDev(0)
    if "ped" in f:
        ped = f["ped"]
        off, lst = oracle_py.kid_lists(ped["dad"], ped["mom"], ped["order"])
        for d in (dev, host):
            d.set_pedigree(ped["dad"], ped["mom"], ped["sex"], off, lst, ped["denovo_rate"])
    if split is None:
        ranges = [(int(pos[0]), int(pos[-1] - pos[0] + 1))]
    else:
        # (the first range lies in front of every record: no columns; the fixture's last range is partly empty)
        first = int(pos[0]) - split
        ranges = [(p, split) for p in range(first, int(pos[-1]) + 1, split)]
    rows, srows = {}, {}
    has = f["reads"].sum(2) > 0
    for p0, span in ranges:
        part = [r[(r["pos"] >= p0) & (r["pos"] < p0 + span)] for r in recs]
        got = dev.call_records(part, p0, span, seq[p0:p0 + span].tobytes())
        call, sp, typ, ac, npass, col_slot = got
        den = dev.denovo.copy()
        idx = np.flatnonzero((pos >= p0) & (pos < p0 + span) & has.any(1))
        assert len(col_slot) == len(idx)
        if len(idx) == 0:
            assert split is not None
            continue
        assert np.array_equal(col_slot.astype(np.int64) + p0, pos[idx])
        # the caller on the host-built columns of the same positions: the same kernels on the same bytes
        exp = host.call_sites_sparse(f["reads"][idx], LUT[seq[pos[idx]]])
        hden = host.denovo.copy()
        assert np.array_equal(call, exp[0]) and np.array_equal(typ, exp[2]) and np.array_equal(ac, exp[3]) and np.array_equal(npass, exp[4])
        assert np.array_equal(den, hden[:len(idx)])
        assert np.array_equal(sp[0], exp[1][0]) and sp[1].tobytes() == exp[1][1].tobytes()
        if split is not None:
            inside = [(r["pos"] >= p0) & (r["pos"] < p0 + span) for r in recs]
            assert all(m.any() and not m.all() for m in inside)    # every stream has records inside and outside the range
        p = dense(len(idx), indiv, sp)
        for k, i in enumerate(idx):
            pos1 = int(pos[i]) + 1
            if typ[k] < 0:
                continue
            rows[pos1] = fx.base_row("chr1", pos1, chr(f["ref"][i]), call[k], p[k])
            if typ[k] > 0:
                srows[pos1] = fx.snp_row("chr1", pos1, chr(f["ref"][i]), call[k], p[k], typ[k], ac[k], den[k])
    # the text the unmodified reference printed, for every position that has a row
    assert set(rows) == set(f["base_rows"]) and set(srows) == set(f["snp_rows"])
    bad = [k for k in rows if rows[k] != f["base_rows"][k]] + [k for k in srows if srows[k] != f["snp_rows"][k]]
    assert not bad, (len(bad), bad[:3])
    dev.close()
    host.close()
