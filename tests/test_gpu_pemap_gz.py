"""pemap_dev_fetch_records_gz on the g1 golden index with the 20,000 golden 2 x 150 pairs: the BGZF members the device makes of a
range's records are, byte for byte, what the serial statement of the rule (tests/csrc/pemap_gz_rule_check.c, pemap_gz_rule.h) writes
for the records pemap_dev_fetch_records returns for the same range, and the insertion list is the records with c[5] > 0."""
import ctypes as C
import numpy as np
import pytest
import fixtures
import pileup_gz_cases as pc

pytestmark = pytest.mark.gpu
R = pc.PIECE_RECORDS


@pytest.fixture(scope="module")
def dev():
    from pecaller_amd import PemapDev
    d = PemapDev(0)
    ix = fixtures.index()
    d.build_index(ix["genome"], ix["contig_len"])
    d.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
    yield d
    d.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pc.build_check(tmp_path_factory.mktemp("pemap_gz_rule_gpu"))


def map_passes(dev, passes):
    """the pileup of the golden batch mapped `passes` times, from zero"""
    r1, l1, r2, l2 = fixtures.reads("r150")
    dev.reset_pileup()
    dev.stage_reads(r1, l1, r2, l2)
    for _ in range(passes):
        dev.run(sync=False)
    dev.sync()


def same_as_the_rule(dev, exe, tmp_path, first, count, tag):
    """fetch_records_gz first (the fold is its own job), then fetch_records and the check program -> the records"""
    gz, n, ins = dev.fetch_records_gz(first, count)
    rec = dev.fetch_records(first, count)
    assert n == len(rec), tag
    want = pc.encode(exe, tmp_path, rec.tobytes(), tag=tag)[0] if len(rec) else b""
    assert len(gz) == len(want) and gz == want, (tag, len(gz), len(want))
    assert ins.tobytes() == rec[rec["c"][:, 5] > 0].tobytes(), tag
    return rec, gz


def ranges_for(rec, gsize):
    """(first, count) by the number of records a call returns, chosen from the host's copy of the records"""
    pos = rec["pos"].astype(np.int64)
    gap = np.flatnonzero(np.diff(pos) > 1)
    assert len(gap), "the golden reads leave no position uncovered"
    out = {0: (int(pos[gap[0]]) + 1, int(pos[gap[0] + 1] - pos[gap[0]] - 1))}
    for k, at in ((1, 7), (R - 1, 1000), (R, 5000), (R + 1, 70000), (2 * R + 1, 300000)):
        out[k] = (int(pos[at]), int(pos[at + k - 1] - pos[at] + 1))
    return out


def test_one_pass_ranges_by_record_count(dev, exe, tmp_path):
    map_passes(dev, 1)
    whole, gz = same_as_the_rule(dev, exe, tmp_path, 0, dev.gsize, "whole")
    assert len(whole) == fixtures.meta()["r150"]["pileup_records"]
    members = pc.walk(gz)
    assert len(members) == (len(whole) + R - 1) // R and b"".join(t for _, t in members) == whole.tobytes()
    assert len(gz) * 2 < whole.nbytes
    assert (whole["c"][:, 5] > 0).sum() > 10
    for k, (first, count) in ranges_for(whole, dev.gsize).items():
        rec, gz = same_as_the_rule(dev, exe, tmp_path, first, count, "n%d" % k)
        assert len(rec) == k and (len(gz) > 0) == (k > 0), k
    # a range that ends at the genome's last position, and one of no positions at all
    tail = int(whole["pos"][-700])
    rec, _ = same_as_the_rule(dev, exe, tmp_path, tail, dev.gsize - tail, "tail")
    assert len(rec) == 700
    assert dev.fetch_records_gz(5, 0)[:2] == (b"", 0)
    ms = dev.fetch_gz_ms()
    assert sorted(ms) == ["deflate", "insertions", "pack", "records"]


def test_hundred_passes_high_bytes(dev, exe, tmp_path):
    """the same batch mapped 100 times: counts pass 255, so the counters' high bytes vary"""
    map_passes(dev, 100)
    rec, gz = same_as_the_rule(dev, exe, tmp_path, 0, dev.gsize, "x100")
    assert rec["c"].max() > 255 and len(rec) == fixtures.meta()["r150"]["pileup_records"]
    assert len(pc.walk(gz)) == (len(rec) + R - 1) // R


def test_after_reset_there_is_nothing(dev):
    map_passes(dev, 1)
    dev.reset_pileup()
    gz, n, ins = dev.fetch_records_gz()
    assert gz == b"" and n == 0 and len(ins) == 0
    assert all(v == 0.0 for k, v in dev.fetch_gz_ms().items() if k != "records")


def test_capacities_and_ranges_are_checked(dev):
    from pecaller_amd import PemapError
    map_passes(dev, 1)
    L, h = dev.L, dev.h
    nb, nr, ni = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.pemap_dev_fetch_records_gz(h, 0, dev.gsize, None, 0, C.byref(nb), C.byref(nr), None, 0, C.byref(ni)) == 0
    assert nb.value > 0 and ni.value > 1 and nr.value == fixtures.meta()["r150"]["pileup_records"]
    gz = np.full(nb.value, 0xa5, np.uint8)
    ins = np.full(ni.value * 16, 0xa5, np.uint8)
    for gz_cap, ins_cap, need in ((nb.value - 1, ni.value, nb.value), (nb.value, ni.value - 1, ni.value)):
        rc = L.pemap_dev_fetch_records_gz(h, 0, dev.gsize, gz.ctypes.data, gz_cap, C.byref(nb), C.byref(nr), ins.ctypes.data, ins_cap, C.byref(ni))
        msg = L.pemap_dev_last_error(h).decode()
        assert rc != 0 and str(need) in msg and "do not fit" in msg, msg
        assert (gz == 0xa5).all() and (ins == 0xa5).all()
    # ins_records may be NULL: the count still comes back
    ni.value = 0
    assert L.pemap_dev_fetch_records_gz(h, 0, dev.gsize, gz.ctypes.data, gz.nbytes, C.byref(nb), C.byref(nr), None, 0, C.byref(ni)) == 0
    assert ni.value * 16 == len(ins) and not (gz[:4] == 0xa5).any()
    with pytest.raises(PemapError, match="beyond the genome"):
        dev.fetch_records_gz(dev.gsize - 10, 11)
    with pytest.raises(PemapError, match="beyond the genome"):
        dev.fetch_records_gz(dev.gsize + 1, 0)


def test_pinned_destination(dev, exe, tmp_path):
    """the members come back straight into a buffer the caller pinned: the same bytes"""
    map_passes(dev, 1)
    want, n, _ = dev.fetch_records_gz()
    buf = np.zeros(len(want) + 4096, np.uint8)
    dev.pin_host(buf)
    try:
        nb, nr, ni = C.c_uint64(), C.c_uint64(), C.c_uint64()
        dev._ck(dev.L.pemap_dev_fetch_records_gz(dev.h, 0, dev.gsize, buf.ctypes.data, buf.nbytes, C.byref(nb), C.byref(nr), None, 0, C.byref(ni)))
    finally:
        dev.unpin_host(buf)
    assert nb.value == len(want) and buf[:nb.value].tobytes() == want and not buf[nb.value:].any()


def test_plane_0_is_folded_by_the_entry(dev, exe, tmp_path):
    """directly behind submit_batch / wait_batch plane 0 still holds differences: the entry folds it itself"""
    r1, l1, r2, l2 = fixtures.reads("r150")
    dev.reset_pileup()
    dev.wait_batch(dev.submit_batch(r1, l1, r2, l2))
    rec, _ = same_as_the_rule(dev, exe, tmp_path, 0, dev.gsize, "submit")
    assert len(rec) == fixtures.meta()["r150"]["pileup_records"]
