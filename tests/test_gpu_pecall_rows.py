"""pecall_dev_sites_base_text: the rows of <outfile>.base.gz made on the device from the resident results of a call.  The expected
text is put together here from the dense call's results with pecall_sites_fixture.base_row (those results are checked against the
oracle and the reference's text in test_pecall_sites.py): the rows of the columns that are neither skipped nor holes; the holes
are the columns pecall_dev_call_sites_sparse lists, each at the length of the expected text in front of it."""
import functools
import numpy as np
import pytest
import pecall_sites_fixture as fx

pytestmark = pytest.mark.gpu
NAMES = ["c", "chr12_KI270904v1_altern"]          # 1 and 23 bytes
# every digit boundary of a position up to the last one
EDGES = [0] + [v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)] + [2147483646, 2147483647]


def expected(names, contig, pos, ref, call, post, typ):
    """-> text, hole columns, hole offsets"""
    text, holes, at = bytearray(), [], []
    for s in range(len(typ)):
        if typ[s] < 0:
            continue
        if (post[s] != 1.0).any():
            holes.append(s)
            at.append(len(text))
            continue
        text += b"\n" + fx.base_row(names[contig[s]], int(pos[s]), chr(ref[s]), call[s], post[s]).encode()
    return bytes(text), np.array(holes, np.uint32), np.array(at, np.uint64)


def splice(text, names, contig, pos, ref, call, post, hole_site, hole_at):
    """the holes' rows, formatted here, put into the device's text -> the rows"""
    out, prev = bytearray(), 0
    for s, a in zip(hole_site, hole_at):
        out += text[prev:int(a)]
        prev = int(a)
        out += b"\n" + fx.base_row(names[contig[s]], int(pos[s]), chr(ref[s]), call[s], post[s]).encode()
    out += text[prev:]
    return bytes(out).decode().split("\n")[1:]


@functools.lru_cache(maxsize=None)
def synthetic(n_sites, n, seed=0):
    """columns of n samples, ~30 % of them variant with shallow samples among the carriers (posteriors below 1: holes, often
    next to each other), reference byte 14 at both ends and elsewhere (skipped), names of 1 and 23 bytes in blocks of 7 columns,
    positions on every digit boundary"""
    rng = np.random.default_rng(1000 * n + n_sites + seed)
    dom = rng.integers(0, 4, n_sites).astype(np.uint8)
    dom[0] = dom[-1] = 14
    dom[11::23] = 14
    depth = rng.integers(20, 40, n)
    depth[1:16:4] = 5                                  # (a few shallow samples: every one of them keeps a column from the shortcut)
    depth[0] = 6
    is_var = np.repeat(rng.random((n_sites + 2) // 3) < 0.3, 3)[:n_sites]       # (in runs of three columns)
    q = rng.uniform(0.05, 0.5, n_sites) * min(1.0, 32.0 / n)      # (a few dozen carriers at most: a column's beam search grows with them)
    alt = (np.where(dom < 4, dom, 0) + rng.integers(1, 4, n_sites)) % 4
    reads = np.zeros((n_sites, n, 6), np.int64)
    idx = np.arange(n_sites)
    r = np.where(dom < 4, dom, 0)
    for i in range(n):
        d = rng.poisson(depth[i], n_sites) + 1
        dose = np.where(is_var, rng.binomial(2, q), 0)
        e = rng.binomial(d, 0.004)
        ar = rng.binomial(d - e, dose / 2.0)
        reads[idx, i, r] += d - e - ar
        reads[idx, i, alt] += ar
        reads[idx, i, rng.integers(0, 4, n_sites)] += e
    contig = ((idx // 7) % 2).astype(np.int32)
    pos = rng.integers(0, 2 ** 31, n_sites).astype(np.uint32)
    k = min(len(EDGES), n_sites)
    pos[rng.permutation(n_sites)[:k]] = EDGES[:k]
    ref = np.frombuffer(b"ACGTNNNNNNNNNNN", np.uint8)[dom]
    for a in (reads, dom, contig, pos):
        a.setflags(write=False)
    return reads.astype(np.uint16), dom, contig, pos, ref


@pytest.fixture(scope="module")
def dev():
    from pecaller_amd.pecall import PecallDev
    d = PecallDev(0)
    yield d
    d.close()


def check_case(dev, reads, dom, names, contig, pos, ref, want_holes=True):
    call, post, typ, _, _ = dev.call_sites(reads, dom)
    call, post, typ = call.copy(), post.copy(), typ.copy()
    text, hole_site, hole_at = dev.base_text(names, contig, pos, ref)
    exp_text, exp_holes, exp_at = expected(names, contig, pos, ref, call, post, typ)
    assert np.array_equal(hole_site, exp_holes), (len(hole_site), len(exp_holes))
    assert np.array_equal(hole_at, exp_at)
    assert len(text) == len(exp_text)
    assert text == exp_text
    # the holes are the columns the sparse call lists for the same columns -- and the text after that call is the same
    _, (site, _), _, _, _ = dev.call_sites_sparse(reads, dom)
    assert np.array_equal(site, exp_holes)
    text2, hole_site2, hole_at2 = dev.base_text(names, contig, pos, ref)
    assert text2 == exp_text and np.array_equal(hole_site2, exp_holes) and np.array_equal(hole_at2, exp_at)
    if want_holes:
        assert len(exp_holes) >= 1 and (np.diff(exp_holes.astype(np.int64)) == 1).any(), "no hole, or no two holes next to each other"
        assert (exp_at[1:] == exp_at[:-1]).any()
    return call, post, typ, text, hole_site, hole_at


@pytest.mark.parametrize("tag", ["pecall_sites", "pecall_wide"])
def test_base_text_of_the_reference_fixtures(dev, tag):
    """the two fixtures of the reference's text (8 and 100 samples): every row the device made equals the row the reference printed
    for the column, and with the holes' rows (base_row of the dense call's posteriors) put in at hole_at every row of the fixture
    is reproduced"""
    f = fx.load(tag)
    n = len(f["pos"])
    contig = np.zeros(n, np.int32)
    pos1 = (f["pos"] + 1).astype(np.uint32)
    call, post, typ, text, hole_site, hole_at = check_case(dev, f["reads"], f["dom"], ["chr1"], contig, pos1, f["ref"], want_holes=False)
    assert f["reads"].shape[1] == (8 if tag == "pecall_sites" else 100)
    holes = set(int(s) for s in hole_site)
    dev_rows = {int(r.split("\t")[1]): r for r in text.decode().split("\n")[1:]}
    n_dev = 0
    for i in range(n):
        exp = f["base_rows"].get(int(pos1[i]))
        if exp is not None and i not in holes:
            assert dev_rows[int(pos1[i])] == exp, int(pos1[i])
            n_dev += 1
    assert n_dev > 1000 and len(holes) > 20
    rows = {int(r.split("\t")[1]): r for r in splice(text, ["chr1"], contig, pos1, f["ref"], call, post, hole_site, hole_at)}
    assert len(rows) == int((typ >= 0).sum())
    for p, exp in f["base_rows"].items():
        assert rows[p] == exp, p


@pytest.mark.parametrize("n_sites,n", [(300, 1), (300, 3), (300, 63), (300, 64), (300, 65), (300, 130), (5000, 3), (40, 512)])
def test_base_text_of_synthetic_columns(dev, n_sites, n):
    """sample counts around the wave's width and beyond two chunks of 64; 5,000 columns: five blocks of the scan; 512 samples: 15
    columns per workgroup of the fill kernel (64 in the other cases) -- no column count is a multiple of it"""
    reads, dom, contig, pos, ref = synthetic(n_sites, n)
    assert set(EDGES[:min(len(EDGES), n_sites)]) <= set(int(p) for p in pos)
    assert dom[0] == 14 and dom[-1] == 14 and (dom[1:-1] == 14).any()
    _, _, typ, text, _, _ = check_case(dev, reads, dom, NAMES, contig, pos, ref)
    assert typ[0] < 0 and typ[-1] < 0
    rows = text.decode().split("\n")[1:]
    assert len(set(r.split("\t")[0] for r in rows)) == 2
    assert all(len(r.split("\t")) == 3 + 2 * n for r in rows)


def records_of(reads, p0):
    from pecaller_amd.pecall import RECORD
    out = []
    for s in range(reads.shape[1]):
        cols = np.nonzero(reads[:, s].sum(axis=1) > 0)[0]
        r = np.zeros(len(cols), RECORD)
        r["pos"] = p0 + cols
        r["counts"] = reads[cols, s]
        out.append(r)
    return out


def test_base_text_after_a_resident_run_and_after_call_records(dev):
    reads, dom, contig, pos, ref = synthetic(300, 20)
    call, post, typ, text, hole_site, hole_at = check_case(dev, reads, dom, NAMES, contig, pos, ref)
    dev.sites_stage(reads, dom)
    with pytest.raises(Exception, match="no call's results"):
        dev.base_text(NAMES, contig, pos, ref)           # staged, not called: what lies on the device is not this stage's
    dev.sites_run()
    got = dev.base_text(NAMES, contig, pos, ref)
    assert got[0] == text and np.array_equal(got[1], hole_site) and np.array_equal(got[2], hole_at)
    # the same columns from record streams: every column has a record (sample 0 is never empty), the letters give the reference bytes
    assert (reads[:, 0].sum(axis=1) > 0).all()
    rcall, _, rtyp, _, _, col_slot = dev.call_records(records_of(reads, 100), 100, 300, bytes(ref))
    assert np.array_equal(col_slot, np.arange(300)) and np.array_equal(rcall, call) and np.array_equal(rtyp, typ)
    got = dev.base_text(NAMES, contig, pos, ref)
    assert got[0] == text and np.array_equal(got[1], hole_site) and np.array_equal(got[2], hole_at)


def test_base_text_special_cases_and_errors(dev):
    from pecaller_amd.pecall import PecallDev
    reads, dom, contig, pos, ref = synthetic(300, 20)
    # every column skipped
    none = np.full(300, 14, np.uint8)
    dev.call_sites(reads, none)
    text, hole_site, hole_at = dev.base_text(NAMES, contig, pos, ref)
    assert text == b"" and dev.text_needed == 0 and len(hole_site) == 0 and len(hole_at) == 0
    _, _, _, text, hole_site, hole_at = check_case(dev, reads, dom, NAMES, contig, pos, ref)
    dev.call_sites(reads, dom)
    # pinned and pageable targets
    pinned = dev.base_text(NAMES, contig, pos, ref, pin=True)
    assert pinned[0] == text and np.array_equal(pinned[1], hole_site) and np.array_equal(pinned[2], hole_at)
    # too little room: the call fails and says what is needed
    with pytest.raises(Exception, match="n_text and n_holes say what is needed"):
        dev.base_text(NAMES, contig, pos, ref, text_cap=len(text) - 1)
    assert dev.text_needed == len(text) and dev.holes_needed == len(hole_site)
    with pytest.raises(Exception, match="n_text and n_holes say what is needed"):
        dev.base_text(NAMES, contig, pos, ref, hole_cap=len(hole_site) - 1)
    assert dev.text_needed == len(text) and dev.holes_needed == len(hole_site)
    exact = dev.base_text(NAMES, contig, pos, ref, text_cap=len(text), hole_cap=len(hole_site))
    assert exact[0] == text and np.array_equal(exact[1], hole_site)
    # what must not become an address
    bad = contig.copy()
    bad[150] = len(NAMES)
    with pytest.raises(Exception, match=r"contig\[150\] = 2"):
        dev.base_text(NAMES, bad, pos, ref)
    bad[150] = -1
    with pytest.raises(Exception, match=r"contig\[150\] = -1"):
        dev.base_text(NAMES, bad, pos, ref)
    far = pos.copy()
    far[7] = 2 ** 31
    with pytest.raises(Exception, match=r"pos\[7\] = 2147483648"):
        dev.base_text(NAMES, contig, far, ref)
    # and the object still works
    again = dev.base_text(NAMES, contig, pos, ref)
    assert again[0] == text
    fresh = PecallDev(0)
    with pytest.raises(Exception, match="no call's results"):
        fresh.base_text(NAMES, contig, pos, ref)
    fresh.close()
