"""pecall_dev_sites_base_gz: the rows of <outfile>.base.gz as gzip members deflated on the device.  The device is held to the serial
statement of the rule, not to itself: the expected bytes are what tests/csrc/gz_rule_check.c (pcg_encode_piece of
pecaller_amd/csrc/pecall_gz_rule.h) makes of pecall_dev_sites_base_text's text -- which test_gpu_pecall_rows.py checks -- cut at hole_at."""
import gzip
import numpy as np
import pytest
import gz_cases as gc
import pecall_sites_fixture as fx
from test_gpu_pecall_rows import NAMES, EDGES, synthetic, records_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from pecaller_amd.pecall import PecallDev
    d = PecallDev(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return gc.build_check(tmp_path_factory.mktemp("gz_rule"))


def boundaries(gz):
    """member boundary in gz -> bytes the members in front of it inflate to"""
    at, text, out = 0, 0, {0: 0}
    for member, inflated in gc.members(gz):
        at += len(member)
        text += len(inflated)
        out[at] = text
    return out


def check_resident(dev, exe, tmp_path, names, contig, pos, ref):
    """base_gz against the serial rule over base_text's text, for the results that lie on the device -> text, holes, gz, places"""
    text, hole_site, hole_at = dev.base_text(names, contig, pos, ref)
    gz, gz_site, gz_at = dev.base_gz(names, contig, pos, ref)
    assert dev.text_needed == len(text) and dev.gz_needed == len(gz) and dev.holes_needed == len(hole_site)
    want = gc.encode(exe, tmp_path, text, hole_at)
    assert len(gz) == len(want)
    assert gz == want
    assert np.array_equal(gz_site, hole_site)
    edge = boundaries(gz)
    assert max(edge) == len(gz)
    for k in range(len(gz_at)):
        assert int(gz_at[k]) in edge, k
        assert edge[int(gz_at[k])] == int(hole_at[k]), k
    assert (gzip.decompress(gz) if gz else b"") == text
    gz2, gz_site2, gz_at2 = dev.base_gz(names, contig, pos, ref)
    assert gz2 == gz and np.array_equal(gz_site2, gz_site) and np.array_equal(gz_at2, gz_at)
    return text, hole_site, hole_at, gz, gz_at


def check_case(dev, exe, tmp_path, reads, dom, names, contig, pos, ref):
    call, post, typ, _, _ = dev.call_sites(reads, dom)
    return (call.copy(), post.copy(), typ.copy()) + check_resident(dev, exe, tmp_path, names, contig, pos, ref)


@pytest.mark.parametrize("tag", ["pecall_sites", "pecall_wide"])
def test_base_gz_of_the_reference_fixtures(dev, exe, tmp_path, tag):
    """the two fixtures of the reference's text (8 and 100 samples): with the holes' rows put in as members of the host's making at
    hole_gz_at, the inflated whole reproduces every row of the fixture"""
    f = fx.load(tag)
    n = len(f["pos"])
    contig = np.zeros(n, np.int32)
    pos1 = (f["pos"] + 1).astype(np.uint32)
    call, post, typ, text, hole_site, hole_at, gz, gz_at = check_case(dev, exe, tmp_path, f["reads"], f["dom"], ["chr1"], contig, pos1, f["ref"])
    assert f["reads"].shape[1] == (8 if tag == "pecall_sites" else 100) and len(hole_site) > 20
    out, prev = bytearray(), 0
    for s, a in zip(hole_site, gz_at):
        out += gz[prev:int(a)]
        prev = int(a)
        out += gzip.compress(b"\n" + fx.base_row("chr1", int(pos1[s]), chr(f["ref"][s]), call[s], post[s]).encode(), 1)
    out += gz[prev:]
    rows = {int(r.split("\t")[1]): r for r in gzip.decompress(bytes(out)).decode().split("\n")[1:]}
    assert len(rows) == int((typ >= 0).sum())
    for p, exp in f["base_rows"].items():
        assert rows[p] == exp, p


@pytest.mark.parametrize("n_sites,n", [(300, 1), (300, 64), (300, 65), (300, 130), (40, 512)])
def test_base_gz_of_synthetic_columns(dev, exe, tmp_path, n_sites, n):
    """many holes, some next to each other (runs without a byte), positions on every digit boundary, two name lengths"""
    reads, dom, contig, pos, ref = synthetic(n_sites, n)
    assert set(EDGES[:min(len(EDGES), n_sites)]) <= set(int(p) for p in pos)
    _, _, _, text, hole_site, hole_at, gz, gz_at = check_case(dev, exe, tmp_path, reads, dom, NAMES, contig, pos, ref)
    assert len(hole_site) >= 1 and (hole_at[1:] == hole_at[:-1]).any() and (gz_at[1:] == gz_at[:-1]).any()


def test_base_gz_of_a_run_of_three_pieces(dev, exe, tmp_path):
    """no hole: one run of 2 * PCG_PIECE + 1 bytes, so two whole pieces and one of a single byte"""
    reads, dom, names, contig, pos, ref = gc.low_hole_columns()
    _, _, _, text, hole_site, _, gz, _ = check_case(dev, exe, tmp_path, reads, dom, names, contig, pos, ref)
    assert len(hole_site) == 0 and len(text) == 2 * gc.PCG_PIECE + 1
    assert [len(t) for _, t in gc.members(gz)] == [gc.PCG_PIECE, gc.PCG_PIECE, 1]
    assert len(gz) * 4 < len(text)


def test_base_gz_without_text(dev, exe, tmp_path):
    reads, dom, contig, pos, ref = synthetic(300, 20)
    # every column skipped
    dev.call_sites(reads, np.full(300, 14, np.uint8))
    gz, site, at = dev.base_gz(NAMES, contig, pos, ref)
    assert gz == b"" and dev.gz_needed == 0 and dev.text_needed == 0 and len(site) == 0 and len(at) == 0
    # every column a hole: the hole columns of the synthetic set alone (a column is called on its own)
    dev.call_sites(reads, dom)
    _, holes, _ = dev.base_text(NAMES, contig, pos, ref)
    n_sites = len(holes)
    assert n_sites > 20
    _, post, typ, _, _ = dev.call_sites(reads[holes], dom[holes])
    assert (typ >= 0).all() and (post != 1.0).any(axis=1).all()
    gz, site, at = dev.base_gz(NAMES, contig[:n_sites], pos[:n_sites], ref[:n_sites])
    assert gz == b"" and dev.gz_needed == 0 and dev.text_needed == 0
    assert np.array_equal(site, np.arange(n_sites)) and (at == 0).all()


def test_base_gz_after_a_resident_run_and_after_call_records(dev, exe, tmp_path):
    reads, dom, contig, pos, ref = synthetic(300, 20)
    call, _, typ, _, _, _, gz, gz_at = check_case(dev, exe, tmp_path, reads, dom, NAMES, contig, pos, ref)
    dev.sites_stage(reads, dom)
    with pytest.raises(Exception, match="no call's results"):
        dev.base_gz(NAMES, contig, pos, ref)
    dev.sites_run()
    got = dev.base_gz(NAMES, contig, pos, ref)
    assert got[0] == gz and np.array_equal(got[2], gz_at)
    rcall, _, rtyp, _, _, col_slot = dev.call_records(records_of(reads, 100), 100, 300, bytes(ref))
    assert np.array_equal(col_slot, np.arange(300)) and np.array_equal(rcall, call) and np.array_equal(rtyp, typ)
    got = dev.base_gz(NAMES, contig, pos, ref)
    assert got[0] == gz and np.array_equal(got[2], gz_at)


def test_base_gz_capacities_buffers_and_errors(dev, exe, tmp_path):
    from pecaller_amd.pecall import PecallDev
    reads, dom, contig, pos, ref = synthetic(300, 20)
    _, _, _, text, hole_site, _, gz, gz_at = check_case(dev, exe, tmp_path, reads, dom, NAMES, contig, pos, ref)
    pinned = dev.base_gz(NAMES, contig, pos, ref, pin=True)
    assert pinned[0] == gz and np.array_equal(pinned[1], hole_site) and np.array_equal(pinned[2], gz_at)
    with pytest.raises(Exception, match="n_gz and n_holes say what is needed"):
        dev.base_gz(NAMES, contig, pos, ref, gz_cap=len(gz) - 1)
    assert dev.gz_needed == len(gz) and dev.holes_needed == len(hole_site) and dev.text_needed == len(text)
    with pytest.raises(Exception, match="n_gz and n_holes say what is needed"):
        dev.base_gz(NAMES, contig, pos, ref, hole_cap=len(hole_site) - 1)
    assert dev.gz_needed == len(gz) and dev.holes_needed == len(hole_site)
    for pin in (False, True):
        exact = dev.base_gz(NAMES, contig, pos, ref, gz_cap=len(gz), hole_cap=len(hole_site), pin=pin)
        assert exact[0] == gz and np.array_equal(exact[1], hole_site) and np.array_equal(exact[2], gz_at)
    bad = contig.copy()
    bad[150] = len(NAMES)
    with pytest.raises(Exception, match=r"sites_base_gz: contig\[150\] = 2"):
        dev.base_gz(NAMES, bad, pos, ref)
    far = pos.copy()
    far[7] = 2 ** 31
    with pytest.raises(Exception, match=r"pos\[7\] = 2147483648"):
        dev.base_gz(NAMES, contig, far, ref)
    assert dev.base_gz(NAMES, contig, pos, ref)[0] == gz
    fresh = PecallDev(0)
    with pytest.raises(Exception, match="no call's results"):
        fresh.base_gz(NAMES, contig, pos, ref)
    fresh.close()
