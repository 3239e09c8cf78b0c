"""Several device objects in ONE process (what pemapper_hip does under PEMAP_DEVICES): pemap_dev_index_share hands a built index to
a second object, pemap_dev_absorb sums two objects' pileups on the device.  Two objects on the one GPU of the box, look-up replicas
off so that the indexes fit side by side.  The staged way of the counter sum (the one two physical GPUs take) is forced with
PEMAP_ABSORB_STAGED=1, in pieces of 5000 KiB: several pieces and a ragged last one over the 23 MB of counters."""
import os
import subprocess
import sys
import numpy as np
import pytest
import fixtures
import multi_object_common as moc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
STAGED = [pytest.param(None, id="direct"), pytest.param("1", id="staged")]


def _env(monkeypatch, staged):
    """the knobs are read once, when an object is created"""
    monkeypatch.setenv("PEMAP_REPLICAS", "0")
    monkeypatch.delenv("PEMAP_ABSORB_STAGED", raising=False)
    monkeypatch.delenv("PEMAP_ABSORB_CHUNK", raising=False)
    if staged:
        monkeypatch.setenv("PEMAP_ABSORB_STAGED", staged)
        monkeypatch.setenv("PEMAP_ABSORB_CHUNK", "5000")


@pytest.fixture(scope="module")
def built():
    """the object that builds the golden index, once for the module; the tests' own objects receive it by index_share"""
    from pecaller_amd import PemapDev
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PEMAP_REPLICAS", "0")
        d = PemapDev(0)
    ix = fixtures.index()
    d.build_index(ix["genome"], ix["contig_len"])
    assert d.lookup_replicas()[0] == 0
    yield d
    d.close()


def _pair(built):
    from pecaller_amd import PemapDev
    A, B = PemapDev(0), PemapDev(0)
    A.index_share(built)
    B.index_share(built)
    return A, B


def test_index_share_copies_the_index(built, monkeypatch):
    from pecaller_amd import PemapDev
    _env(monkeypatch, None)
    A, B = built, PemapDev(0)
    try:
        B.index_share(A)
        assert B.index_info() == A.index_info()
        assert B.lookup_replicas()[0] == 0
        for which, dt in ((1, np.uint32), (2, np.uint8), (3, np.uint32)):
            assert np.array_equal(B.read_buffer(which, dt), A.read_buffer(which, dt)), which
        nb = A.buffer(0)[1]
        assert nb == ((1 << 32) + 1) * 4 and B.buffer(0)[1] == nb
        big, small = 64 << 20, 16 << 20
        windows = [(0, big), (nb - big, big)] + [((nb // 4 * q) & ~3, small) for q in (1, 2, 3)]
        for off, n in windows:
            assert np.array_equal(B.read_buffer(0, np.uint32, offset_bytes=off, n_bytes=n), A.read_buffer(0, np.uint32, offset_bytes=off, n_bytes=n)), off
        assert B.read_buffer(0, np.uint32, offset_bytes=nb - 4, n_bytes=4)[0] == A.index_info()[0]
        n = len(fixtures.reads("r150")[1])
        m1, m2, _ = moc.map_range(B, 0, n)
        assert np.array_equal(m1, fixtures.golden_m("r150", 1)) and np.array_equal(m2, fixtures.golden_m("r150", 2))
    finally:
        B.close()


@pytest.mark.parametrize("staged", STAGED)
def test_absorb_sums_two_objects(built, monkeypatch, staged):
    _env(monkeypatch, staged)
    A, B = _pair(built)
    try:
        ma, mb = moc.map_halves(A, B)
        moc.absorb_checked(A, B)
        moc.check_sum_is_the_whole_read_set(A)
        moc.check_emptied(B)
        # B starts over: the same words as before, and its pileup is that batch's alone
        again = moc.map_range(B, moc.CUT, len(fixtures.reads("r150")[1]))
        assert np.array_equal(again[0], mb[0]) and np.array_equal(again[1], mb[1]) and np.array_equal(again[2], mb[2])
        assert B.summary()[4:13].sum() == len(mb[0])
    finally:
        A.close()
        B.close()


WRAP_CHILD = r'''
import sys, numpy as np, torch
torch.cuda.set_device(0)
import fixtures
import multi_object_common as moc
from pecaller_amd import PemapDev, dist as pd
ix = fixtures.index()
A, B = PemapDev(0), PemapDev(0)
A.build_index(ix["genome"], ix["contig_len"])
B.index_share(A)
HI = (40000 << 16) - (1 << 32)          # the bit pattern of 40000 << 16 as an int32
for d in (A, B):
    cnt = pd.device_tensor(torch, d, 4)
    cnt[:600] += 40000
    cnt[600:1200] += HI
torch.cuda.synchronize()
moc.map_halves(A, B)
a, b = moc.absorb_checked(A, B)
# the bumped counters did pass 65,535 in both halves, and their neighbours in the same words are ordinary sums
w = np.arange(1200)
bumped = np.where(w < 600, 2 * w, 2 * w + 1)
assert ((a[bumped].astype(np.int64) + b[bumped]) > 65535).all()
counts, ins = A.fetch_pileup()
# take the two objects' 40,000 out again, modulo 2^16: plane 0 holds the reference base's own column (PmPile's rotation); the low
# halves of words 0..599 are positions 0, 2, .. 1198, the high halves of words 600..1199 positions 1201, 1203, .. 2399
rows = np.concatenate([np.arange(0, 1200, 2), np.arange(1201, 2400, 2)])
col = fixtures.plane0_column(rows)
counts[rows, col] = (counts[rows, col].astype(np.uint32) - 2 * 40000).astype(np.uint16)
moc.check_sum_is_the_whole_read_set(A, counts, ins)
moc.check_emptied(B)
A.close()
B.close()
print("wrap ok")
'''


@pytest.mark.parametrize("staged", STAGED)
def test_absorb_wraps_like_one_u16_counter(monkeypatch, staged):
    """two objects' counters that together pass 65,535 -- 40,000 preset in each, in low halves of some words and high halves of
    others, through torch views of buffer 4 -- sum like ONE unsigned short counter (pemapper.c:53-58), without a carry into the
    counter that shares the word.  In a process of its own, torch initialised first as bench.py does."""
    _env(monkeypatch, staged)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE]))
    r = subprocess.run([sys.executable, "-c", WRAP_CHILD], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and b"wrap ok" in r.stdout, r.stdout[-3000:].decode(errors="replace")


def test_refusals_leave_the_objects_usable(built, monkeypatch):
    from pecaller_amd import PemapDev, PemapError
    _env(monkeypatch, None)
    A, B = _pair(built)
    bare, small = PemapDev(0), PemapDev(0)
    try:
        def refused(call, *args):
            with pytest.raises(PemapError) as e:
                call(*args)
            assert str(e.value).strip()
        refused(A.absorb, A)
        refused(A.index_share, A)
        refused(B.index_share, bare)            # the source has no index
        refused(A.absorb, bare)
        refused(bare.absorb, A)
        # a second genome: the first 1 Mbp of the golden one
        ix = fixtures.index()
        lens, left = [], 1000000
        for c in ix["contig_len"]:
            lens.append(min(int(c), left))
            left -= lens[-1]
            if left == 0:
                break
        assert sum(lens) == 1000000 and lens[-1] >= 16
        small.build_index(ix["genome"][:1000000], np.array(lens, np.uint32))
        refused(A.absorb, small)
        refused(small.absorb, A)
        # a batch that was submitted and not waited for, in the destination and in the source
        r1, l1, r2, l2 = fixtures.reads("r150")
        A.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
        t = A.submit_batch(r1[:4000], l1[:4000], r2[:4000], l2[:4000])
        refused(A.absorb, B)
        refused(B.absorb, A)
        m1, m2, _ = A.wait_batch(t)
        assert np.array_equal(m1, fixtures.golden_m("r150", 1)[:4000]) and np.array_equal(m2, fixtures.golden_m("r150", 2)[:4000])
        # nothing was changed by the refused calls: B is still empty, and both map the golden words
        moc.check_emptied(B)
        A.reset_pileup()
        moc.map_halves(A, B)
        moc.absorb_checked(A, B)
        moc.check_sum_is_the_whole_read_set(A)
    finally:
        for d in (A, B, bare, small):
            d.close()
