"""Plane 0 of the pileup kept as differences while the object maps (PmPile, pemap_pile_diff.h): pm_pile_kernel adds +1 where a
run of matched bases starts and -1 behind it, the host layer unfolds the plane before the first pile kernel of a run and folds it
back for every entry that reads the counters.  Against the oracle, exactly (counts and insertions), on a genome of a dozen random
contigs of about 3 kb with a stretch of odd reference letters, in batches of a few hundred pairs of 64 and 150 bases.

  run boundaries   reads placed so that run starts and ends fall on both position parities with both length parities
  form changes     fetch / reset / a kept view / asynchronous slices / absorb between and around batches
  conversions      preset planes through unfold and fold with nothing mapped: bit-equal, at the scan tile's edges
  wrap             plane-0 counters preset to 0xFFFE / 0xFFFF under the reads
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py
import refio

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[:] = ord("N")
for _a, _b in zip(b"ACGT", b"TGCA"):
    COMP[_a] = _b
PARAMS = dict(min_dist=0, max_dist=500, min_align=0.85)
ODD_CONTIG, ODD_AT, ODD_LETTERS = 3, 700, b"NaRncYgtKN"        # one odd letter every 37 bases from ODD_AT on
SCAN_TILE_WORDS = 1024          # PD_TILE, pemap_aux.hip.h


@functools.lru_cache(maxsize=None)
def _contigs():
    rng = np.random.default_rng(909)
    cs = [ACGT[rng.integers(0, 4, 2600 + 97 * k)].copy() for k in range(12)]
    for k, ch in enumerate(ODD_LETTERS):
        cs[ODD_CONTIG][ODD_AT + 37 * k] = ch
    return cs


@functools.lru_cache(maxsize=None)
def _index(bis):
    contigs = _contigs()
    mers, ukmer, ustart, cs = refio.kmer_index(contigs, bisulfite=bis)
    return dict(mers=mers, ukmer=ukmer, ustart=ustart, genome=np.concatenate(contigs), contig_starts=cs,
                contig_len=np.array([len(c) for c in contigs], dtype=np.uint32))


def _upper_plain(x):
    """a read's letters over reference letters: upper case, and a base where the reference has none"""
    y = x.copy()
    low = (y >= ord("a")) & (y <= ord("z"))
    y[low] -= 32
    y[~np.isin(y, ACGT)] = ord("G")
    return y


def _other(ch, rng):
    return ACGT[ACGT != ch][int(rng.integers(0, 3))]


def _pairs(L, bis, seed):
    """(mate 1 on the forward strand from s, mate 2 reverse-complemented ending at s + fl) x the edits listed in the module's text"""
    rng = np.random.default_rng(seed)
    cs = _contigs()
    out = []

    def pair(ci, s, fl, L1=L, L2=L, edit1=None, edit2=None):
        c = cs[ci]
        a = _upper_plain(c[s:s + L1])
        b = _upper_plain(c[s + fl - L2:s + fl])
        if edit1 is not None:
            a = edit1(a, c, s)
        if edit2 is not None:
            b = edit2(b, c, s + fl - L2)
        b = COMP[b][::-1].copy()
        if bis:
            for x in (a, b):
                conv = (x == ord("C")) & (rng.random(len(x)) < 0.95)
                x[conv] = ord("T")
        if rng.random() < 0.5:      # both strands for either mate
            a, b = b, a
        out.append((a.tobytes(), b.tobytes()))

    def subs(*offs):
        def f(x, c, lo):
            for o in offs:
                x[o % len(x)] = _other(x[o % len(x)], rng)
            return x
        return f

    def put(ch, *offs):
        def f(x, c, lo):
            for o in offs:
                x[o] = ch
            return x
        return f

    def dele(p, g):
        def f(x, c, lo):
            return _upper_plain(np.concatenate([c[lo:lo + p], c[lo + p + g:lo + len(x) + g]]))
        return f

    def inse(p, g):
        def f(x, c, lo):
            return np.concatenate([x[:p], ACGT[rng.integers(0, 4, g)], x[p:]])[:len(x)].copy()
        return f

    n_c = len(cs)
    # the genome's first base, its last base, every contig's ends
    for ci in range(n_c):
        pair(ci, 0, L + 60)
        pair(ci, len(cs[ci]) - L - 61, L + 61)
    # both position parities x both length parities, mates apart and mates that overlap
    for s in range(200, 204):
        for L1, L2 in ((L, L), (L - 1, L), (L, L - 1), (L - 1, L - 1)):
            pair(1, s, L + 90, L1, L2)
            pair(2, s, L + 11, L1, L2)
    # substitutions: first base, last base, two adjacent, either side of a word boundary, on both parities of the read's start
    for s in (300, 301):
        for e in (subs(0), subs(-1), subs(30, 31), subs(31, 32), subs(0, 1), subs(-2, -1), subs(20, 41), put(ord("N"), 33),
                  put(ord("N"), 0), put(ord("N"), -1)):
            pair(4, s, L + 70, edit1=e)
            pair(5, s, L + 71, edit2=e)
    # reads over the odd reference letters: a base where the letter is, then 'A' there (plane 0 without agreement), then 'N'
    for k in range(0, len(ODD_LETTERS), 2):
        at = ODD_AT + 37 * k
        for s in (at - 20, at - 21, at - L + 5):
            pair(ODD_CONTIG, s, L + 80)
            pair(ODD_CONTIG, s, L + 80, edit1=put(ord("A"), at - s))
            pair(ODD_CONTIG, s, L + 81, edit1=put(ord("N"), at - s))
    # the walked alignments: deletions of 1 and 10 bases and an insertion, in the middle and within 5 bases of an end
    for s in (400, 401):
        for p in (L // 2, L // 2 + 1, 3, 5, L - 4, L - 5):
            for e in (dele(p, 1), dele(p, 10), inse(p, 3)):
                pair(6, s, L + 75, edit1=e)
                pair(7, s, L + 76, edit2=e)
    # and a random fill with about 1 % substitutions
    for _ in range(120):
        ci = int(rng.integers(0, n_c))
        fl = int(rng.integers(L + 1, L + 200))
        s = int(rng.integers(0, len(cs[ci]) - fl))
        offs = [int(o) for o in np.nonzero(rng.random(L) < 0.01)[0]]
        pair(ci, s, fl, edit1=subs(*offs) if offs else None)
    return out


@functools.lru_cache(maxsize=None)
def _batch(L, bis, part=None):
    """the packed pairs; part 0 / 1: the even / odd ones"""
    ps = _pairs(L, bis, 31 * L + int(bis))
    if part is not None:
        ps = ps[part::2]
    return refio.pack_reads([a for a, _ in ps]) + refio.pack_reads([b for _, b in ps])


@functools.lru_cache(maxsize=None)
def _expected(L, bis, part=None):
    """the oracle's counts and insertions for a batch on an empty pileup (computed once, shared, never modified)"""
    b1, l1, b2, l2 = _batch(L, bis, part)
    o = oracle_py.Oracle(_index(bis), paired=True, bisulfite=bis, **PARAMS)
    m1, m2, mt, _, _ = o.map_batch(b1, l1, b2, l2, threads=8)
    return dict(m1=m1, m2=m2, mt=mt, counts=o.counts().copy(), ins=sorted(o.insertions()))


def _dev(bis):
    from pecaller_amd import PemapDev
    dev = PemapDev(0)
    ix = _index(bis)
    dev.build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
    dev.set_params(paired=True, bisulfite=bis, **PARAMS)
    return dev


def _same(counts, ins, exp_counts, exp_ins, tag):
    bad = np.nonzero((counts != exp_counts).any(axis=1))[0]
    assert bad.size == 0, (tag, bad[:10], counts[bad[:4]], exp_counts[bad[:4]])
    assert sorted(ins) == sorted(exp_ins), tag


@pytest.mark.parametrize("L,bis", [(64, False), (150, False), (64, True), (150, True)])
def test_run_boundaries(L, bis):
    exp = _expected(L, bis)
    b1, l1, b2, l2 = _batch(L, bis)
    dev = _dev(bis)
    m1, m2, mt = dev.map_batch(b1, l1, b2, l2)
    counts, ins = dev.fetch_pileup()
    stats, _ = dev.run_stats()
    dev.close()
    assert np.array_equal(m1, exp["m1"]) and np.array_equal(m2, exp["m2"]) and np.array_equal(mt, exp["mt"])
    _same(counts, ins, exp["counts"], exp["ins"], (L, bis))
    # what the batch was built to hold did map: plain diagonals and walked alignments, gaps of both kinds, the genome's two ends
    ec = exp["counts"]
    assert stats["walked"] > 10 and stats["walks"] - stats["walked"] > 100, stats
    assert int(ec[:, 4].sum()) > 50 and int(ec[:, 5].sum()) > 5
    assert ec[0].any()
    # (the read that ends on the genome's last base is in every batch; the reference's window stops 14 bases short of the genome's
    # end, so at 150 bases it maps clipped and the last position incremented is the 15th from the end; at 64 bases it does not map)
    if (L, bis) == (150, False):
        assert ec[-15].any() and not ec[-14:].any()
    g = _index(bis)["genome"]
    odd = np.nonzero(~np.isin(g, ACGT))[0]
    assert int((ec[odd, 0] > 0).sum()) >= 3         # column A under odd reference letters: plane 0 without agreement


def _in_child(*args):
    """the tests that write or read the counters through a torch view run in a process of their own, torch initialised first as
    bench.py does: this file as a program (see the end)"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and b"child ok" in r.stdout, r.stdout[-3000:].decode(errors="replace")


def test_form_changes_between_batches():
    _in_child("form")


def _child_form(torch):
    from pecaller_amd import dist as pd
    L, bis = 150, False
    ea, eb = _expected(L, bis, 0), _expected(L, bis, 1)
    a, b = _batch(L, bis, 0), _batch(L, bis, 1)
    both = ea["counts"] + eb["counts"]          # (uint16: modulo 2^16 like the counters)
    dev = _dev(bis)
    # map half A, fetch, map half B, fetch
    dev.map_batch(*a)
    _same(*dev.fetch_pileup(), ea["counts"], ea["ins"], "A")
    dev.map_batch(*b)
    _same(*dev.fetch_pileup(), both, ea["ins"] + eb["ins"], "A + B")
    rec = dev.fetch_records()
    nz = np.nonzero(both.any(axis=1))[0]
    assert np.array_equal(rec["pos"], nz.astype(np.uint32))
    # reset in between: B alone
    dev.reset_pileup()
    dev.map_batch(*a)
    dev.reset_pileup()
    dev.map_batch(*b)
    _same(*dev.fetch_pileup(), eb["counts"], eb["ins"], "B after reset")
    # a view of buffer 4 taken before map_batch holds the counts after it, with no library call in between
    dev.reset_pileup()
    view = pd.device_tensor(torch, dev, 4)
    dev.map_batch(*a)
    torch.cuda.synchronize()
    words = view.cpu().numpy().view(np.uint32)
    direct = dev.read_buffer(4, np.uint32)
    assert np.array_equal(words, direct)
    plane0 = words[:len(words) // 6].view(np.uint16)[:dev.gsize]
    g = _index(bis)["genome"]
    code = np.full(256, -1)
    for k, ch in enumerate(b"ACGT"):
        code[ch] = k
    col = np.where(code[g] >= 0, code[g], 0)
    assert np.array_equal(plane0, ea["counts"][np.arange(dev.gsize), col])
    # two asynchronous slices, sync, fetch
    dev.reset_pileup()
    r1, l1, r2, l2 = _batch(L, bis)
    n = len(l1)
    # (the even pairs first, then the odd ones: the two halves the expectations were computed for)
    order = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
    dev.stage_reads(r1[order].copy(), l1[order].copy(), r2[order].copy(), l2[order].copy())
    na = len(a[1])
    dev.run_slice(0, na, sync=False)
    dev.run_slice(na, n - na, sync=False)
    dev.sync()
    _same(*dev.fetch_pileup(), both, ea["ins"] + eb["ins"], "two slices")
    dev.close()


@pytest.mark.parametrize("fresh_is_dst", [False, True])
def test_absorb_between_forms(fresh_is_dst):
    """one object in the form a run leaves (slices run and synchronised, nothing folded), the other freshly reset"""
    L, bis = 150, False
    ea = _expected(L, bis, 0)
    run, fresh = _dev(bis), _dev(bis)
    run.stage_reads(*_batch(L, bis, 0))
    run.run(sync=True)
    fresh.map_batch(*_batch(L, bis, 1))
    fresh.reset_pileup()
    dst, src = (fresh, run) if fresh_is_dst else (run, fresh)
    dst.absorb(src)
    _same(*dst.fetch_pileup(), ea["counts"], ea["ins"], "absorbed")
    assert not src.read_buffer(4, np.uint32).any()
    run.close()
    fresh.close()


def _n_reads(n, L):
    return refio.pack_reads([b"N" * L] * n) + refio.pack_reads([b"N" * L] * n)


def _plane_words(g):
    return ((g + 2) // 2 + 63) & ~63


# genome lengths whose plane ends exactly on a scan-tile boundary, one 64-word block short of it and one block past it
# (and one of many tiles with a half-used last word)
@pytest.mark.parametrize("gsize", [2 * (2 * SCAN_TILE_WORDS) - 2, 2 * (2 * SCAN_TILE_WORDS - 64) - 2, 2 * (2 * SCAN_TILE_WORDS + 64) - 2, 33001])
def test_conversions_alone_are_bit_exact(gsize):
    _in_child("conversions", gsize)


def _child_conversions(torch, gsize):
    from pecaller_amd import PemapDev, dist as pd
    rng = np.random.default_rng(gsize)
    genome = ACGT[rng.integers(0, 4, gsize)].copy()
    dev = PemapDev(0)
    dev.build_index(genome, np.array([gsize], np.uint32))
    dev.set_params(paired=True, **PARAMS)
    pw = _plane_words(gsize)
    assert dev.buffer(4)[1] == 6 * pw * 4
    if gsize < 10000:
        assert (pw % SCAN_TILE_WORDS) in (0, 64, SCAN_TILE_WORDS - 64)
    reads = _n_reads(256, 64)
    presets = []
    alt = np.zeros(6 * pw, np.uint32)
    alt[:pw] = 0xFFFF0000
    alt[:pw:3] = 0x0000FFFF
    presets.append(alt)
    half = np.full(6 * pw, 0x80008000, np.uint32)
    half[:pw:5] = 0x00008000
    half[1:pw:7] = 0x80000000
    presets.append(half)
    presets.append(rng.integers(0, 1 << 32, 6 * pw, dtype=np.uint64).astype(np.uint32))
    for k, preset in enumerate(presets):
        if k < 2:
            preset[pw:] = rng.integers(0, 1 << 32, 5 * pw, dtype=np.uint64).astype(np.uint32)      # planes 1-5: random words
        view = pd.device_tensor(torch, dev, 4)
        view.copy_(torch.from_numpy(preset.view(np.int32)))
        torch.cuda.synchronize()
        m1, m2, mt = dev.map_batch(*reads)
        assert not m1.any() and not m2.any()
        got = dev.read_buffer(4, np.uint32)
        bad = np.nonzero(got != preset)[0]
        assert bad.size == 0, (gsize, k, bad[:10], got[bad[:4]], preset[bad[:4]])
        # and through a run that is only synchronised, then folded by the read
        dev.stage_reads(*reads)
        dev.run(sync=True)
        assert np.array_equal(dev.read_buffer(4, np.uint32), preset), (gsize, k)
    dev.close()


def test_wrap_under_the_reads():
    _in_child("wrap")


def _child_wrap(torch):
    from pecaller_amd import dist as pd
    L, bis = 150, False
    exp = _expected(L, bis)
    dev = _dev(bis)
    pw = _plane_words(dev.gsize)
    # plane-0 counters of every third position (both parities) preset to 0xFFFE / 0xFFFF; their neighbours share their words
    pos = np.arange(0, dev.gsize, 3)
    val = np.where((pos // 3) % 2 == 0, 0xFFFE, 0xFFFF).astype(np.uint16)
    plane0 = np.zeros(2 * pw, np.uint16)
    plane0[pos] = val
    view = pd.device_tensor(torch, dev, 4)
    view[:pw] = torch.from_numpy(plane0.view(np.int32))
    torch.cuda.synchronize()
    dev.map_batch(*_batch(L, bis))
    counts, ins = dev.fetch_pileup()
    words = dev.read_buffer(4, np.uint32)
    dev.close()
    g = _index(bis)["genome"]
    code = np.full(256, -1)
    for k, ch in enumerate(b"ACGT"):
        code[ch] = k
    col = np.where(code[g] >= 0, code[g], 0)          # the column plane 0 holds at each position (PmPile's rotation)
    want = exp["counts"].copy()
    want[pos, col[pos]] += val          # modulo 2^16
    _same(counts, ins, want, exp["ins"], "wrap")
    assert int(((exp["counts"][pos, col[pos]].astype(np.int64) + val) > 65535).sum()) > 1000       # they did wrap
    # the padding behind the genome's last position is as it was preset: zero
    assert not words[:pw].view(np.uint16)[dev.gsize:].any()


if __name__ == "__main__":
    import torch
    torch.cuda.set_device(0)
    if sys.argv[1] == "form":
        _child_form(torch)
    elif sys.argv[1] == "conversions":
        _child_conversions(torch, int(sys.argv[2]))
    else:
        _child_wrap(torch)
    print("child ok")
