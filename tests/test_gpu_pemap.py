"""GPU parity tests: the HIP path, called through the C-ABI (libpemap_hip.so), against the reference's golden outputs
and against the oracle on the same inputs.  Bit-exact: integer coordinates, counters, and fp64 SW scores."""
import numpy as np
import pytest
import fixtures
import oracle_py
import refio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from pecaller_amd import PemapDev
    d = PemapDev(0)
    ix = fixtures.index()
    d.build_index(ix["genome"], ix["contig_len"])
    yield d
    d.close()


def test_device_index_equals_reference_index(dev):
    """pemap_dev_build_index must produce the arrays index_genome_whole.c writes (.mdx bytes, .idx prefix table)."""
    ix = fixtures.index()
    m = fixtures.meta()["index"]
    n_mers, gsize, n_contigs, idepth = dev.index_info()
    assert (n_mers, gsize, n_contigs, idepth) == (m["n_mers"], m["seq_len"], 10, 16)
    mers = dev.read_buffer(1, np.uint32)
    assert refio.md5(mers) == m["mdx_md5"]
    assert np.array_equal(dev.read_buffer(3, np.uint32), ix["contig_starts"])
    assert np.array_equal(dev.read_buffer(2, np.uint8), ix["genome"])
    # prefix table: pos_index[k] = number of indexed positions whose k-mer is < k; checked on four 64 Mi-entry
    # windows, on both ends, and at every bucket boundary
    uk, us = ix["ukmer"].astype(np.int64), ix["ustart"]
    W = 1 << 26
    for start in (0, (1 << 30) + 12345, (1 << 31) - W // 2, (1 << 32) + 1 - W):
        got = dev.read_buffer(0, np.uint32, offset_bytes=start * 4, n_bytes=W * 4)
        k = np.arange(start, start + W, dtype=np.int64)
        exp = us[np.searchsorted(uk, k, side="left")]
        assert np.array_equal(got, exp), start
    full_last = dev.read_buffer(0, np.uint32, offset_bytes=(1 << 32) * 4, n_bytes=4)
    assert full_last[0] == n_mers
    rng = np.random.default_rng(1)
    for i in rng.integers(0, len(uk), size=2000):
        two = dev.read_buffer(0, np.uint32, offset_bytes=int(uk[i]) * 4, n_bytes=8)
        assert two[0] == us[i] and two[1] == us[i + 1]


def _swap_fields(k, p):
    k = np.asarray(k, dtype=np.uint64)
    sh = np.uint64(4 * p)
    f0, fp = k & np.uint64(15), (k >> sh) & np.uint64(15)
    return (k & ~(np.uint64(15) | (np.uint64(15) << sh))) | (f0 << sh) | fp


def test_lookup_replicas_encode_the_reference_table(dev):
    """The 8 re-ordered copies of the table that serve the look-ups on the device: every sampled entry must say what
    pos_index / mers say about its bucket (get_mers, pemapper.c:2158-2165): empty, the only position, the record of 2..99
    positions in .mdx order, or the too_many_spots marker."""
    ix = fixtures.index()
    n_rep, rec_bytes = dev.lookup_replicas()
    assert n_rep == 8, "an MI355X has the memory for the replicas: they must be in use"
    n_mers, gsize, _, _ = dev.index_info()
    uk, us = ix["ukmer"].astype(np.int64), ix["ustart"].astype(np.int64)
    mers = dev.read_buffer(1, np.uint32)
    multi = dev.read_buffer(6, np.uint32)
    assert multi.nbytes == rec_bytes
    ln_of = dict(zip(uk.tolist(), (us[1:] - us[:-1]).tolist()))
    st_of = dict(zip(uk.tolist(), us[:-1].tolist()))
    rng = np.random.default_rng(5)
    ks = set(uk[rng.integers(0, len(uk), size=600)].tolist())
    big = uk[np.nonzero((us[1:] - us[:-1]) >= 2)[0]]
    ks |= set(big[rng.integers(0, len(big), size=300)].tolist()) if len(big) else set()
    ks |= set(rng.integers(0, 1 << 32, size=100).tolist()) | {0, (1 << 32) - 1}
    # every bucket on or over too_many_spots (one of 386 positions in this genome): the marker entries of populated buckets
    over = uk[np.nonzero((us[1:] - us[:-1]) >= 100)[0]]
    assert len(over) >= 1
    ks |= set(over.tolist())
    # neighbours of a few of them: the entries the kernel reads from the same lines
    for k in list(ks)[:50]:
        for f in range(16):
            ks.add(k ^ (1 << (2 * f)))
    seen = {0: 0, 1: 0, 2: 0, 100: 0}
    for k in sorted(ks):
        ln = ln_of.get(k, 0)
        if k == (1 << 32) - 1:      # `which + 1` wraps to entry 0 (pemapper.c:2163): pos_index[0] - pos_index[k] in 32 bits
            ln = (0 - st_of.get(k, n_mers)) & 0xFFFFFFFF
        for p in range(8):
            d = int(_swap_fields(k, p))
            e = int(dev.read_buffer(5, np.uint32, offset_bytes=((p << 32) + d) * 4, n_bytes=4)[0])
            if ln == 0:
                assert e == 0xFFFFFFFF, (k, p)
            elif ln >= 100:
                assert e == 0xFFFFFFFE, (k, p)
            elif ln == 1:
                assert e == mers[st_of[k]], (k, p)
            else:
                assert gsize <= e < 0xFFFFFFFE, (k, p)
                o = (e - gsize) * 4
                assert multi[o] == ln and np.array_equal(multi[o + 1:o + 1 + ln], mers[st_of[k]:st_of[k] + ln]), (k, p)
        seen[0 if ln == 0 else 1 if ln == 1 else 2 if ln < 100 else 100] += 1
    assert seen[1] > 100 and seen[2] > 100 and seen[0] > 100
    assert seen[100] >= len(over) + 1           # (+ 1: the absent all-T k-mer, whose wrapped length is huge)
    # one whole window of replica 0 (the reference's order): emptiness agrees with the prefix table everywhere
    W = 1 << 24
    start = int(uk[len(uk) // 2]) & ~(W - 1)
    win = dev.read_buffer(5, np.uint32, offset_bytes=start * 4, n_bytes=W * 4)
    pi = dev.read_buffer(0, np.uint32, offset_bytes=start * 4, n_bytes=(W + 1) * 4).astype(np.int64)
    lens = pi[1:] - pi[:-1]
    assert np.array_equal(win == 0xFFFFFFFF, lens == 0)
    assert np.array_equal(win == 0xFFFFFFFE, lens >= 100)
    one = lens == 1
    assert np.array_equal(win[one], mers[pi[:-1][one]])


def test_run_stats_times_cover_every_stage(dev):
    """the eight kernel times of run_stats (pemap_hip.h) are sums of event intervals of the run's chunks; an interval between
    a wrong pair of events fails silently and leaves 0.  Every stage that launches a kernel must show a time, and the seed
    stage's time holds its look-ups' (and, with the reference's table layout, the vote kernel's, which the fused seed kernel
    does not have) whatever the GPU's speed: the intervals are nested.  (Replicas 8 first: the layout the test before leaves.)"""
    r1, l1, r2, l2 = fixtures.reads("r150")
    dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
    for replicas in (8, 0):
        dev.set_lookup_replicas(replicas)
        dev.reset_pileup()
        dev.map_batch(r1, l1, r2, l2)
        _, t = dev.run_stats()
        print(replicas, t)
        assert sorted(t) == sorted(["seed", "sw_single", "sw_multi", "select", "sw_redo", "walk", "lookup", "vote"])
        assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
        if replicas == 8:
            for k in ("seed", "lookup", "sw_single", "sw_multi", "select", "sw_redo", "walk"):
                assert t[k] > 0, (k, t)
            assert t["seed"] >= t["lookup"], t
        else:
            assert t["vote"] > 0, t
            assert t["seed"] >= t["lookup"] + t["vote"], t


@pytest.mark.parametrize("replicas", [8, 0])
@pytest.mark.parametrize("name", ["r150", "r100", "r250"])
def test_map_matches_reference_golden(dev, name, replicas):
    s = fixtures.SETS[name]
    r1, l1, r2, l2 = fixtures.reads(name)
    # 8: the look-ups read the replicas (the default on an MI355X); 0: the reference's table (pm_lookup_wave_kernel)
    dev.set_lookup_replicas(replicas)
    assert dev.lookup_replicas()[0] == replicas
    dev.set_params(paired=s["paired"], min_dist=0, max_dist=500, min_align=0.85)
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(r1, l1, r2, l2)
    g1 = fixtures.golden_m(name, 1)
    assert np.array_equal(m1, g1), "m1 differs at %s" % np.nonzero(m1 != g1)[0][:10]
    if s["paired"]:
        g2 = fixtures.golden_m(name, 2)
        assert np.array_equal(m2, g2), "m2 differs at %s" % np.nonzero(m2 != g2)[0][:10]
    counts, ins = dev.fetch_pileup()
    rec = fixtures.check_pileup_against_golden(name, counts)
    # the compacted record stream the pileup writer consumes is the same thing
    assert np.array_equal(dev.fetch_records(), rec)
    names, contigs = fixtures.genome()
    gold_ins, _ = fixtures.golden_insertions(name)
    assert fixtures.ins_to_named(ins, names, contigs) == gold_ins
    tot, head, rows = fixtures.golden_summary(name)
    sm = dev.summary()
    assert sm[0] == tot
    assert head[3] == "%g" % (sm[1] / sm[0])
    assert head[7] == "%g" % ((sm[2] / sm[3]) if sm[3] else 0.0)
    if s["paired"]:
        assert rows["Unique Mate-Paired"] == sm[4] and rows["Non-Unique Mate-Paired"] == sm[8] and rows["Neither Map"] == sm[12]
    else:
        assert rows["Unique Mapping"] == sm[6] and rows["Non-Unique Mapping, discarded"] == sm[11]


def test_load_index_entry_takes_the_reference_arrays():
    """pemap_dev_load_index, the first entry of the drop-in ABI and the one INTEGRATION.md's patch calls: the reference's own
    in-memory index (init_index_buffer, pemapper.c:2129-2155: the 2^32+1-entry prefix table of the .idx file, the .mdx position
    lists, the .seq letters, the compressed contig starts) handed over from host memory.  The look-up replicas are built from
    the host-supplied tables; the r150 goldens must come out, with the replicas and with the reference's layout."""
    from pecaller_amd import PemapDev
    ix = fixtures.index()
    uk, us = ix["ukmer"].astype(np.int64), ix["ustart"]
    # pos_index[k] = number of indexed positions whose 16-mer is < k
    lens = np.concatenate([[uk[0] + 1], np.diff(uk), [(1 << 32) - uk[-1]]])
    pos_index = np.repeat(us, lens)
    assert pos_index.dtype == np.uint32 and len(pos_index) == (1 << 32) + 1 and pos_index[-1] == len(ix["mers"])
    d = PemapDev(0)
    d.load_index(pos_index, ix["mers"], ix["genome"], ix["contig_starts"])
    del pos_index
    assert d.index_info() == (len(ix["mers"]), len(ix["genome"]), 10, 16)
    assert d.lookup_replicas()[0] == 8
    r1, l1, r2, l2 = fixtures.reads("r150")
    for replicas in (8, 0):
        d.set_lookup_replicas(replicas)
        d.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
        d.reset_pileup()
        m1, m2, mt = d.map_batch(r1, l1, r2, l2)
        assert np.array_equal(m1, fixtures.golden_m("r150", 1)) and np.array_equal(m2, fixtures.golden_m("r150", 2))
        counts, ins = d.fetch_pileup()
        fixtures.check_pileup_against_golden("r150", counts)
    d.close()


def test_hits_and_scores_match_oracle(dev):
    """per read-end: the hit list (spot, strand) in order, the SW window, and per hit the fp64 score bits and start cell"""
    ix = fixtures.index()
    r1, l1, r2, l2 = fixtures.reads("r150")
    n = 4000
    dev.set_lookup_replicas(8)
    dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(r1[:n], l1[:n], r2[:n], l2[:n])
    dbg = dev.debug_hits(2 * n)
    o = oracle_py.Oracle(ix, paired=True)
    om1, om2, omt, d1, d2 = o.map_batch(r1[:n], l1[:n], r2[:n], l2[:n], debug=True, threads=8)
    assert np.array_equal(m1, om1) and np.array_equal(m2, om2) and np.array_equal(mt, omt)
    multi = 0
    for which, od in ((0, d1), (1, d2)):
        nh = dbg["n_hits"][which::2]
        assert np.array_equal(nh, od["n_hits"])
        for i in np.nonzero(nh)[0]:
            k = nh[i]
            e = 2 * i + which
            assert np.array_equal(dbg["spot"][e, :k], od["spot"][i, :k])
            assert np.array_equal(dbg["orient"][e, :k], od["orient"][i, :k])
            assert np.array_equal(dbg["win_start"][e, :k].astype(np.int32), od["win_start"][i, :k])
            assert np.array_equal(dbg["win_len"][e, :k], od["win_len"][i, :k])
            # scores as bits
            assert np.array_equal(dbg["score"][e, :k].view(np.uint64), od["score"][i, :k].view(np.uint64)), (e, k)
            assert np.array_equal(dbg["start_k"][e, :k], od["start"][i, :k, 0])
            assert np.array_equal(dbg["start_i"][e, :k], od["start"][i, :k, 1])
            multi += k > 1
    assert multi > 10
    stats, times = dev.run_stats()
    assert stats["ends"] == 2 * n and stats["sw_score"] == int(dbg["n_hits"].sum())
    assert stats["walks"] == int((m1 > 0).sum() + (m2 > 0).sum())


def test_rerun_is_additive_and_slices_compose(dev):
    """running the staged batch twice doubles every counter; two half slices equal one full run"""
    r1, l1, r2, l2 = fixtures.reads("r150")
    n = 2000
    dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
    dev.reset_pileup()
    dev.stage_reads(r1[:n], l1[:n], r2[:n], l2[:n])
    dev.run()
    a1 = dev.collect()
    c1, i1 = dev.fetch_pileup()
    dev.run()
    dev.collect()
    c2, i2 = dev.fetch_pileup()
    assert np.array_equal(c2, (2 * c1.astype(np.uint32)).astype(np.uint16))
    assert len(i2) == 2 * len(i1)
    dev.reset_pileup()
    dev.run_slice(0, n // 2)
    b1 = dev.collect()
    dev.run_slice(n // 2, n - n // 2)
    b2 = dev.collect()
    c3, i3 = dev.fetch_pileup()
    assert np.array_equal(c3, c1) and i3 == i1
    assert np.array_equal(np.concatenate([b1[0], b2[0]]), a1[0])
    assert np.array_equal(np.concatenate([b1[1], b2[1]]), a1[1])


def test_batches_in_flight_equal_one_call(dev):
    """pemap_dev_submit_batch / pemap_dev_wait_batch: uneven batches queued three deep (copies, kernels and result copies of
    different batches overlap, the fourth submit delivers the oldest), waited for out of order, must give what one synchronous
    call gives -- coordinates, classes, pileup, insertions, summary -- and so must two host threads calling map_batch on one object."""
    import threading
    r1, l1, r2, l2 = fixtures.reads("r150")
    dev.set_lookup_replicas(8)
    dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
    cuts = [0, 3000, 3001, 9000, 12000, 16500, 20000]
    dev.reset_pileup()
    dev.pin_host(r1)                   # one buffer pinned by the caller (DMA straight out of it), the other staged by the library
    tickets = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        tickets.append((a, b, dev.submit_batch(r1[a:b], l1[a:b], r2[a:b], l2[a:b])))
    m1 = np.zeros(20000, np.uint32)
    m2 = np.zeros(20000, np.uint32)
    mt = np.zeros(20000, np.int32)
    for a, b, t in reversed(tickets):
        x1, x2, xt = dev.wait_batch(t)
        m1[a:b], m2[a:b], mt[a:b] = x1, x2, xt
    dev.unpin_host(r1)
    assert np.array_equal(m1, fixtures.golden_m("r150", 1)) and np.array_equal(m2, fixtures.golden_m("r150", 2))
    counts, ins = dev.fetch_pileup()
    fixtures.check_pileup_against_golden("r150", counts)
    names, contigs = fixtures.genome()
    assert fixtures.ins_to_named(ins, names, contigs) == fixtures.golden_insertions("r150")[0]
    tot, head, rows = fixtures.golden_summary("r150")
    sm = dev.summary()
    assert sm[0] == tot and rows["Unique Mate-Paired"] == sm[4] and rows["Neither Map"] == sm[12]
    assert head[3] == "%g" % (sm[1] / sm[0]) and head[7] == "%g" % (sm[2] / sm[3])
    # two host threads, one batch each at a time (the reference's worker threads)
    dev.reset_pileup()
    out = {}

    def worker(k):
        for a in range(k * 2500, 20000, 5000):
            out[a] = dev.map_batch(r1[a:a + 2500], l1[a:a + 2500], r2[a:a + 2500], l2[a:a + 2500])
    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert np.array_equal(np.concatenate([out[a][0] for a in sorted(out)]), fixtures.golden_m("r150", 1))
    assert np.array_equal(np.concatenate([out[a][2] for a in sorted(out)]), mt)
    counts, ins = dev.fetch_pileup()
    fixtures.check_pileup_against_golden("r150", counts)
    assert dev.summary()[0] == tot
    # six worker threads (more than the ring's three slots: submits queue up behind a full ring and must each keep a slot of
    # their own -- the round-2 review's slot race), then two threads that keep two batches in flight each (four over three slots)
    for mode in ("map_batch x 6", "submit, submit, wait x 2"):
        dev.reset_pileup()
        out = {}
        errs = []

        def worker6(k):
            try:
                for a in range(k * 500, 20000, 3000):
                    out[a] = dev.map_batch(r1[a:a + 500], l1[a:a + 500], r2[a:a + 500], l2[a:a + 500])
            except Exception as e:          # noqa: BLE001
                errs.append(e)

        def worker2(k):
            try:
                starts = list(range(k * 1000, 20000, 2000))
                for i in range(0, len(starts), 2):
                    pend = [(a, dev.submit_batch(r1[a:a + 1000], l1[a:a + 1000], r2[a:a + 1000], l2[a:a + 1000])) for a in starts[i:i + 2]]
                    for a, t in pend:
                        out[a] = dev.wait_batch(t)
            except Exception as e:          # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=worker6, args=(k,)) for k in range(6)] if mode.startswith("map") else [threading.Thread(target=worker2, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, (mode, errs)
        assert np.array_equal(np.concatenate([out[a][0] for a in sorted(out)]), fixtures.golden_m("r150", 1)), mode
        assert np.array_equal(np.concatenate([out[a][1] for a in sorted(out)]), fixtures.golden_m("r150", 2)), mode
        assert np.array_equal(np.concatenate([out[a][2] for a in sorted(out)]), mt), mode
        counts, ins = dev.fetch_pileup()
        fixtures.check_pileup_against_golden("r150", counts)
        assert dev.summary()[0] == tot, mode


def test_torch_tensors_alias_the_library_buffers():
    """what the multi-GPU start-up relies on: torch views of pemap_dev_buffer pointers share memory with the library, so an RCCL
    broadcast into them lands in the index the kernels read (pecaller_amd/dist.py: device_tensor).  In a process of its own,
    torch initialised first as bench.py does (torch brings its own HIP runtime)."""
    import subprocess
    import sys
    code = r'''
import sys, numpy as np, torch
torch.cuda.set_device(0)
import fixtures
from pecaller_amd import PemapDev, dist as pd
ix = fixtures.index()
dev = PemapDev(0)
dev.build_index(ix["genome"], ix["contig_len"])
for which in (0, 1, 2, 3):
    t = pd.device_tensor(torch, dev, which)
    host = dev.read_buffer(which, np.uint8 if which == 2 else np.uint32, n_bytes=min(4096, t.numel() * t.element_size()))
    got = t[:len(host)].cpu().numpy()
    assert np.array_equal(got if which == 2 else got.view(np.uint32), host), which
t = pd.device_tensor(torch, dev, 3)
old = t.clone()
t[0] = 12345
torch.cuda.synchronize()
assert dev.read_buffer(3, np.uint32)[0] == 12345
t.copy_(old)
torch.cuda.synchronize()
assert np.array_equal(dev.read_buffer(3, np.uint32), ix["contig_starts"])
dev.close()
print("alias ok")
'''
    import os
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]))
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and b"alias ok" in r.stdout, r.stdout[-2000:]


def test_pileup_counters_wrap_like_unsigned_short():
    """the device keeps the reference's unsigned short counters two to a 32-bit word (PmPile) and increments them with 32-bit
    atomics: a low half that passes 65,535 must wrap to 0 WITHOUT carrying into the counter that shares its word.  The plane-0
    counters of the first 40,000 even positions start at 65,535 (words of plane 0 preset to 0x0000FFFF through the torch view of
    the buffer; plane 0 holds the column of the reference base itself, fixtures.plane0_column), the reads are mapped -- most of
    their increments land exactly there, many of them as one add to both halves of a word -- and every column must be the golden
    pileup modulo 2^16; the odd positions' counters, in the high halves of those words, exactly the golden."""
    import subprocess
    import sys
    code = r'''
import numpy as np, torch
torch.cuda.set_device(0)
import fixtures
from pecaller_amd import PemapDev, dist as pd
ix = fixtures.index()
dev = PemapDev(0)
dev.build_index(ix["genome"], ix["contig_len"])
r1, l1, r2, l2 = fixtures.reads("r150")
dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
cnt = pd.device_tensor(torch, dev, 4)
cnt[:20000] = 0xFFFF
torch.cuda.synchronize()
dev.map_batch(r1, l1, r2, l2)
counts, _ = dev.fetch_pileup()
rows = np.arange(0, 40000, 2)
col = fixtures.plane0_column(rows)
bumped = counts[rows, col].copy()
assert (bumped != 65535).sum() > 8000          # the positions a read covers and agrees with (~3x coverage): those low halves did wrap
counts[rows, col] = (bumped.astype(np.uint32) + 1).astype(np.uint16)        # 65,535 + n = n - 1 modulo 2^16
fixtures.check_pileup_against_golden("r150", counts)
dev.close()
print("wrap ok")
'''
    import os
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]))
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0 and b"wrap ok" in r.stdout, r.stdout[-2000:]


def test_gapless_rule_counts_and_dp_schedules_match_golden(dev):
    """the gapless rule (pm_gapless_kernel) decides most alignments of the golden read set without the DP; its results are
    already pinned by the golden tests above -- here: it is in use, and the full-DP path (PEMAP_GAPLESS=0, a process of
    its own because the setting is read once) still reproduces the reference's outputs, hit scores included; so do the
    one-stream schedules (PEMAP_PIPELINE=2) of both table layouts"""
    import os
    import subprocess
    import sys
    r1, l1, r2, l2 = fixtures.reads("r150")
    dev.set_lookup_replicas(8)
    dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
    dev.reset_pileup()
    dev.map_batch(r1, l1, r2, l2)
    stats, _ = dev.run_stats()
    assert stats["gapless"] > stats["sw_score"] // 3, stats
    assert stats["gapless"] + (stats["sw_dirs"] - stats["redo"]) <= stats["sw_score"]
    code = r'''
import os, numpy as np, fixtures, oracle_py
from pecaller_amd import PemapDev
ix = fixtures.index()
dev = PemapDev(0)
dev.build_index(ix["genome"], ix["contig_len"])
for name in ("r150", "r100"):
    s = fixtures.SETS[name]
    r1, l1, r2, l2 = fixtures.reads(name)
    dev.set_params(paired=s["paired"], min_dist=0, max_dist=500, min_align=0.85)
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(r1, l1, r2, l2)
    st = dev.run_stats()[0]
    assert (st["gapless"] == 0) == (os.environ.get("PEMAP_GAPLESS") == "0")
    assert (st["banded"] == 0) == (os.environ.get("PEMAP_BAND") == "0" or os.environ.get("PEMAP_GAPLESS") == "0")
    assert np.array_equal(m1, fixtures.golden_m(name, 1))
    if s["paired"]:
        assert np.array_equal(m2, fixtures.golden_m(name, 2))
    counts, ins = dev.fetch_pileup()
    fixtures.check_pileup_against_golden(name, counts)
dev.close()
print("full dp ok")
'''
    here = os.path.dirname(os.path.abspath(__file__))
    # the full DP in the default pipeline (8 lanes x 19 columns per alignment for 150 bases); the gapless rule without the banded
    # DP behind it (what the rule leaves goes to the full DP, 16 lanes x 10); the two-stream pipeline's kernels on ONE stream; and
    # the same on the reference's table layout (the schedule no other test runs); and the rule with its first case only
    for extra in (dict(PEMAP_GAPLESS="0"), dict(PEMAP_BAND="0"), dict(PEMAP_PIPELINE="2"), dict(PEMAP_PIPELINE="2", PEMAP_REPLICAS="0"),
                  dict(PEMAP_GAPLESS="1")):
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here]), **extra)
        r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        assert r.returncode == 0 and b"full dp ok" in r.stdout, (extra, r.stdout[-2000:])


@pytest.mark.gpu
def test_scheduling_knobs_do_not_change_results():
    """every environment knob that is left (grids, wave priorities, the chunking) gives the reference's coordinates
    and pileup on the golden read sets: they are schedules, not algorithms.  One process per setting (the knobs are read once, when
    the library is loaded).  (Round 3 removed the knobs that moved kernels between streams: the first run of this test found one of
    them, unused since round 1, faulting.)"""
    import os
    import subprocess
    import sys
    code = r'''
import os, numpy as np, fixtures
from pecaller_amd import PemapDev
ix = fixtures.index()
dev = PemapDev(0)
dev.build_index(ix["genome"], ix["contig_len"])
for name in ("r150", "r250"):
    s = fixtures.SETS[name]
    r1, l1, r2, l2 = fixtures.reads(name)
    dev.set_params(paired=s["paired"], min_dist=0, max_dist=500, min_align=0.85)
    dev.reset_pileup()
    m1, m2, mt = dev.map_batch(r1, l1, r2, l2)
    assert np.array_equal(m1, fixtures.golden_m(name, 1))
    if s["paired"]:
        assert np.array_equal(m2, fixtures.golden_m(name, 2))
    counts, ins = dev.fetch_pileup()
    fixtures.check_pileup_against_golden(name, counts)
dev.close()
print("knob ok")
'''
    here = os.path.dirname(os.path.abspath(__file__))
    settings = [
        dict(PEMAP_CHUNK_PAIRS="4096"), dict(PEMAP_LOOKUP_WAVES="3", PEMAP_LOOKUP_PRIO="2"),
        dict(PEMAP_SW_PRIO="1", PEMAP_VOTE_PRIO="1", PEMAP_SW_WAVES_PER_CU="3", PEMAP_BAND_WAVES_PER_CU="2", PEMAP_GAPLESS_BLOCKS_PER_CU="3"),
        dict(PEMAP_WALK_BLOCKS_PER_CU="1", PEMAP_PILE_BLOCKS_PER_CU="1"),
        # the table layout of the reference (no replicas): the two-kernel seed stage, its vote on few waves
        dict(PEMAP_REPLICAS="0", PEMAP_VOTE_WAVES="64", PEMAP_BIG_BLOCKS_PER_CU="2"),
        # (0 is clamped to one wave per CU: the second tier still runs)
        dict(PEMAP_TIER2_WAVES="0"),
    ]
    for extra in settings:
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here]), **extra)
        r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0 and b"knob ok" in r.stdout, (extra, r.stdout[-2000:])


@pytest.mark.gpu
def test_pipeline_setting_outside_its_range_is_refused():
    """PEMAP_PIPELINE is 1 or 2; any other value (0 once selected a seed path that is gone) makes pemap_dev_create fail with an
    error that names the variable, instead of measuring something else.  In a child process, as the knob test does."""
    import os
    import subprocess
    import sys
    code = r'''
from pecaller_amd import PemapDev, PemapError
try:
    PemapDev(0)
except PemapError as e:
    assert "PEMAP_PIPELINE" in str(e), str(e)
    print("refused ok")
'''
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here]), PEMAP_PIPELINE="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"refused ok" in r.stdout, r.stdout[-2000:]
