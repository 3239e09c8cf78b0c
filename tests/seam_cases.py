"""Plans for the host pipeline of the mapper (run_slice / ring_setup of pemap_capi.hip): which batches are submitted, in which order and
with which lengths, so that a run continues a pending pipeline with several chunks, fills the table of 256 chunks, changes the longest
read between batches in flight and re-makes the ring.  No GPU in here: tests/test_seam_cases_cpu.py asserts what the plans reach,
tests/test_gpu_chunk_seam.py runs them.

CHUNK is the PEMAP_CHUNK_PAIRS of the child processes that run the r150 plans; MAX_CHUNKS restates PM_MAX_CHUNKS.  All rows have stride
304 unless a plan says otherwise.

One batch of the plan `remade` is not what was first written down for it: its last batch (reads of up to 278 bases) was to have stride
160, which no row of 278 bases fits (the C-ABI refuses a read longer than the stride).  It has stride 304: the ring is re-made a third
time, with the 1,500-pair batch in flight, and the bound rises from at most 120 to 278 as intended."""
import functools
import numpy as np
import fixtures
import refio

CHUNK = 64
MAX_CHUNKS = 256
STRIDE = 304
NARROW = 160
PARAMS = dict(min_dist=0, max_dist=500, min_align=0.85)

COMP = np.zeros(256, np.uint8)
COMP[:] = ord("N")
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b


def ragged_reads(seed, n, lo, hi):
    """pairs from the fixture genome with independent random lengths per end, 1 % substitutions, a few indels, some junk"""
    rng = np.random.default_rng(seed)
    _, contigs = fixtures.genome()
    r1, r2 = [], []
    for k in range(n):
        c = contigs[int(rng.integers(0, len(contigs)))]
        la, lb = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
        fl = int(rng.integers(max(la, lb) + 20, max(la, lb) + 400))
        s = int(rng.integers(0, len(c) - fl - 1))
        a = c[s:s + la].copy()
        b = COMP[c[s + fl - lb:s + fl]][::-1].copy()
        for x in (a, b):
            m = rng.random(len(x)) < 0.01
            x[m] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(m.sum()))]
        if k % 50 == 0 and la > 40:
            a = np.concatenate([a[:20], a[23:]])                      # a 3-base deletion
        if k % 50 == 1 and lb > 40:
            b = np.concatenate([b[:25], np.frombuffer(b"AC", np.uint8), b[25:]])[:hi]
        if k % 97 == 0:
            a[:] = ord("N")                                          # filtered by the N rule
        if k % 97 == 1:
            a[:] = ord("A")                                          # every bucket over the too-many-spots limit
        if k % 97 == 2:
            a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, la)]   # junk
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a.tobytes())
        r2.append(b.tobytes())
    return refio.pack_reads(r1) + refio.pack_reads(r2)


def chunks_of(n, chunk=CHUNK):
    """chunks run_slice cuts a run of n pairs into, and their size: the wanted chunk, raised when the run would need more than the table holds"""
    chunk = min(chunk, n)
    if -(-n // chunk) > MAX_CHUNKS:
        chunk = -(-n // MAX_CHUNKS)
    return -(-n // chunk), chunk


# ---- the r150 plans: cuts of the golden 2 x 150 set (its 20,000 pairs), as lists of (first, end)
UNEVEN_SIZES = [1000, 1, 63, 64, 65, 127, 128, 129, 1000, 640, 999, 257, 512, 333, 1000, 65, 768, 129, 1000, 500]
N_R150 = 20000


def uneven():
    """batches of uneven size, the first the largest; the list above, repeated until the set is used up"""
    cuts, at, k = [], 0, 0
    while at < N_R150:
        n = min(UNEVEN_SIZES[k % len(UNEVEN_SIZES)], N_R150 - at)
        cuts.append((at, at + n))
        at += n
        k += 1
    return cuts


EXACT_FILL_BATCHES, EXACT_FILL_PAIRS = 70, 256


def exact_fill():
    """70 batches of 4 chunks: the 64th fills the table exactly, the 65th does not fit"""
    return [(k * EXACT_FILL_PAIRS, (k + 1) * EXACT_FILL_PAIRS) for k in range(EXACT_FILL_BATCHES)]


def one_run():
    return [(0, N_R150)]


# ---- the ragged plans: lists of dict(reads = (b1, l1, b2, l2), stride, hi)
LENGTHS_HI = [60, 104, 105, 112, 113, 160, 161, 208, 209, 256, 257, 278, 150, 40, 278, 100]
LENGTHS_PAIRS = 200
SEG_EDGES = (112, 160, 208, 256)          # seg_template: 7 / 10 / 13 / 16 / 19 segments
GEOM_EDGES = (104, 160, 208, 256)         # pemap_dev_sw_geom with the default knobs: 8 x 13, 16 x 10 / 13 / 16 / 19


def seg_template(L):
    segs = -(-L // 16)
    return 7 if segs <= 7 else 10 if segs <= 10 else 13 if segs <= 13 else 16 if segs <= 16 else 19


def sw_geom(L):
    return (8, 13) if L <= 104 else (16, 10) if L <= 160 else (16, 13) if L <= 208 else (16, 16) if L <= 256 else (16, 19)


def _force_first(reads, seed, hi):
    """the first pair's first end becomes a read of exactly hi bases"""
    b1, l1, b2, l2 = reads
    _, contigs = fixtures.genome()
    c = contigs[seed % len(contigs)]
    s = 1000 + 37 * (seed % 1000)
    b1[0, :] = 0
    b1[0, :hi] = c[s:s + hi]
    l1[0] = hi
    return b1, l1, b2, l2


def _plant_deletion(reads, seed, L):
    """ragged_reads plants its indels in ends of more than 40 bases only: a batch of shorter reads gets a second pair whose first end
    skips 3 reference bases behind its 20th, so that the traceback and the deletion plane have work in every batch"""
    b1, l1, b2, l2 = reads
    _, contigs = fixtures.genome()
    c = contigs[(seed + 3) % len(contigs)]
    s = 5000 + 41 * (seed % 1000)
    for buf, ln, x in ((b1, l1, np.concatenate([c[s:s + 20], c[s + 23:s + L + 3]])), (b2, l2, COMP[c[s + 200:s + 200 + L]][::-1])):
        buf[1, :] = 0
        buf[1, :L] = x
        ln[1] = L
    return b1, l1, b2, l2


def restride(reads, stride):
    b1, l1, b2, l2 = reads
    assert max(int(l1.max()), int(l2.max())) <= stride
    return np.ascontiguousarray(b1[:, :stride]), l1, np.ascontiguousarray(b2[:, :stride]), l2


@functools.lru_cache(maxsize=None)
def lengths():
    out = []
    for k, hi in enumerate(LENGTHS_HI):
        lo = hi if hi in (104, 257) else 16
        seed = 7100 + k
        reads = _force_first(ragged_reads(seed, LENGTHS_PAIRS, lo, hi), seed, hi)
        if hi <= 40:
            reads = _plant_deletion(reads, seed, hi)
        out.append(dict(reads=reads, stride=STRIDE, hi=hi, lo=lo))
    return out


@functools.lru_cache(maxsize=None)
def remade():
    spec = [(8101, 300, 16, 278, STRIDE), (8102, 300, 16, 150, NARROW), (8103, 1500, 16, 120, NARROW), (8104, 300, 16, 278, STRIDE)]
    return [dict(reads=restride(ragged_reads(seed, n, lo, hi), stride), stride=stride, hi=hi, lo=lo) for seed, n, lo, hi, stride in spec]


PARAMS_MAX_DIST = (500, 100)


@functools.lru_cache(maxsize=None)
def params():
    """two paired batches (max_dist 500), then -- behind set_params (paired = False, max_dist = 100) -- the first mates of a third"""
    out = [dict(reads=ragged_reads(8201 + k, 300, 100, 278), stride=STRIDE, hi=278, lo=100, paired=True, max_dist=PARAMS_MAX_DIST[0]) for k in range(2)]
    b1, l1, _, _ = ragged_reads(8203, 300, 100, 278)
    out.append(dict(reads=(b1, l1, None, None), stride=STRIDE, hi=278, lo=100, paired=False, max_dist=PARAMS_MAX_DIST[1]))
    return out


def fold(m1, m2, mt, l1, l2, paired, max_dist):
    """the 13 summary numbers of one delivered batch (pemapper.c:1238-1265): total_reads, total_bases, total_dist, no_dists, mate_counts"""
    S = np.zeros(13, np.int64)
    a = m1.astype(np.int64)
    b = m2.astype(np.int64) if (paired and m2 is not None) else np.zeros(len(m1), np.int64)
    lb = l2.astype(np.int64) if paired else np.zeros(len(m1), np.int64)
    S[4:] = np.bincount(mt, minlength=9)
    S[0] = (a > 0).sum() + (b > 0).sum()
    S[1] = l1.astype(np.int64)[a > 0].sum() + lb[b > 0].sum()
    dist = (a - b) % (1 << 32)                   # the unsigned difference widened to long
    near = (a > 0) & (b > 0) & (dist < max_dist * 4)
    S[2] = dist[near].sum()
    S[3] = near.sum()
    return S


# ---- what the oracle makes of the ragged plans: computed once per process, shared by the tests, never changed
def _oracle_run(batches, **prm):
    """one oracle maps the batches in order -> per batch (m1, m2, mt, insertions logged so far, deletion counts so far), and the oracle"""
    import oracle_py
    o = oracle_py.Oracle(fixtures.index(), **prm)
    per = []
    for b in batches:
        m1, m2, mt, _, _ = o.map_batch(*b["reads"], threads=8)
        per.append(dict(m1=m1, m2=m2, mt=mt, n_ins=len(o.insertions()), n_del=int(o.counts()[:, 4].astype(np.int64).sum())))
    return per, o


def _final(os_):
    counts = os_[0].counts().copy()
    for o in os_[1:]:
        counts = counts + o.counts()                     # (uint16: the sum wraps as the device's counters do)
    ins = sorted(x for o in os_ for x in o.insertions())
    return dict(counts=counts, ins=ins, summary=sum(np.array(o.summary()) for o in os_))


@functools.lru_cache(maxsize=None)
def oracle(plan):
    """plan: "lengths", "remade", "params" or "params_dist" (the first paired batch of params alone, under max_dist 500 and under 100)
    -> dict(per = per-batch results, final = dict(counts, ins, summary), seconds)"""
    import time
    t0 = time.time()
    if plan in ("lengths", "remade"):
        per, o = _oracle_run({"lengths": lengths, "remade": remade}[plan](), paired=True, **PARAMS)
        fin = _final([o])
    elif plan == "params":
        bs = params()
        per, o1 = _oracle_run(bs[:2], paired=True, **PARAMS)
        per3, o2 = _oracle_run(bs[2:], paired=False, **dict(PARAMS, max_dist=PARAMS_MAX_DIST[1]))
        per, fin = per + per3, _final([o1, o2])
    else:
        bs = params()[:1]
        per, o = _oracle_run(bs, paired=True, **PARAMS)
        fin = _final([o])
        fin["summary_narrow"] = np.array(_oracle_run(bs, paired=True, **dict(PARAMS, max_dist=PARAMS_MAX_DIST[1]))[1].summary())
    return dict(per=per, final=fin, seconds=time.time() - t0)
