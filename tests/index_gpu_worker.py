"""Child process of test_gpu_index_cases.py: the device-built index of the ladder genome (index_cases.py) checked over ALL 2^32 k-mers.
torch is initialised first, as bench.py does, and only extracts from the library's buffers (pecaller_amd.dist.device_tensor: views,
no copies) what numpy then compares with refio.kmer_index's arrays: the change points of the prefix table, the occupied entries of
look-up replica 0, and whether replicas 1..7 are replica 0 with two 4-bit fields of the k-mer swapped.

  python index_gpu_worker.py arrays|replicas plain|bisulfite full|trunc
"""
import json
import os
import sys
import time

import numpy as np
import torch

torch.cuda.set_device(0)

import fixtures  # noqa: E402
import index_cases as ic  # noqa: E402
import refio  # noqa: E402
from pecaller_amd import PemapDev, dist as pd  # noqa: E402

CHUNK = 1 << 28
N_KMERS = 1 << 32


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def change_points(pi):
    """-> (k, pi[k]) for every k with pi[k + 1] != pi[k], over the whole table"""
    ks, vs = [], []
    for o in range(0, N_KMERS, CHUNK):
        c = pi[o:o + CHUNK + 1]
        nz = torch.nonzero(c[1:] != c[:-1]).flatten()
        ks.append((nz + o).cpu().numpy().astype(np.uint32))
        vs.append(u32(c[nz]))
    return np.concatenate(ks), np.concatenate(vs)


def occupied(rep0):
    """-> (k, rep0[k]) for every entry of replica 0 that is not the empty marker"""
    ks, vs = [], []
    for o in range(0, N_KMERS, CHUNK):
        c = rep0[o:o + CHUNK]
        nz = torch.nonzero(c != -1).flatten()
        ks.append((nz + o).cpu().numpy().astype(np.uint32))
        vs.append(u32(c[nz]))
    return np.concatenate(ks), np.concatenate(vs)


def check_arrays(dev, ix, meta):
    n_mers, gsize, n_contigs, idepth = dev.index_info()
    assert (n_mers, gsize, n_contigs, idepth) == (len(ix["mers"]), len(ix["genome"]), len(ix["contig_len"]), 16)
    mers = dev.read_buffer(1, np.uint32)
    assert mers.tobytes() == ix["mers"].tobytes()
    if meta is not None:
        assert (n_mers, gsize) == (meta["n_mers"], meta["seq_len"])
        assert refio.md5(mers) == meta["mdx_md5"] and refio.md5(dev.read_buffer(2, np.uint8)) == meta["seq_md5"]
    assert np.array_equal(dev.read_buffer(3, np.uint32), ix["contig_starts"])
    assert np.array_equal(dev.read_buffer(2, np.uint8), ix["genome"])
    pi = pd.device_tensor(torch, dev, 0)
    assert pi.numel() == N_KMERS + 1
    k, v = change_points(pi)
    assert np.array_equal(k, ix["ukmer"]) and np.array_equal(v, ix["ustart"][:-1])
    assert u32(pi[N_KMERS:])[0] == n_mers == ix["ustart"][-1]
    if meta is not None:
        assert refio.md5(k) == meta["idx_ukmer_md5"] and refio.md5(np.concatenate([v, [np.uint32(n_mers)]]).astype(np.uint32)) == meta["idx_ustart_md5"]


def swap_fields(k, p):
    """the k-mer with its 4-bit fields 0 and p exchanged (int64 tensors)"""
    sh = 4 * p
    f0, fp = k & 15, (k >> sh) & 15
    return (k & ~(15 | (15 << sh))) | (f0 << sh) | fp


def check_replicas(dev, ix):
    n_rep, rec_bytes = dev.lookup_replicas()
    assert n_rep == 8, "an MI355X has the memory for the replicas: they must be in use"
    n_mers, gsize, _, _ = dev.index_info()
    mers = ix["mers"]
    uk = ix["ukmer"]
    start = ix["ustart"][:-1].astype(np.int64)
    ln = np.diff(ix["ustart"].astype(np.int64))
    assert int(uk[-1]) == 0xFFFFFFFF
    ln[-1] = (0 - int(start[-1])) & 0xFFFFFFFF          # `which + 1` wraps to entry 0 (pemapper.c:2163)
    rep = pd.device_tensor(torch, dev, 5)
    assert rep.numel() == 8 * N_KMERS
    t0 = time.time()
    k, e = occupied(rep[:N_KMERS])
    # the expected table is 0xFFFFFFFF everywhere but at the occupied k-mers
    assert np.array_equal(k, uk)
    one, many, rec = ln == 1, ln >= ic.TOO_MANY, (ln >= 2) & (ln < ic.TOO_MANY)
    assert np.array_equal(e[one], mers[start[one]])
    assert (e[many] == 0xFFFFFFFE).all() and many[-1]
    # 2 .. 99 positions: a pointer to a record of (ln + 4) / 4 units of four words: the count, the positions in .mdx order, zeros
    multi = dev.read_buffer(6, np.uint32)
    units = (ln[rec] + 4) // 4
    assert multi.nbytes == rec_bytes == 16 * int(units.sum())
    ptr = e[rec].astype(np.int64)
    assert ((ptr >= gsize) & (ptr < 0xFFFFFFFE)).all()
    off = ptr - gsize
    order = np.argsort(off, kind="stable")
    assert off[order][0] == 0 and np.array_equal(off[order][1:], np.cumsum(units[order])[:-1])       # the records tile the buffer
    words = off * 4
    assert np.array_equal(multi[words], ln[rec].astype(np.uint32))
    lens, starts = ln[rec], start[rec]
    for n in np.unique(lens):                # all records of one length at a time
        sel = np.nonzero(lens == n)[0]
        got = multi[words[sel, None] + 1 + np.arange(4 * ((n + 4) // 4) - 1)]
        assert np.array_equal(got[:, :n], mers[starts[sel, None] + np.arange(n)]), n
        assert (got[:, n:] == 0).all(), n
    seen = {int(n): int((ln == n).sum()) for n in ic.ISLANDS}
    assert all(v > 0 for v in seen.values()) and seen[99] > 0 and seen[100] > 0, seen
    assert set(np.unique(units).tolist()) >= {1, 2, 3, 4, 25}
    t1 = time.time()
    # replicas 1 .. 7: rep[p][swap_fields(k, p)] == rep[0][k] for every k
    times = []
    for p in range(1, 8):
        t = time.time()
        rp = rep[p * N_KMERS:(p + 1) * N_KMERS]
        for o in range(0, N_KMERS, CHUNK):
            kk = torch.arange(o, o + CHUNK, dtype=torch.int64, device="cuda")
            assert bool((rp[swap_fields(kk, p)] == rep[o:o + CHUNK]).all()), (p, o)
        torch.cuda.synchronize()
        times.append(round(time.time() - t, 2))
    return dict(replica0_s=round(t1 - t0, 2), permuted_s=times, seen=seen)


def main():
    what, mode, size = sys.argv[1:4]
    bis = mode == "bisulfite"
    ix = ic.index(bis, trunc=size == "trunc")
    with open(os.path.join(fixtures.GOLD, "ladder.json")) as f:
        meta = json.load(f)[mode] if size == "full" else None
    t = time.time()
    dev = PemapDev(0)
    dev.build_index(ix["genome"], ix["contig_len"], bisulfite=bis)
    out = dict(build_s=round(time.time() - t, 2))
    t = time.time()
    if what == "arrays":
        check_arrays(dev, ix, meta)
    else:
        out.update(check_replicas(dev, ix))
    out["check_s"] = round(time.time() - t, 2)
    dev.close()
    print("index ok", json.dumps(out))


if __name__ == "__main__":
    main()
