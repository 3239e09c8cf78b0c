"""pecaller_amd/csrc/pemap_seed_entry.h -- where lane j of a seed wave finds the table entry of neighbour j of a k-mer -- on the
CPU, for all 64 lanes of 100,004 k-mers: the header is compiled for the host into a small shared object (tests/csrc/seed_entry_check.c)
and held against the neighbour order of fill_mers (restated here in numpy and pinned to the oracle's ora_neighbours) and the
replicas' permutation (test_gpu_pemap._swap_fields, the one the replica tests use).  No GPU is needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_py
from test_gpu_pemap import _swap_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pecaller_amd", "csrc", "pemap_seed_entry.h")
SRC = os.path.join(ROOT, "tests", "csrc", "seed_entry_check.c")
EDGES = [0, 0xFFFFFFFF, 0x0000000F, 0xF0000000]


def neighbours(k):
    """-> [n, 49] uint64: column 0 the k-mers, then their 48 single-substitution neighbours, 2-bit fields from the low end,
    alternatives ascending (fill_mers, pemapper.c:1969-2003)"""
    k = np.asarray(k, dtype=np.uint64)
    out = np.empty((len(k), 49), np.uint64)
    out[:, 0] = k
    for f in range(16):
        sh = np.uint64(2 * f)
        cur = (k >> sh) & np.uint64(3)
        base = k & ~(np.uint64(3) << sh)
        for a in range(3):
            alt = np.uint64(a) + (np.uint64(a) >= cur).astype(np.uint64)
            out[:, 1 + 3 * f + a] = base + (alt << sh)
    return out


def replica_of_lane(j):
    """the replica (= 4-bit field of the k-mer) that holds the base neighbour j replaces; the k-mer itself: replica 0"""
    return 0 if j == 0 else ((j - 1) // 3) // 2


@pytest.fixture(scope="module")
def kmers():
    rng = np.random.default_rng(15)
    return np.concatenate([rng.integers(0, 1 << 32, size=100000, dtype=np.uint64), np.array(EDGES, np.uint64)]).astype(np.uint32)


@pytest.fixture(scope="module")
def tables(kmers, tmp_path_factory):
    so = str(tmp_path_factory.mktemp("seed_entry") / "seed_entry_check.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, SRC])
    lib = ctypes.CDLL(so)
    outs = []
    for fn in (lib.seed_entry_table, lib.seed_entry_table_two_step):
        fn.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
        fn.restype = None
        out = np.full((len(kmers), 64), -7, np.int64)
        fn(kmers.ctypes.data, len(kmers), out.ctypes.data)
        outs.append(out)
    return outs


def test_the_numpy_neighbour_order_is_the_oracles(kmers):
    L = oracle_py.lib()
    sample = np.concatenate([kmers[:500], kmers[-len(EDGES):]])
    nb = neighbours(sample)
    buf = np.zeros(49, np.uint32)
    for i, k in enumerate(sample.tolist()):
        L.ora_neighbours(k, buf.ctypes.data)
        assert np.array_equal(buf.astype(np.uint64), nb[i]), hex(k)


def test_lanes_0_to_48_give_the_replica_entry_of_their_neighbour(kmers, tables):
    nb = neighbours(kmers)
    for t in tables:
        for j in range(49):
            p = replica_of_lane(j)
            want = (np.uint64(p) << np.uint64(32)) + _swap_fields(nb[:, j], p)
            assert np.array_equal(t[:, j].astype(np.uint64), want), j
            assert (t[:, j] >= 0).all()


def test_lanes_49_to_63_are_off(tables):
    for t in tables:
        assert (t[:, 49:] == -1).all()


def test_the_49_entries_lie_in_eight_lines_one_per_replica(tables):
    """a line is 16 entries of 4 bytes; the lanes of one replica are neighbours in the wave"""
    for t in tables:
        lines = t[:, :49] >> 4
        rep = t[:, :49] >> 32
        assert np.array_equal(rep, np.broadcast_to(np.array([replica_of_lane(j) for j in range(49)]), rep.shape))
        for p in range(8):
            mine = lines[:, [j for j in range(49) if replica_of_lane(j) == p]]
            assert mine.shape[1] == (7 if p == 0 else 6)
            assert (mine == mine[:, :1]).all(), p
        srt = np.sort(lines, axis=1)
        assert ((srt[:, 1:] != srt[:, :-1]).sum(axis=1) + 1 == 8).all()


def test_the_header_is_plain_c():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-function", "-fsyntax-only", "-x", "c", HEADER])
