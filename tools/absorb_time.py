#!/usr/bin/env python3
"""What pemap_dev_absorb and pemap_dev_index_share cost on an hg38-sized genome: two objects on device 0, look-up replicas off.

  python3 tools/absorb_time.py [--genome-size 3.1e9] [--reps 7]

Object A is created with the knobs unset, object B with PEMAP_ABSORB_STAGED=1 (the knobs are read when an object is created), so
A.absorb(B) takes the direct way -- pm_pile_add_kernel reads B's planes in place -- and B.absorb(A) the staged way, the one two
physical GPUs take: pieces of PEMAP_ABSORB_CHUNK KiB through two staging buffers.  HIP events on the null stream around each call
(the call ends with the device idle, so they bracket everything it does), medians of `reps` after two warm-up calls.  A call is
more than its kernel: it also zeroes the source's planes (pemap_dev_reset_pileup), timed here on its own as well.  Bytes: the add
reads both objects' planes and writes one (3 N), the reset writes N, the staged way copies N once more (read + write: 2 N).
Both objects sit on ONE GPU: the staged figures say what the staging costs there and nothing about a link between two GPUs."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HBM_TBS = 6.3


class Events:
    """hipEvent timing through the HIP runtime the library itself loaded (found in this process's map, not by name)"""

    def __init__(self):
        path = [l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l][0]
        self.hip = C.CDLL(path)
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time_ms(self, call):
        assert self.hip.hipEventRecord(self.a, None) == 0
        call()
        assert self.hip.hipEventRecord(self.b, None) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value


def median_ms(ev, call, reps):
    return float(np.median([ev.time_ms(call) for _ in range(reps + 2)][2:]))


def line(name, ms, nbytes):
    tbs = nbytes / (ms * 1e-3) / 1e12
    print("  %-44s %9.3f ms  %8.2f GB  %5.2f TB/s = %4.1f %% of %.1f TB/s" % (name, ms, nbytes / 1e9, tbs, 100.0 * tbs / HBM_TBS, HBM_TBS), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-size", type=float, default=3.1e9)
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--share-reps", type=int, default=3)
    a = ap.parse_args()
    from pecaller_amd import PemapDev
    os.environ["PEMAP_REPLICAS"] = "0"
    os.environ.pop("PEMAP_ABSORB_STAGED", None)
    A = PemapDev(0)
    os.environ["PEMAP_ABSORB_STAGED"] = "1"
    B = PemapDev(0)
    gsize = int(a.genome_size)
    t0 = time.time()
    d_g, contig_len = A.synth_genome(1, gsize, a.contigs, 0.5)
    A.build_index_resident(d_g, gsize, contig_len)
    A.free(d_g)
    print("index of %d letters built in %.1f s" % (gsize, time.time() - t0), flush=True)
    ev = Events()
    # ---- index_share: index_alloc (with the zeroing of the new planes), the four copies, index_commit without replicas
    n_idx = sum(A.buffer(w)[1] for w in (0, 1, 2, 3))
    ms = [ev.time_ms(lambda: B.index_share(A)) for _ in range(a.share_reps + 1)][1:]
    assert B.index_info() == A.index_info()
    print("pemap_dev_index_share, %d calls after one warm-up: %s ms" % (a.share_reps, " ".join("%.1f" % x for x in ms)))
    line("index_share (copied bytes, read + write)", float(np.median(ms)), 2 * n_idx)
    # ---- absorb
    N = A.buffer(4)[1]
    print("pileup planes: %.2f GB per object; medians of %d calls after two warm-ups" % (N / 1e9, a.reps))
    t_reset = median_ms(ev, B.reset_pileup, a.reps)
    line("reset_pileup alone (writes N)", t_reset, N)
    t_direct = median_ms(ev, lambda: A.absorb(B), a.reps)
    line("absorb, direct: whole call (3 N + reset N)", t_direct, 4 * N)
    line("absorb, direct: call less the reset (3 N)", t_direct - t_reset, 3 * N)
    t_staged = median_ms(ev, lambda: B.absorb(A), a.reps)
    line("absorb, staged: whole call (5 N + reset N)", t_staged, 6 * N)
    line("absorb, staged: call less the reset (5 N)", t_staged - t_reset, 5 * N)
    A.close()
    B.close()


if __name__ == "__main__":
    main()
