"""ctypes mirror of the pecall_dev_* entry points of include/pemap_hip.h (PECaller per-site genotype likelihoods)."""
import ctypes as C
import os
import re
import numpy as np
from .pemap import load_library, PemapError

MAX_GEN = 14
ALLELES = 6
RC_UNORDERED = 3  # PECALL_RC_UNORDERED
# a pileup record: the 16 bytes of the pileup file
RECORD = np.dtype([("pos", "<u4"), ("counts", "<u2", (6,))])
# bytes of text a gzip member of base_gz holds at most (csrc/pecall_gz_rule.h, which states the whole rule)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "pecall_gz_rule.h")) as _f:
    PCG_PIECE = int(re.search(r"#define\s+PCG_PIECE\s+(\d+)u", _f.read()).group(1))


class PecallUnordered(PemapError):
    """a record stream does not ascend strictly or leaves the range (PECALL_RC_UNORDERED); .rc is the return code"""
    rc = RC_UNORDERED


def _p(a):
    return None if a is None else a.ctypes.data


class PecallDev:
    def __init__(self, device_id=0):
        L = load_library()
        vp, i, dbl = C.c_void_p, C.c_int, C.c_double
        L.pecall_dev_create.argtypes = [C.POINTER(vp), i]
        L.pecall_dev_destroy.argtypes = [vp]
        L.pecall_dev_destroy.restype = None
        L.pecall_dev_last_error.argtypes = [vp]
        L.pecall_dev_last_error.restype = C.c_char_p
        L.pecall_dev_site_like.argtypes = [vp, vp, vp, i, i, i, i, dbl, vp, vp, vp]
        L.pecall_dev_stage.argtypes = [vp, vp, vp, i, i]
        L.pecall_dev_run.argtypes = [vp, i, i, i, i, dbl, i]
        L.pecall_dev_collect.argtypes = [vp, i, i, vp, vp, vp]
        L.pecall_dev_call_sites.argtypes = [vp, vp, vp, vp, C.c_long, i, i, dbl, dbl, vp, vp, vp, vp, vp, vp]
        L.pecall_dev_call_sites_sparse.argtypes = [vp, vp, vp, vp, C.c_long, i, i, dbl, dbl, vp, vp, vp, C.c_uint64, vp, vp, vp, vp, vp]
        L.pecall_dev_set_pedigree.argtypes = [vp, i, vp, vp, vp, vp, vp, dbl]
        L.pecall_dev_sites_stage.argtypes = [vp, vp, vp, vp, C.c_long, i]
        L.pecall_dev_sites_run.argtypes = [vp, i, dbl, dbl, C.POINTER(C.c_float)]
        L.pecall_dev_sites_stats.argtypes = [vp, vp]
        L.pecall_dev_sites_collect.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.pecall_dev_pin_host.argtypes = [vp, vp, C.c_uint64]
        L.pecall_dev_unpin_host.argtypes = [vp, vp]
        u32, u64 = C.c_uint32, C.c_uint64
        L.pecall_dev_sites_stage_records.argtypes = [vp, vp, vp, i, u32, u32, vp, u32, vp, C.POINTER(C.c_long), vp]
        L.pecall_dev_sites_gather.argtypes = [vp, vp, u64, vp, vp, vp]
        L.pecall_dev_sites_merge_ms.argtypes = [vp, vp]
        L.pecall_dev_call_records.argtypes = [vp, vp, vp, i, u32, u32, vp, u32, vp, C.POINTER(C.c_long), vp,
                                              i, dbl, dbl, vp, vp, vp, u64, vp, vp, vp, vp, vp]
        L.pecall_dev_sites_stage_records_guided.argtypes = [vp, vp, vp, i, u32, u32, vp, u32, vp, vp, vp, u32, C.POINTER(C.c_long), vp]
        L.pecall_dev_call_records_guided.argtypes = [vp, vp, vp, i, u32, u32, vp, u32, vp, vp, vp, u32, C.POINTER(C.c_long), vp,
                                                     i, dbl, dbl, vp, vp, vp, u64, vp, vp, vp, vp, vp]
        L.pecall_dev_sites_base_text.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, u64, C.POINTER(u64), vp, vp, u64, C.POINTER(u64), vp]
        L.pecall_dev_sites_base_gz.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, u64, C.POINTER(u64), vp, vp, u64, C.POINTER(u64), C.POINTER(u64), vp]
        self.L = L
        h = vp()
        if L.pecall_dev_create(C.byref(h), device_id):
            raise PemapError(L.pecall_dev_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.pecall_dev_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _ck(self, rc):
        if rc:
            raise PemapError(self.L.pecall_dev_last_error(self.h).decode())

    def site_like(self, reads, alpha_mean, norm, max_gen=14, min_depth=2):
        """reads [n_sites][indiv][6] u16, alpha_mean [n_sites][14][6] f64 -> like [n_sites][indiv][14], best, margin"""
        reads = np.ascontiguousarray(reads, np.uint16)
        alpha_mean = np.ascontiguousarray(alpha_mean, np.float64)
        n_sites, indiv = reads.shape[:2]
        like = np.zeros((n_sites, indiv, MAX_GEN))
        best = np.zeros((n_sites, indiv), np.int8)
        margin = np.zeros((n_sites, indiv))
        self._ck(self.L.pecall_dev_site_like(self.h, _p(reads), _p(alpha_mean), n_sites, indiv, max_gen, min_depth, norm, _p(like),
                                             _p(best), _p(margin)))
        return like, best, margin

    def stage(self, reads, alpha_mean):
        reads = np.ascontiguousarray(reads, np.uint16)
        alpha_mean = np.ascontiguousarray(alpha_mean, np.float64)
        self._shape = reads.shape[:2]
        self._ck(self.L.pecall_dev_stage(self.h, _p(reads), _p(alpha_mean), reads.shape[0], reads.shape[1]))

    def run(self, norm, max_gen=14, min_depth=2, sync=True):
        self._ck(self.L.pecall_dev_run(self.h, self._shape[0], self._shape[1], max_gen, min_depth, norm, int(sync)))

    def collect(self):
        n_sites, indiv = self._shape
        like = np.zeros((n_sites, indiv, MAX_GEN))
        best = np.zeros((n_sites, indiv), np.int8)
        margin = np.zeros((n_sites, indiv))
        self._ck(self.L.pecall_dev_collect(self.h, n_sites, indiv, _p(like), _p(best), _p(margin)))
        return like, best, margin

    def set_pedigree(self, dad, mom, sex, kid_off, kid_list, denovo_rate):
        """parents as sample indices (-1 = none), sex, kids of i = kid_list[kid_off[i]:kid_off[i+1]] in ped-file order; None clears"""
        if dad is None:
            self._ck(self.L.pecall_dev_set_pedigree(self.h, 0, None, None, None, None, None, 0.0))
            return
        a = [np.ascontiguousarray(x, np.int32) for x in (dad, mom, sex, kid_off, kid_list)]
        self._ck(self.L.pecall_dev_set_pedigree(self.h, len(a[0]), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), float(denovo_rate)))

    def sites_stage(self, reads, ref_base, chrom=None):
        reads = np.ascontiguousarray(reads, np.uint16)
        ref_base = np.ascontiguousarray(ref_base, np.uint8)
        cy = None if chrom is None else np.ascontiguousarray(chrom, np.uint8)
        self._sshape = reads.shape[:2]
        self._ck(self.L.pecall_dev_sites_stage(self.h, _p(reads), _p(ref_base), _p(cy), reads.shape[0], reads.shape[1]))

    def sites_run(self, threshold=0.95, theta=0.001, haploid=False):
        """the kernel on the staged columns -> its duration in ms (HIP events on the object's stream)"""
        ms = C.c_float(0)
        self._rindiv = self._sshape[1]
        self._ck(self.L.pecall_dev_sites_run(self.h, int(haploid), float(threshold), float(theta), C.byref(ms)))
        return ms.value

    def sites_stats(self):
        """how the last sites_run divided its columns (pecall_dev_sites_stats) -> dict(columns, listed [4], deep, early [4]): columns the
        shortcut kernels left to the beam search by unsettled samples (< 3, < 8, < 20, more), columns on the deep list, columns whose
        beam search started ahead of the shortcut kernels by samples with variant reads (< 12, < 20, < 32, more)"""
        out = np.zeros(10, np.uint64)
        self._ck(self.L.pecall_dev_sites_stats(self.h, _p(out)))
        v = [int(x) for x in out]
        return dict(columns=v[0], listed=v[1:5], deep=v[5], early=v[6:10])

    def sites_collect(self):
        n_sites, indiv = self._sshape
        call = np.zeros((n_sites, indiv), np.int8)
        post = np.zeros((n_sites, indiv))
        typ = np.zeros(n_sites, np.int8)
        ac = np.zeros((n_sites, ALLELES), np.int32)
        npass = np.zeros(n_sites, np.int8)
        self.denovo = np.zeros(n_sites, np.int32)
        self._ck(self.L.pecall_dev_sites_collect(self.h, _p(call), _p(post), _p(typ), _p(ac), _p(npass), _p(self.denovo)))
        return call, post, typ, ac, npass

    def _ck_records(self, rc):
        if rc == RC_UNORDERED:
            raise PecallUnordered(self.L.pecall_dev_last_error(self.h).decode())
        self._ck(rc)

    @staticmethod
    def _record_args(recs, span, ref_letters, chrom):
        """recs: per sample an array of records ((n, 16) bytes, RECORD, or anything of 16 bytes a row) -> the arrays (kept alive by
        the caller), their addresses, their lengths, the letters and the chromosome bytes"""
        keep = []
        for r in recs:
            r = np.ascontiguousarray(r)
            if r.size and r.nbytes % 16:
                raise ValueError("a record is 16 bytes")
            keep.append(r)
        ptrs = (C.c_void_p * len(keep))(*[r.ctypes.data if r.nbytes else None for r in keep])
        n = np.array([r.nbytes // 16 for r in keep], np.uint64)
        if isinstance(ref_letters, str):
            ref_letters = ref_letters.encode()
        letters = np.frombuffer(bytes(ref_letters), np.uint8) if not isinstance(ref_letters, np.ndarray) else np.ascontiguousarray(ref_letters).view(np.uint8)
        cy = None
        if chrom is not None:
            cy = np.ascontiguousarray(chrom, np.uint8)
            if cy.size != span:
                raise ValueError("chrom has one byte per position of the range")
        return keep, ptrs, n, letters, cy

    def sites_stage_records(self, recs, p0, span, ref_letters, chrom=None):
        """columns from the samples' records of [p0, p0 + span) (pecall_dev_sites_stage_records): recs = a list of per-sample record
        arrays, ref_letters = the reference letters from p0 on (at most span), chrom = per position of the range or None
        -> n_cols, col_slot [n_cols]; the columns are staged for sites_run / sites_collect / sites_gather"""
        keep, ptrs, n, letters, cy = self._record_args(recs, span, ref_letters, chrom)
        col_slot = np.zeros(max(int(span), 1), np.uint32)
        n_cols = C.c_long(0)
        rc = self.L.pecall_dev_sites_stage_records(self.h, C.addressof(ptrs), _p(n), len(keep), int(p0), int(span), _p(letters) if letters.size else None,
                                                   letters.size, _p(cy), C.byref(n_cols), _p(col_slot))
        self._ck_records(rc)
        self._sshape = (n_cols.value, len(keep))
        return n_cols.value, col_slot[:n_cols.value]

    def sites_gather(self, cols=None):
        """the staged columns (all, or those listed) -> reads [n][indiv][6] u16, ref [n] u8, chrom [n] u8"""
        n_sites, indiv = self._sshape
        c = None if cols is None else np.ascontiguousarray(cols, np.uint32)
        n = n_sites if c is None else c.size
        reads = np.zeros((n, indiv, ALLELES), np.uint16)
        ref = np.zeros(n, np.uint8)
        cy = np.zeros(n, np.uint8)
        if n:
            self._ck(self.L.pecall_dev_sites_gather(self.h, _p(c), n, _p(reads), _p(ref), _p(cy)))
        return reads, ref, cy

    def sites_merge_ms(self):
        """kernel times of the last sites_stage_records in ms: mark, scan, tile"""
        ms = np.zeros(3, np.float32)
        self._ck(self.L.pecall_dev_sites_merge_ms(self.h, _p(ms)))
        return ms

    def call_records(self, recs, p0, span, ref_letters, threshold=0.95, theta=0.001, haploid=False, chrom=None, cap=None):
        """sites_stage_records and the caller in one call (pecall_dev_call_records)
        -> call, (post_site, post_rows), site_type, allele_count, n_pass as call_sites_sparse returns them, for the n_cols columns, and col_slot"""
        keep, ptrs, n, letters, cy = self._record_args(recs, span, ref_letters, chrom)
        indiv = len(keep)
        call, _, typ, ac, npass, den = self.out_arrays(max(int(span), 1), indiv, posterior=False)
        cap = int(cap) if cap is not None else max(1024, int(span) // 8)
        site, rows = np.empty(cap, np.uint32), np.empty((cap, indiv), np.float64)
        col_slot = np.zeros(max(int(span), 1), np.uint32)
        n_cols, n_post = C.c_long(0), C.c_uint64(0)
        self.sparse_needed = 0
        self._rindiv = indiv
        rc = self.L.pecall_dev_call_records(self.h, C.addressof(ptrs), _p(n), indiv, int(p0), int(span), _p(letters) if letters.size else None, letters.size, _p(cy),
                                            C.byref(n_cols), _p(col_slot), int(haploid), float(threshold), float(theta), _p(call), _p(site), _p(rows), cap,
                                            C.byref(n_post), _p(typ), _p(ac), _p(npass), _p(den))
        self.sparse_needed = int(n_post.value)
        self._ck_records(rc)
        m = n_cols.value
        self._sshape = (m, indiv)
        self.denovo = den[:m]
        return call[:m], (site[:n_post.value], rows[:n_post.value]), typ[:m], ac[:m], npass[:m], col_slot[:m]

    @staticmethod
    def _interval_args(iv_first, iv_count, iv_chrom):
        first = np.ascontiguousarray(iv_first, np.uint32)
        count = np.ascontiguousarray(iv_count, np.uint32)
        cy = None if iv_chrom is None else np.ascontiguousarray(iv_chrom, np.uint8)
        if count.size != first.size or (cy is not None and cy.size != first.size):
            raise ValueError("iv_first, iv_count and iv_chrom have one entry per interval")
        return first, count, cy

    def sites_stage_records_guided(self, recs, p0, span, ref_letters, iv_first, iv_count, iv_chrom=None):
        """columns at every position of the intervals (pecall_dev_sites_stage_records_guided): recs, p0, span, ref_letters as for
        sites_stage_records; interval k holds the slots iv_first[k] .. iv_first[k] + iv_count[k] - 1 (slot = position - p0), its
        columns get the chromosome byte iv_chrom[k] (None: 0) -> n_cols, col_slot [n_cols]"""
        keep, ptrs, n, letters, _ = self._record_args(recs, span, ref_letters, None)
        first, count, cy = self._interval_args(iv_first, iv_count, iv_chrom)
        col_slot = np.zeros(max(int(span), 1), np.uint32)
        n_cols = C.c_long(0)
        rc = self.L.pecall_dev_sites_stage_records_guided(self.h, C.addressof(ptrs), _p(n), len(keep), int(p0), int(span), _p(letters) if letters.size else None,
                                                          letters.size, _p(first), _p(count), _p(cy), first.size, C.byref(n_cols), _p(col_slot))
        self._ck_records(rc)
        self._sshape = (n_cols.value, len(keep))
        return n_cols.value, col_slot[:n_cols.value]

    def call_records_guided(self, recs, p0, span, ref_letters, iv_first, iv_count, iv_chrom=None, threshold=0.95, theta=0.001, haploid=False, cap=None):
        """sites_stage_records_guided and the caller in one call (pecall_dev_call_records_guided) -> as call_records"""
        keep, ptrs, n, letters, _ = self._record_args(recs, span, ref_letters, None)
        first, count, cy = self._interval_args(iv_first, iv_count, iv_chrom)
        indiv = len(keep)
        call, _, typ, ac, npass, den = self.out_arrays(max(int(span), 1), indiv, posterior=False)
        cap = int(cap) if cap is not None else max(1024, int(span) // 8)
        site, rows = np.empty(cap, np.uint32), np.empty((cap, indiv), np.float64)
        col_slot = np.zeros(max(int(span), 1), np.uint32)
        n_cols, n_post = C.c_long(0), C.c_uint64(0)
        self.sparse_needed = 0
        self._rindiv = indiv
        rc = self.L.pecall_dev_call_records_guided(self.h, C.addressof(ptrs), _p(n), indiv, int(p0), int(span), _p(letters) if letters.size else None, letters.size,
                                                   _p(first), _p(count), _p(cy), first.size, C.byref(n_cols), _p(col_slot), int(haploid), float(threshold),
                                                   float(theta), _p(call), _p(site), _p(rows), cap, C.byref(n_post), _p(typ), _p(ac), _p(npass), _p(den))
        self.sparse_needed = int(n_post.value)
        self._ck_records(rc)
        m = n_cols.value
        self._sshape = (m, indiv)
        self.denovo = den[:m]
        return call[:m], (site[:n_post.value], rows[:n_post.value]), typ[:m], ac[:m], npass[:m], col_slot[:m]

    def base_text(self, names, contig, pos, ref_char, text_cap=None, hole_cap=None, pin=False):
        """the .base rows of the last call's columns from the device (pecall_dev_sites_base_text): names = the contig names (str or
        bytes), contig / pos / ref_char per column -> (text bytes, hole_site, hole_at): the rows of the columns that are neither
        skipped nor holes; the caller's own row of column hole_site[k] belongs at byte hole_at[k].  text_cap / hole_cap default
        to the bound (every column a row of the longest form, every column a hole); a failure for want of room leaves what is
        needed in self.text_needed / self.holes_needed.  pin: the text buffer is page-locked for the call.
        self.rows_ms = the kernels' durations (length, scan, fill)"""
        nm = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
        blob = np.frombuffer(b"".join(nm) + b"\0", np.uint8)
        name_off = np.concatenate([[0], np.cumsum([len(x) for x in nm])]).astype(np.uint32)
        contig = np.ascontiguousarray(contig, np.int32)
        pos = np.ascontiguousarray(pos, np.uint32)
        ref = np.frombuffer(ref_char.encode() if isinstance(ref_char, str) else bytes(ref_char), np.uint8) if not isinstance(ref_char, np.ndarray) else np.ascontiguousarray(ref_char).view(np.uint8)
        n = len(contig)
        if len(pos) != n or ref.size != n:
            raise ValueError("contig, pos and ref_char have one entry per column")
        indiv = getattr(self, "_rindiv", 0) or 512          # (samples of the last call)
        if text_cap is None:
            text_cap = n * (14 + max([len(x) for x in nm] + [0]) + 4 * indiv)
        if hole_cap is None:
            hole_cap = n
        text = np.zeros(max(int(text_cap), 1), np.uint8)
        site, at = np.zeros(max(int(hole_cap), 1), np.uint32), np.zeros(max(int(hole_cap), 1), np.uint64)
        n_text, n_holes = C.c_uint64(0), C.c_uint64(0)
        ms = np.zeros(3, np.float32)
        if pin:
            self.pin_host(text)
        try:
            rc = self.L.pecall_dev_sites_base_text(self.h, _p(blob), _p(name_off), len(nm), _p(contig), _p(pos), _p(ref), _p(text), int(text_cap),
                                                   C.byref(n_text), _p(site), _p(at), int(hole_cap), C.byref(n_holes), _p(ms))
        finally:
            if pin:
                self.unpin_host(text)
        self.text_needed, self.holes_needed, self.rows_ms = int(n_text.value), int(n_holes.value), ms
        self._ck(rc)
        return text[:n_text.value].tobytes(), site[:n_holes.value], at[:n_holes.value]

    def base_gz(self, names, contig, pos, ref_char, gz_cap=None, hole_cap=None, pin=False):
        """the same rows as gzip members deflated on the device (pecall_dev_sites_base_gz), arguments as base_text ->
        (gz bytes, hole_site, hole_gz_at): inflating gz gives base_text's text; the caller's own row of column hole_site[k], as a
        member of its own, belongs at byte hole_gz_at[k] of gz, a member boundary.  gz_cap defaults to the bound (every column a
        row of the longest form, each piece of PCG_PIECE bytes stored, a piece more per column).  A failure for want of room leaves
        what is needed in self.gz_needed / self.holes_needed.  self.text_needed = the inflated length; self.gz_ms = the kernels'
        durations (length, scan, fill, deflate, pack)"""
        nm = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
        blob = np.frombuffer(b"".join(nm) + b"\0", np.uint8)
        name_off = np.concatenate([[0], np.cumsum([len(x) for x in nm])]).astype(np.uint32)
        contig = np.ascontiguousarray(contig, np.int32)
        pos = np.ascontiguousarray(pos, np.uint32)
        ref = np.frombuffer(ref_char.encode() if isinstance(ref_char, str) else bytes(ref_char), np.uint8) if not isinstance(ref_char, np.ndarray) else np.ascontiguousarray(ref_char).view(np.uint8)
        n = len(contig)
        if len(pos) != n or ref.size != n:
            raise ValueError("contig, pos and ref_char have one entry per column")
        indiv = getattr(self, "_rindiv", 0) or 512          # (samples of the last call)
        if gz_cap is None:
            text_cap = n * (14 + max([len(x) for x in nm] + [0]) + 4 * indiv)
            gz_cap = text_cap + 23 * (text_cap // PCG_PIECE + n + 1)
        if hole_cap is None:
            hole_cap = n
        gz = np.zeros(max(int(gz_cap), 1), np.uint8)
        site, at = np.zeros(max(int(hole_cap), 1), np.uint32), np.zeros(max(int(hole_cap), 1), np.uint64)
        n_gz, n_holes, n_text = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        ms = np.zeros(5, np.float32)
        if pin:
            self.pin_host(gz)
        try:
            rc = self.L.pecall_dev_sites_base_gz(self.h, _p(blob), _p(name_off), len(nm), _p(contig), _p(pos), _p(ref), _p(gz), int(gz_cap),
                                                 C.byref(n_gz), _p(site), _p(at), int(hole_cap), C.byref(n_holes), C.byref(n_text), _p(ms))
        finally:
            if pin:
                self.unpin_host(gz)
        self.gz_needed, self.holes_needed, self.text_needed, self.gz_ms = int(n_gz.value), int(n_holes.value), int(n_text.value), ms
        self._ck(rc)
        return gz[:n_gz.value].tobytes(), site[:n_holes.value], at[:n_holes.value]

    def pin_host(self, a):
        self._ck(self.L.pecall_dev_pin_host(self.h, a.ctypes.data, a.nbytes))

    def unpin_host(self, a):
        self._ck(self.L.pecall_dev_unpin_host(self.h, a.ctypes.data))

    @staticmethod
    def out_arrays(n_sites, indiv, posterior=True):
        """the six result arrays of call_sites, touched (np.zeros leaves the pages to the first write); posterior=False: a token
        array in its place (call_sites_sparse does not fill it)"""
        out = (np.zeros((n_sites, indiv), np.int8), np.zeros((n_sites, indiv) if posterior else (1, 1)), np.zeros(n_sites, np.int8), np.zeros((n_sites, ALLELES), np.int32),
               np.zeros(n_sites, np.int8), np.zeros(n_sites, np.int32))
        for a in out:
            a.fill(0)
        return out

    def call_sites_sparse(self, reads, ref_base, threshold=0.95, theta=0.001, haploid=False, chrom=None, cap=None, out=None, sparse_out=None):
        """call_sites with the posteriors as a list (pecall_dev_call_sites_sparse): -> call, (post_site [k] ascending, post_rows [k][indiv]),
        site_type, allele_count, n_pass; columns that are not listed have posterior 1 for every sample.  cap = rows the list may take
        (default: one per 8 columns, at least 1024); out / sparse_out: arrays to reuse (out as for call_sites, its posterior unused)"""
        reads = np.ascontiguousarray(reads, np.uint16)
        ref_base = np.ascontiguousarray(ref_base, np.uint8)
        n_sites, indiv = reads.shape[:2]
        cy = None if chrom is None else np.ascontiguousarray(chrom, np.uint8)
        call, _, typ, ac, npass, den = out if out is not None else self.out_arrays(n_sites, indiv, posterior=False)
        if sparse_out is not None:
            site, rows = sparse_out
            cap = len(site)
        else:
            cap = int(cap) if cap is not None else max(1024, n_sites // 8)
            site, rows = np.empty(cap, np.uint32), np.empty((cap, indiv), np.float64)
        n = C.c_uint64(0)
        self.denovo = den
        self.sparse_needed = 0
        self._rindiv = indiv
        rc = self.L.pecall_dev_call_sites_sparse(self.h, _p(reads), _p(ref_base), _p(cy), n_sites, indiv, int(haploid), float(threshold),
                                                 float(theta), _p(call), _p(site), _p(rows), cap, C.byref(n), _p(typ), _p(ac), _p(npass), _p(den))
        self.sparse_needed = int(n.value)
        self._ck(rc)
        return call, (site[:n.value], rows[:n.value]), typ, ac, npass

    def call_sites(self, reads, ref_base, threshold=0.95, theta=0.001, haploid=False, chrom=None, out=None):
        """the whole per-site caller (pecaller.c:1207-1691): reads [n_sites][indiv][6] u16, ref_base [n_sites] (0..3 = ACGT, else
        skipped), chrom [n_sites] 0 autosome / 1 X / 2 Y / 3 MT -> call [n_sites][indiv] (0..13, 14 = 'N'), posterior, site_type,
        allele_count, n_pass; self.denovo = d_count per site (with a pedigree).  out: the arrays of out_arrays(), reused by a
        caller that keeps (and may have pinned) its buffers"""
        reads = np.ascontiguousarray(reads, np.uint16)
        ref_base = np.ascontiguousarray(ref_base, np.uint8)
        n_sites, indiv = reads.shape[:2]
        cy = None if chrom is None else np.ascontiguousarray(chrom, np.uint8)
        call, post, typ, ac, npass, den = out if out is not None else self.out_arrays(n_sites, indiv)
        self.denovo = den
        self._rindiv = indiv
        self._ck(self.L.pecall_dev_call_sites(self.h, _p(reads), _p(ref_base), _p(cy), n_sites, indiv, int(haploid), float(threshold),
                                              float(theta), _p(call), _p(post), _p(typ), _p(ac), _p(npass), _p(den)))
        return call, post, typ, ac, npass
