/*
 * pemap_hip.h -- C-ABI of the MI355X (gfx950) PEMapper / PECaller hot path.
 *
 * Plain C: opaque handles, plain pointers and sizes, int return codes (0 = ok, non-zero = error; the text is in
 * pemap_dev_last_error()).  Nothing here depends on torch or on C++ types.  A host program written in C (the
 * reference's language) links libpemap_hip.so and calls these; pecaller_amd/csrc/pemapper_main.c does exactly that.
 *
 * What each entry replaces in the reference (wingolab-org/pecaller, paths under src/):
 *
 *   pemap_dev_create / _destroy      the process-wide globals of pemapper.c:140-176 (one object per GPU instead)
 *   pemap_dev_load_index             init_index_buffer + genome/.sdx load, pemapper.c:411-494, 2129-2155
 *   pemap_dev_build_index            index_genome_whole.c:93-354 (rolling 16-mer, N resets, len-15 coordinates), on device
 *   pemap_dev_set_params             argv parsing of max_dist/min_dist/is_bisulfite/min_match, pemapper.c:233-297
 *   pemap_dev_map_batch              pthread_create(..., map_everything, batch) + the result fold,
 *                                    pemapper.c:684, 759, 907-1309 (initial_map, find_matches, smith_waterman_align,
 *                                    find_mate_pairs, smith_waterman_backtrack)
 *   pemap_dev_submit_batch / _wait_batch  the same seam, asynchronous like the reference's (pthread_create returns at once, the
 *                                    batch mutex is released at pemapper.c:1307)
 *   pemap_dev_stage_reads/_run/_collect   the same call split in three, so that a caller can time the device part
 *   pemap_dev_fetch_pileup           the final genome walk that feeds the pileup / indel writers, pemapper.c:819-866
 *   pemap_dev_summary                total_reads/total_bases/total_dist/no_dists/mate_counts, pemapper.c:144-149, 1238-1265
 *   pemap_dev_index_share            nothing: the reference's threads share one index in host memory (pemapper.c:411-494); here every
 *                                    object (one per GPU) holds its own copy, made device to device from the object that loaded or built it
 *   pemap_dev_absorb                 the reference's ONE all_base_list that every thread increments (pemapper.c:53-58, 156) and its one
 *                                    set of totals: the objects' counters, insertion lists and summaries summed into one of them
 *   pecall_dev_*                     fill_sample_like and its callers, pecaller.c:2448-2507 (see below)
 *
 * Threading: calls on different pemap_dev objects may run concurrently from different host threads; calls on one
 * object must be serialised by the caller (the reference serialises a batch behind its own mutex, pemapper.c:661),
 * except pemap_dev_submit_batch / _wait_batch / _map_batch, which several host threads may call on one object.
 * pemap_dev_index_share and pemap_dev_absorb are calls on BOTH their objects, with one relaxation: index_share only reads its
 * source, so several index_share calls from one source to different destinations may run side by side.  Calls on disjoint
 * pairs of objects may run concurrently.
 * Ownership: the caller owns every host buffer and may reuse it as soon as a call returns; the object owns all
 * device memory.
 */
#ifndef PEMAP_HIP_H
#define PEMAP_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PEMAP_MAX_HITS   200    /* max_hits, pemapper.c:162 */
#define PEMAP_MIN_READ   16     /* one full 16-mer segment (pemapper.c:1573-1587 reads garbage below this) */
#define PEMAP_MAX_READ   278    /* L + 21 window rows must fit the reference's 300 x 300 matrices (pemapper.c:155, 932-956) */

/* mapping_type values, pemapper.c:37-45 */
enum
{
  PEMAP_UNIQUE_MATE = 0, PEMAP_UNIQUE_SLIP = 1, PEMAP_UNIQUE_SINGLE = 2, PEMAP_UNIQUE_MIS = 3, PEMAP_NON_MATE = 4,
  PEMAP_NON_MIS = 5, PEMAP_FRAG_MIS = 6, PEMAP_NON_NO = 7, PEMAP_NEITHER_MAP = 8
};

typedef struct pemap_dev pemap_dev;

/* insertion callback for pemap_dev_fetch_pileup: pos = 0-based index into .seq, seq = inserted bases in read order */
typedef void (*pemap_ins_cb) (void *user, uint32_t pos, const char *seq, int len);

const char *pemap_dev_last_error (const pemap_dev * dev);       /* dev may be NULL: error of the last failed create */

int pemap_dev_create (pemap_dev ** out, int device_id);
void pemap_dev_destroy (pemap_dev * dev);

/* Index from the reference's on-disk arrays already in host memory.  pos_index has 2^32 + 1 entries (.idx inflated),
 * mers has n_mers entries (.mdx), genome is the upper-cased .seq stream, contig_starts has n_contigs + 1 entries:
 * prefix sums of the .sdx "len-15" column (pemapper.c:434-448).  idepth is the last .sdx line (16). */
int pemap_dev_load_index (pemap_dev * dev, const uint32_t * pos_index, const uint32_t * mers, uint64_t n_mers,
                          const char *genome, uint64_t genome_size, const uint32_t * contig_starts, int n_contigs,
                          int idepth);

/* Index built on the device from the concatenated genome letters (what .seq holds) and the contig lengths
 * (full lengths, not len-15).  Produces exactly the arrays the reference builder writes.  bisulfite = the builder's
 * "bisulfite converted" answer (C indexed as T, index_genome_whole.c:174-177). */
int pemap_dev_build_index (pemap_dev * dev, const char *genome, uint64_t genome_size, const uint32_t * contig_len,
                           int n_contigs, int bisulfite);

/* Same, from letters already in device memory (d_genome is a device pointer; the object takes a copy). */
int pemap_dev_build_index_resident (pemap_dev * dev, const void *d_genome, uint64_t genome_size,
                                    const uint32_t * contig_len, int n_contigs, int bisulfite);

/* Multi-GPU replica set-up: allocate empty index arrays of the given sizes so that a collective (RCCL broadcast
 * from the rank that loaded or built the index) can fill them, then pemap_dev_index_commit(). */
int pemap_dev_index_alloc (pemap_dev * dev, uint64_t n_mers, uint64_t genome_size, int n_contigs, int idepth);
int pemap_dev_index_commit (pemap_dev * dev);

/* Several objects in one process (one per GPU, or several on one GPU as a rehearsal): dst receives a copy of src's committed
 * index -- pemap_dev_index_alloc with src's sizes, buffers 0..3 (pemap_dev_buffer) copied device to device on dst's stream in
 * pieces of at most 1 GiB (hipMemcpyPeerAsync: no peer access needs enabling; a plain device copy when both sit on one GPU), then
 * pemap_dev_index_commit, so dst builds its look-up replicas or not by its own setting.  src is only read.  Fails when src has no
 * committed index or dst == src. */
int pemap_dev_index_share (pemap_dev * dst, pemap_dev * src);

/* Look-up replicas -- an MI355X-side layout with no counterpart in the reference.  The look-ups of a read-end
 * (2 x segments x 49 buckets, fill_mers / get_mers, pemapper.c:1969-2003, 2158-2165) cost one 64-byte HBM request each
 * in the reference's table; index_commit therefore also builds 8 re-ordered copies of the table (128 GiB + the records
 * of the multi-position buckets) in which a k-mer and its 48 neighbours share 8 lines.  Results are identical either
 * way.  n = -1: build them when the device has the memory (default; PEMAP_REPLICAS=0/1 in the environment overrides),
 * 0: never, 8: fail if they cannot be built.  May be called before or after the index is in place. */
int pemap_dev_set_lookup_replicas (pemap_dev * dev, int n);
/* how many replicas serve the look-ups now (0 or 8), and the bytes of the multi-position records */
int pemap_dev_lookup_replicas (pemap_dev * dev, int *n_replicas, uint64_t * record_bytes);
/* The last launch of the fused seed kernel's first tier (host only, zeros before the first run): persistent one-wave workgroups
 * per CU asked for (PEMAP_LOOKUP_WAVES or its default), how many the runtime keeps resident on a CU for the launched form with its
 * dynamic LDS (hipOccupancyMaxActiveBlocksPerMultiprocessor), how many were launched (the smaller of the two, at most four per
 * SIMD's register bound) and the LDS bytes of one. */
int pemap_dev_seed_launch (pemap_dev * dev, int *asked, int *resident, int *launched, int *lds_bytes);

/* Device pointers and sizes of the resident arrays: which = 0 pos_index (u32[2^32+1]), 1 mers (u32[n_mers]),
 * 2 genome (u8[genome_size]), 3 contig_starts (u32[n_contigs+1]), 4 pileup counters (six planes A C G T Del Ins of 16-bit
 * wrapping counters, two positions to a 32-bit word, each plane padded to 256-byte blocks: n_bytes / 6 bytes per plane),
 * 5 the look-up replicas (u32[8][2^32]; replica p holds the entry of k-mer k at k with its 4-bit fields 0 and p
 * swapped), 6 the records of the multi-position buckets (16-byte units {count, positions...}); 5 and 6 are empty
 * (n_bytes = 0) when no replicas are in use.
 * For collectives (broadcast of 0..3 at start-up, sum of 4 at the end) and for copying the index back to the host.
 * Buffer 4 while the object maps: its first plane then holds differences of neighbouring counters, not counts (two atomics per
 * run of matched bases instead of one per word), and is turned back into counts -- a scan over the plane, waited for -- by
 * pemap_dev_buffer (which = 4) and pemap_dev_read_buffer through it, pemap_dev_fetch_pileup, pemap_dev_fetch_records (and _gz),
 * pemap_dev_absorb (both objects) and pemap_dev_map_batch before it returns; NOT by pemap_dev_run, pemap_dev_run_slice,
 * pemap_dev_sync, pemap_dev_submit_batch or pemap_dev_wait_batch.  So the view of buffer 4 holds counts when it is obtained, and
 * again after every pemap_dev_map_batch; a view kept across asynchronous runs (run / run_slice / submit_batch) must be obtained
 * again before it is read.  A caller may write counts into the view while nothing is in flight and the view holds counts. */
int pemap_dev_buffer (pemap_dev * dev, int which, void **d_ptr, uint64_t * n_bytes);
int pemap_dev_index_info (pemap_dev * dev, uint64_t * n_mers, uint64_t * genome_size, int *n_contigs, int *idepth);
/* copy one of the buffers above (or a byte range of it) to host memory */
int pemap_dev_read_buffer (pemap_dev * dev, int which, uint64_t byte_offset, void *host_dst, uint64_t n_bytes);

/* The parameters of the batches submitted from here on.  A call that changes a value while a batch is in flight or a run is pending
 * first delivers every batch (as pemap_dev_wait_batch would, oldest first) and accounts the run, under the values they were
 * submitted with: the later pemap_dev_wait_batch of such a batch returns 0 and finds it delivered.  It takes the locks of
 * submit / wait, so it may be called beside them.  A call that changes nothing does nothing. */
int pemap_dev_set_params (pemap_dev * dev, int paired, int min_dist, int max_dist, double min_align, int bisulfite);

/* One batch.  reads are `stride`-spaced byte rows (not necessarily NUL terminated), len1/len2 their lengths,
 * PEMAP_MIN_READ <= len <= PEMAP_MAX_READ, reads2/len2/m2 NULL in single-end mode.  m1/m2 receive
 * 0 (unmapped) or the reference's coordinate (0-based index of the last aligned reference base, + 2),
 * mapping_type the class.  The pileup and the summary counters accumulate on the object. */
int pemap_dev_map_batch (pemap_dev * dev, const char *reads1, const int *len1, const char *reads2, const int *len2,
                         int n, int stride, uint32_t * m1, uint32_t * m2, int *mapping_type);

/* The same call split at the point where the reference's reader thread lets go of a batch: pthread_create (pemapper.c:684)
 * returns at once and the batch's mutex is released when the worker is done (1307).  submit queues the batch (host-to-device
 * copies on a copy stream, kernels on the object's pipeline, device-to-host copy of the results) and returns a ticket; wait
 * blocks until that batch's m1 / m2 / mapping_type are in the buffers given to submit and its summary counters are folded.
 * Up to 3 batches are in flight per object; a 4th submit first delivers the oldest.  With at least 2 in flight the copies hide
 * under the kernels and the kernel pipeline never drains between batches: the host sees the device-resident rate.
 * The caller's buffers (reads, lengths, results) belong to the library from submit until the batch is delivered.
 * submit / wait / map_batch may be called from several host threads on one object (they serialise on an internal lock
 * that is released while a thread blocks in wait); everything else on the object still needs the caller's serialisation.
 * pemap_dev_map_batch == submit + wait. */
int pemap_dev_submit_batch (pemap_dev * dev, const char *reads1, const int *len1, const char *reads2, const int *len2,
                            int n, int stride, uint32_t * m1, uint32_t * m2, int *mapping_type, uint64_t * ticket);
int pemap_dev_wait_batch (pemap_dev * dev, uint64_t ticket);
/* Optional: page-lock a host range that read rows will be submitted from, so that they move by DMA straight out of it (the
 * reference allocates its batch buffers once, pd_node_alloc at pemapper.c:2340-2372, and reuses them: pin them once after
 * that, unpin before freeing them).  Rows submitted from memory that is not pinned are first copied into a pinned staging
 * buffer of the library (a few host threads, ~10 ms per million pairs).  The library never page-locks caller memory by itself. */
int pemap_dev_pin_host (pemap_dev * dev, const void *host_ptr, uint64_t n_bytes);
int pemap_dev_unpin_host (pemap_dev * dev, const void *host_ptr);

/* The same in three steps.  stage: host -> device copy of a batch; run: the kernels (asynchronous on the object's
 * stream unless sync != 0); collect: device -> host copy of the results + summary fold.  After stage, run may be
 * called repeatedly (each run maps the staged batch again and adds to the pileup): that is what bench.py times. */
int pemap_dev_stage_reads (pemap_dev * dev, const char *reads1, const int *len1, const char *reads2, const int *len2,
                           int n, int stride);
int pemap_dev_run (pemap_dev * dev, int sync);
/* map only rows [first, first + n) of the staged reads (one bench "step" = one slice of a resident read set) */
int pemap_dev_run_slice (pemap_dev * dev, int first, int n, int sync);
int pemap_dev_collect (pemap_dev * dev, uint32_t * m1, uint32_t * m2, int *mapping_type);
int pemap_dev_sync (pemap_dev * dev);

/* Synthetic workload, generated on the device (bench and scale tests): a seeded genome of
 * n_contigs contigs (repeat families, N runs at contig ends), and a staged batch of n read pairs of length read_len
 * sampled from the resident genome with substitutions/indels.  synth_genome fills contig_len[n_contigs]. */
int pemap_dev_synth_genome (pemap_dev * dev, uint64_t seed, uint64_t genome_size, int n_contigs, double repeat_frac,
                            void **d_genome, uint32_t * contig_len);
int pemap_dev_synth_reads (pemap_dev * dev, uint64_t seed, int n, int read_len, int paired, double sub_rate,
                           double indel_rate, uint64_t first_read);
/* the same with ONE insertion or deletion of 1..10 bases in the given share of the read-ends instead of a per-base indel rate
 * (BASELINE config "5 % indel-enriched 2x250bp reads") */
int pemap_dev_synth_reads_indel (pemap_dev * dev, uint64_t seed, int n, int read_len, int paired, double sub_rate,
                                 double indel_read_frac, uint64_t first_read);
/* copy the staged batch back (for the CPU baseline): reads as stride-spaced rows */
int pemap_dev_staged_reads (pemap_dev * dev, char *reads1, int *len1, char *reads2, int *len2, int stride);
int pemap_dev_staged_info (pemap_dev * dev, int *n, int *stride, int *paired);
/* release a device allocation handed out by pemap_dev_synth_genome */
int pemap_dev_free (pemap_dev * dev, void *d_ptr);

/* ---- read rows made on the device from fastq text ----
 * What the host program otherwise does before pemap_dev_submit_batch: fill_rows of pemapper_main.c, which follows the reference's read
 * loop (pemapper.c:649-748 with the trims of pemapper_tsw.c:693-704) -- a search for every line's end and a copy of every sequence.
 * The rule is pecaller_amd/csrc/pemap_fastq_rule.h (the kernels: pemap_fastq.hip.h).  A line is a run of bytes ended by '\n' ('\r' is
 * part of it); bytes behind a text's last '\n' are not looked at.  The first line of a stream is skipped, the next is the first
 * record's sequence; behind a sequence two lines are skipped whatever they hold, then lines up to and including one that begins
 * with '@', and the line behind that is the next sequence.
 *   text1/bytes1, text2/bytes2   one piece of each mate file's text, at most 2^30 bytes each; text2 = NULL, 0, 0 in single-end mode
 *   state1, state2               0: the piece is the beginning of its stream; 1: it begins behind a sequence line
 *   trim_start, trim_end         bases dropped from either end of every read, as fill_rows does it
 *   max_records                  records examined per mate at most (the batch's size)
 *   stride                       of the rows, PEMAP_MAX_READ at least
 *   res->got[m]                  records of mate m that count: those in front of the first one that stops the mate
 *   res->end[m]                  0 got == max_records; 1 the text ran out of complete records; 2 (first mate only) a read of 12 bases
 *                                or fewer; 3 a read shorter than PEMAP_MIN_READ or longer than PEMAP_MAX_READ, its length in bad_len[m]
 *   res->n                       pairs in the batch: min (got[0], got[1]); got[0] in single-end mode
 *   res->consumed[m]             offset just behind the '\n' of mate m's n-th sequence line (0 when n == 0): the caller puts the
 *                                bytes from there on in front of the next piece and passes state 1 (n == 0: the state it passed)
 * An end of 2 or 3 is a result, not an error; n == 0 is success, nothing is staged or queued and *ticket is not written.  Non-zero is
 * returned for bad arguments (a NULL pointer, paired mode without text2, stride < PEMAP_MAX_READ, max_records <= 0, a state other
 * than 0 or 1, a negative trim, a text of more than 2^30 bytes) and for HIP errors.
 * pemap_dev_stage_fastq is pemap_dev_stage_reads with the rows made on the device: it leaves the object as stage_reads would for the
 * same rows (the lengths come back to the host, 4 bytes a read), so pemap_dev_run / _run_slice / _collect / _staged_reads /
 * _staged_info follow unchanged.
 * pemap_dev_submit_fastq is pemap_dev_submit_batch with the same substitution, under the same threading rules: the text goes up on the
 * copy stream (by DMA straight out of a range pinned with pemap_dev_pin_host), the parse kernels run there in front of the event the
 * pipeline waits for, and the call waits only for their control blocks and the lengths while the batches in flight keep the device
 * busy.  It returns with res filled and batch n queued; m1 / m2 / mapping_type need room for max_records entries.  The result arrays
 * belong to the library until the batch is delivered; the texts may be reused when the call returns. */
typedef struct
{
  int32_t n, got[2], end[2], bad_len[2];
  uint64_t consumed[2];
} pemap_fastq_result;
int pemap_dev_stage_fastq (pemap_dev * dev, const char *text1, uint64_t bytes1, int state1, const char *text2, uint64_t bytes2, int state2,
                           int trim_start, int trim_end, int max_records, int stride, pemap_fastq_result * res);
int pemap_dev_submit_fastq (pemap_dev * dev, const char *text1, uint64_t bytes1, int state1, const char *text2, uint64_t bytes2, int state2,
                            int trim_start, int trim_end, int max_records, int stride, uint32_t * m1, uint32_t * m2, int *mapping_type,
                            pemap_fastq_result * res, uint64_t * ticket);

/* counts[genome_size][6] u16 (A,C,G,T,Del,Ins), wrapping as the reference's unsigned short counters do
 * (pemapper.c:53-58); cb (may be NULL) is called once per logged insertion, in unspecified order. */
int pemap_dev_fetch_pileup (pemap_dev * dev, uint16_t * counts, pemap_ins_cb cb, void *user);
/* compacted 16-byte records {u32 pos; u16 A,C,G,T,Del,Ins} of the non-zero sites in [first, first+count), ascending;
 * returns the number of records through n_records (out may be NULL to count only). */
int pemap_dev_fetch_records (pemap_dev * dev, uint64_t first, uint64_t count, void *out, uint64_t out_capacity,
                             uint64_t * n_records);
/* pemap_dev_fetch_records with the records deflated on the device: the records of [first, first + count) are cut into pieces of 512
 * and every piece becomes one BGZF member (a complete gzip member of under 65,536 bytes whose head says how long it is; the rule is
 * pecaller_amd/csrc/pemap_gz_rule.h, tests/csrc/pemap_gz_rule_check.c states it serially).  gz_out receives the members back to back,
 * *gz_bytes their length: they inflate to exactly the bytes pemap_dev_fetch_records returns for the range.  A file made of the
 * members of consecutive ranges and the 28-byte empty member (pmz_eof_byte) is a BGZF file.  ins_records (may be NULL) receives the
 * 16-byte records whose insertion count is not 0, ascending, *n_ins their number.  The range is checked and plane 0 folded as by
 * pemap_dev_fetch_records.  With gz_out == NULL the call returns the three sizes only.  A gz_capacity (bytes) or an ins_capacity
 * (records) that is too small fails with a message that names what is needed, and nothing is written to either buffer.  The members
 * are copied straight into gz_out where the caller pinned it (pemap_dev_pin_host), else through page-locked blocks of the object. */
int pemap_dev_fetch_records_gz (pemap_dev * dev, uint64_t first, uint64_t count, void *gz_out, uint64_t gz_capacity, uint64_t * gz_bytes,
                                uint64_t * n_records, void *ins_records, uint64_t ins_capacity, uint64_t * n_ins);
/* kernel milliseconds of the last pemap_dev_fetch_records_gz: the records (count, scan, emit), the insertion list, the deflate, the scan
 * over the members' lengths and the pack */
int pemap_dev_fetch_gz_ms (pemap_dev * dev, float *ms4);
/* Counters, insertion log and summary start over.  Fails, changing nothing, while a submitted batch was not waited for. */
int pemap_dev_reset_pileup (pemap_dev * dev);
/* The end of a run on several objects: afterwards dst is what it would be had it mapped src's batches as well, and src is as
 * after pemap_dev_reset_pileup.  Every 16-bit counter of buffer 4 becomes (dst + src) mod 2^16 -- the arithmetic of the reference's
 * one shared unsigned short array -- on the device (pm_pile_add_kernel); src's insertion log is appended to dst's; the 13 summary
 * numbers are added.  Both objects on one device: the kernel reads src's planes in place.  Different devices (or
 * PEMAP_ABSORB_STAGED=1): src's planes arrive in pieces of PEMAP_ABSORB_CHUNK KiB (default 262144) in two staging buffers on
 * dst's device, the copy of a piece under the add of the piece before.
 * Fails, changing nothing, when dst == src, when either object has no index, when the two hold genomes of different size, contig
 * count or plane size, or when either has a submitted batch that was not waited for. */
int pemap_dev_absorb (pemap_dev * dst, pemap_dev * src);

/* out13: total_reads, total_bases, total_dist, no_dists, mate_counts[0..8] */
int pemap_dev_summary (pemap_dev * dev, long *out13);

/* Persistent waves of a launch of the full DP (CUs x PEMAP_SW_WAVES_PER_CU), each of which works on 64 / lanes-per-alignment problems
 * at a time.  Without PEMAP_BAND_GATE a chunk of no more read-ends than one pass of this grid takes problems is routed by x <= 6 alone. */
int pemap_dev_sw_grid (pemap_dev * dev);

/* The full DP's lane geometry for a batch whose longest read has read_len bases, as this object's knobs (read when it was made)
 * choose it: *lanes lanes share one alignment, each owns *columns read columns; lanes x columns >= read_len.  8 x 13 up to 104 bases,
 * 16 x 10 / 13 / 16 / 19 up to 160 / 208 / 256 / 278, and with PEMAP_GAPLESS=0 8 x 19 for 105..152.  Host code only; an error for a
 * length outside PEMAP_MIN_READ .. PEMAP_MAX_READ. */
int pemap_dev_sw_geom (pemap_dev * dev, int read_len, int *lanes, int *columns);

/* Which way the host pipeline went, counted since the object was made (host integers only: nothing is synchronised, absorbed or
 * launched, unlike pemap_dev_run_stats, which accounts the pending run first).  A run is one pemap_dev_run / _run_slice or the kernels
 * of one submitted batch; it is cut into chunks, and a run queued behind a pending one continues its chunk numbering (and its event
 * chain) unless the pending runs have to be waited for and accounted ("absorbed") first.  out8:
 *   [0] runs queued                      [1] of them, runs that continued a pending pipeline (first chunk number > 0)
 *   [2] absorbs because the table of 256 chunks was full
 *   [3] absorbs because the longest read (the kernels' geometry) changed
 *   [4] absorbs because the pending runs' arrays are too small for the new chunk, or PEMAP_PIPELINE is 2
 *   [5] set-ups of the ring of batches in flight (the first submit, another stride or pairing, a batch beyond its capacity)
 *   [6] chunks of the run queued last    [7] its first chunk's number */
int pemap_dev_pipeline_stats (pemap_dev * dev, uint64_t * out8);

/* Counters the reference does not have, summed over the last run --
 * stats[0] = read-ends, [1] = positions gathered from .mdx (P), [2] = SW problems scored (H), [3] = SW problems
 * scored with direction nibbles (single-hit ends + re-scored winners), [4] = DP cells without nibbles, [5] = DP cells
 * with nibbles, [6] = pileup increments, [7] = insertions logged, [8] = alignments walked back, [9] = winners re-scored,
 * [10] = read-ends the fused seed kernel's first tier passed over (more positions than its list holds, or too many next to candidate
 *        anchors): taken by its second tier; [15] = of them, the ones left to the monolithic seed kernel,
 * [11] = chunks the run was cut into (= launches of every kernel),
 * [12] = problems decided without the DP (a diagonal with at most one mismatch; with PEMAP_GAPLESS=0 none):
 *        [3], [5] count the DP's share only.
 * [13] = problems scored by the DP restricted to a band of 32 diagonals (exact for them: pemap_band.hip.h), part of [2] and,
 *        for the single-hit ends, of [3]; [14] = band cells computed (not part of [4], [5]).
 * [16] = of [8], the alignments whose traceback was followed cell by cell; the others are known to be plain diagonals (decided
 *        without the DP, or banded with a traceback that never leaves the start cell's diagonal) and go to the pileup as such.
 * [17] = of [13], the problems without a diagonal of at most 6 mismatches that two diagonals and one gap admit to the band
 *        (PEMAP_BAND_GATE: 1 in every chunk, 0 in none -- they are scored by the full DP as before; unset, in the chunks that hold
 *        more read-ends than one pass of the full DP's grid takes problems, see pemap_dev_sw_grid).
 * times_ms[0..7] = seed stage (look-up + vote), SW single-hit (with nibbles), SW multi-hit, select, SW re-score,
 * walk+pileup, look-up kernel alone, vote kernel alone (the list-mode remainder of the big read-ends and the emit kernel count
 * towards [0] only): kernel durations from HIP events on the object's streams, summed over the run's chunks (the streams of
 * the pipeline overlap in time, so their sum exceeds the wall time). */
int pemap_dev_run_stats (pemap_dev * dev, uint64_t * stats18, float *times_ms8);

/* Debug/parity taps: per read-end hit lists and per-hit SW results of the last run.
 * n_hits[n_ends]; the other arrays are [n_ends][PEMAP_MAX_HITS]. Any pointer may be NULL. end = 2*pair + mate in paired mode. */
int pemap_dev_debug_hits (pemap_dev * dev, int *n_hits, uint32_t * spot, uint8_t * orient, uint32_t * win_start,
                          int *win_len, double *score, int *start_k, int *start_i);

/* ---- PECaller: per-(site, sample) Dirichlet-multinomial genotype log-likelihood ----
 * fill_sample_like (pecaller.c:2448-2507) together with the per-sample set-up it depends on (pecaller.c:1230-1260:
 * tot = A+C+G+T+Del, coef = ln tot! - sum ln reads[i]! over all six counts).
 *   reads[n_sites][indiv][6] u16        one pileup column per sample, the 6 counters of the pileup record
 *   alpha_mean[n_sites][14][6] f64      d_alpha_mean of the pass (pecaller.c:1354-1364)
 *   max_gen / min_depth                 14 / 2 diploid, as set at pecaller.c:326-336 for haploid
 *   norm                                new_norm[pass] (pecaller.c:1339-1344)
 *   like[n_sites][indiv][14]            log-likelihoods (0 where the reference skips the sample: tot <= min_depth)
 *   best[n_sites][indiv]  (may be NULL) initial_call, 14 where skipped;  margin (may be NULL) initial_p
 * The confidence ordering (qsort at 2506) and the configuration search stay on the host. */
typedef struct pecall_dev pecall_dev;
int pecall_dev_create (pecall_dev ** out, int device_id);
void pecall_dev_destroy (pecall_dev * dev);
const char *pecall_dev_last_error (const pecall_dev * dev);
int pecall_dev_site_like (pecall_dev * dev, const uint16_t * reads, const double *alpha_mean, int n_sites, int indiv,
                          int max_gen, int min_depth, double norm, double *like, int8_t * best, double *margin);
/* the same call in three steps (host->device, kernel, device->host), so that the kernel can be timed on resident data */
int pecall_dev_stage (pecall_dev * dev, const uint16_t * reads, const double *alpha_mean, int n_sites, int indiv);
int pecall_dev_run (pecall_dev * dev, int n_sites, int indiv, int max_gen, int min_depth, double norm, int sync);
int pecall_dev_collect (pecall_dev * dev, int n_sites, int indiv, double *like, int8_t * best, double *margin);

/* ---- PECaller: the whole per-site caller ----
 * The body of call_single_base for one pileup column (pecaller.c:1207-1691), with or without a pedigree: site filters,
 * up to five passes of { Dirichlet means, fill_sample_like, confidence order, the beam over joint configurations
 * (fill_config_like / fill_config_probs / clean_config_probs with the exact Hardy-Weinberg prior), configuration
 * posteriors, per-sample marginal posteriors and calls, moment-matched alpha re-estimation + check_alpha_sanity }, then the
 * site classification of pecaller.c:1565-1636.
 *   reads[n_sites][indiv][6] u16     as above, samples in the reference's column order (it matters: ties, beam order)
 *   ref_base[n_sites]                0..3 = A C G T (gen_to_int of the .seq letter); anything else = a site the reference
 *                                    skips (pecaller.c:1208, 1718): calls 'N', posterior 1, site_type -1
 *   chrom_type[n_sites] (may be NULL) 0 autosome, 1 chrX, 2 chrY, 3 chrMT: the lower-cased contig-name prefix rule of
 *                                    pecaller.c:474-482 (chrY lifts the half-the-samples filter, 1303; X/Y/MT change add_denovo);
 *                                    + 16 = HAPLOID forced for the column, as the BED guide mode does on chrY / chrMT (955-957)
 *   haploid / threshold / theta      argv[7] / argv[5] (Prob_to_call) / argv[6] of pecaller
 *   call[n_sites][indiv]             0..13 = A C G T D I M R W S Y K E H (int_to_gen), 14 = 'N'
 *   posterior[n_sites][indiv]        final_p, what the reference prints with %g
 *   site_type[n_sites]  (may be NULL) 0 reference, 1 SNP, 2 DEL, 3 INS, 4 LOW, 5 MULTIALLELIC, 6 MESS
 *   allele_count[n_sites][6], n_pass[n_sites]  (may be NULL) Allele_Counts of the .snp row; passes run
 *   denovo[n_sites]     (may be NULL) d_count of the row (pecaller.c:1650-1671): > 0 = the type is printed as DENOVO_<type>
 * indiv <= 512: up to 64 samples one lane per sample (the fast case: shortcut kernel + beam search of the columns it lists);
 * 65..512 a lane stands for a sample of each chunk of 64 -- the shortcut kernel holds two chunks in registers (up to 128 samples) or works a
 * chunk at a time; the beam search of the columns it lists runs one wave per CU from 257 samples on.  Text formatting and
 * the merge of the pileup streams stay on the host.
 * The columns travel in chunks of 2^18 (PECALL_CHUNK_LOG2): the host-to-device copy of chunk k + 1, the kernels of chunk k and the
 * device-to-host copy of chunk k - 1 run side by side.  Arrays the caller page-locked with pecall_dev_pin_host are copied from and
 * to directly; the others pass through pinned staging buffers of the object (host copies on a few threads). */
int pecall_dev_call_sites (pecall_dev * dev, const uint16_t * reads, const uint8_t * ref_base, const uint8_t * chrom_type, long n_sites,
                           int indiv, int haploid, double threshold, double theta, int8_t * call, double *posterior,
                           int8_t * site_type, int32_t * allele_count, int8_t * n_pass, int32_t * denovo);
/* The same call with the posteriors as a list: nearly every column of real data has posterior 1 for every sample (the shortcut of
 * the pass loop), and of the 606 bytes a 64-sample column sends back 512 are these doubles -- at the rate of the PCIe link they are
 * what the call takes.  Here only the columns in which SOME posterior differs from 1 come back: post_site[k] = the column's number
 * (ascending), post_rows[k][indiv] = its samples' posteriors; every column that is not listed has posterior exactly 1 for every
 * sample.  post_cap = rows the two arrays hold; *n_post = columns listed.  More columns than post_cap: the call fails (its message
 * says so) with *n_post = the number needed; nothing else of the results is to be used then.  The other arrays are as above. */
int pecall_dev_call_sites_sparse (pecall_dev * dev, const uint16_t * reads, const uint8_t * ref_base, const uint8_t * chrom_type, long n_sites,
                                  int indiv, int haploid, double threshold, double theta, int8_t * call, uint32_t * post_site,
                                  double *post_rows, uint64_t post_cap, uint64_t * n_post, int8_t * site_type, int32_t * allele_count,
                                  int8_t * n_pass, int32_t * denovo);
/* Page-lock a host range the caller will hand to pecall_dev_call_sites again and again (its tile buffers): the same table of
 * ranges as pemap_dev_pin_host's; a range stays until its last unpin.  Unpin before freeing the memory. */
int pecall_dev_pin_host (pecall_dev * dev, const void *host_ptr, uint64_t n_bytes);
int pecall_dev_unpin_host (pecall_dev * dev, const void *host_ptr);
/* the same call in three steps (host->device, kernel, device->host): bench.py times the kernel on resident columns with them.
 * kernel_ms (may be NULL) receives the kernel's duration from HIP events on the object's stream. */
int pecall_dev_sites_stage (pecall_dev * dev, const uint16_t * reads, const uint8_t * ref_base, const uint8_t * chrom_type, long n_sites,
                            int indiv);
int pecall_dev_sites_run (pecall_dev * dev, int haploid, double threshold, double theta, float *kernel_ms);
int pecall_dev_sites_collect (pecall_dev * dev, int8_t * call, double *posterior, int8_t * site_type, int32_t * allele_count,
                              int8_t * n_pass, int32_t * denovo);
/* How the last pecall_dev_sites_run divided its columns among the kernels (what PECALL_LIST_STATS prints), valid from that run until
 * something new is staged or called.  out[10]:
 *   [0]     columns run
 *   [1..4]  columns the shortcut kernels left to the beam search, by unsettled samples < 3 / < 8 / < 20 / more (beyond 128 samples a
 *           column too deep for the head of the ln n! table counts under "more"); where a chunk had a second pass with the whole
 *           table, what both passes listed
 *   [5]     columns on the deep list (up to 128 samples: a sample of 1,447 reads or more; they get the second pass)
 *   [6..9]  columns whose beam search was started ahead of the shortcut kernels (PECALL_HEAVY_MIN), by samples with variant reads
 *           < 12 / < 20 / < 32 / more; these are in none of [1..5] */
int pecall_dev_sites_stats (pecall_dev * dev, uint64_t * out);
/* ---- PECaller: pileup columns made on the device from the samples' record streams ----
 * What the host otherwise does before pecall_dev_call_sites: the k-way merge of the pileup streams (find_lowest and the dispatcher's
 * per-column loop, pecaller.c:865-923, 1820-1833).  A record is the pileup file's own 16 bytes, little-endian:
 * {u32 pos; u16 A,C,G,T,Del,Ins} -- what pemapper_hip writes and pemap_dev_fetch_records returns.
 * pecall_dev_sites_stage_records takes every sample's records of the positions [p0, p0 + span) and leaves the columns staged as
 * pecall_dev_sites_stage does (pecall_dev_sites_run / _collect follow unchanged):
 *   recs[indiv], n_recs[indiv]        host arrays of records, one per sample (NULL where n_recs is 0); ranges page-locked with
 *                                     pecall_dev_pin_host are copied from directly, others through the object's staging buffer.
 *                                     Each sample's positions ascend strictly and lie in [p0, p0 + span).
 *   ref_letters[ref_len <= span]      the .seq letters of the range from p0 on: a column's reference byte is its letter's index in
 *                                     "ACGTDIMRWSYKEHN" (gen_to_int, pecaller.c:2869-2907), 255 for any other byte and for
 *                                     positions at or beyond ref_len (the caller skips such columns: anything above 3)
 *   chrom_by_slot[span] (may be NULL) the chromosome class of every position of the range (chrom_type above); NULL: 0
 *   *n_cols                           columns made: a position is a column if and only if some sample has a record there (all six
 *                                     counts zero or not); a sample without a record there has six zeros.  Ascending positions.
 *   col_slot[span] (may be NULL)      position - p0 of each of the n_cols columns
 * Limits: 1 <= indiv <= 512, 1 <= span <= 2^22.  Returns 0; PECALL_RC_UNORDERED when a stream does not ascend strictly or leaves
 * the range (no other path returns that value; the error text names the lowest such sample and its record's index; nothing is
 * staged); another non-zero value for bad arguments.  No records at all: 0, *n_cols = 0, nothing staged. */
#define PECALL_RC_UNORDERED 3
int pecall_dev_sites_stage_records (pecall_dev * dev, const void *const *recs, const uint64_t * n_recs, int indiv, uint32_t p0, uint32_t span,
                                    const char *ref_letters, uint32_t ref_len, const uint8_t * chrom_by_slot /* may be NULL */ ,
                                    long *n_cols, uint32_t * col_slot /* [span], may be NULL */ );
/* The staged columns back on the host -- the result of the merge above (merge_columns' reads[n][indiv][6], reference and chromosome
 * bytes; in the reference the columns of pecaller.c:865-923): columns cols[0 .. n) (NULL: columns 0 .. n - 1) through a gather
 * kernel and one device-to-host copy (per 64 MB).  Any output may be NULL.  Valid for whatever is staged, until the next stage or call. */
int pecall_dev_sites_gather (pecall_dev * dev, const uint32_t * cols /* NULL: columns 0..n-1 */ , uint64_t n,
                             uint16_t * reads_out, uint8_t * ref_base_out, uint8_t * chrom_out /* any may be NULL */ );
/* Kernel durations of the last pecall_dev_sites_stage_records in ms (HIP events): mark, scan, tile. */
int pecall_dev_sites_merge_ms (pecall_dev * dev, float *ms3);
/* The one-call form (the merge of pecaller.c:865-923, 1820-1833 and call_single_base behind it): pecall_dev_sites_stage_records,
 * then the chunk pipeline of pecall_dev_call_sites_sparse over the resident columns, without its host-to-device copies.  The result
 * arrays are sized by the caller for span columns and filled for *n_cols; post_cap too small: as pecall_dev_call_sites_sparse. */
int pecall_dev_call_records (pecall_dev * dev, const void *const *recs, const uint64_t * n_recs, int indiv, uint32_t p0, uint32_t span,
                             const char *ref_letters, uint32_t ref_len, const uint8_t * chrom_by_slot, long *n_cols, uint32_t * col_slot,
                             int haploid, double threshold, double theta, int8_t * call, uint32_t * post_site, double *post_rows,
                             uint64_t post_cap, uint64_t * n_post, int8_t * site_type, int32_t * allele_count, int8_t * n_pass,
                             int32_t * denovo);
/* ---- PECaller: the columns of a guide file's intervals made on the device ----
 * What the host otherwise does with a BED guide file (the per-position loop of pecaller.c:941-1039): every position of the listed
 * intervals is a column, covered or not.  pecall_dev_sites_stage_records_guided is pecall_dev_sites_stage_records with the columns'
 * positions taken from a list of intervals instead of from the records; recs, n_recs, indiv, p0, span, ref_letters, ref_len, *n_cols
 * and col_slot are as there, and instead of chrom_by_slot:
 *   iv_first[n_iv], iv_count[n_iv]    interval k holds the slots (slot = position - p0) [iv_first[k], iv_first[k] + iv_count[k])
 *   iv_chrom[n_iv] (may be NULL: 0)   the chromosome byte of every column of interval k (chrom_type above; the host program passes
 *                                     chrom_type | 16 for chrY / chrMT, whose columns are called with HAPLOID forced, pecaller.c:955-957)
 *   *n_cols                           columns made: a position is a column if and only if it lies in an interval, so the sum of the
 *                                     counts.  A sample's counts are its record's at that position, six zeros where it has none.
 * Records at positions outside every interval are allowed: they are checked for order and range like the others (PECALL_RC_UNORDERED
 * as above, nothing staged) and ignored.  The reference byte is made as above.  The intervals are checked on the host before any
 * kernel runs, because they become addresses: iv_count[k] >= 1, iv_first[k] + iv_count[k] <= span, and
 * iv_first[k] + iv_count[k] <= iv_first[k + 1] (ascending, disjoint; adjacent is fine).  A violation is a non-zero return with a
 * message, never PECALL_RC_UNORDERED.  n_iv == 0: 0, *n_cols = 0, nothing staged.  Limits as above.  pecall_dev_sites_gather,
 * _sites_run / _collect, _sites_base_text / _gz and _sites_merge_ms (mark = the marks from the intervals and the records' check) follow a
 * guided stage unchanged.  pecall_dev_call_records_guided is the one-call form, as pecall_dev_call_records. */
int pecall_dev_sites_stage_records_guided (pecall_dev * dev, const void *const *recs, const uint64_t * n_recs, int indiv, uint32_t p0,
                                           uint32_t span, const char *ref_letters, uint32_t ref_len, const uint32_t * iv_first,
                                           const uint32_t * iv_count, const uint8_t * iv_chrom /* may be NULL */ , uint32_t n_iv, long *n_cols,
                                           uint32_t * col_slot /* [span], may be NULL */ );
int pecall_dev_call_records_guided (pecall_dev * dev, const void *const *recs, const uint64_t * n_recs, int indiv, uint32_t p0, uint32_t span,
                                    const char *ref_letters, uint32_t ref_len, const uint32_t * iv_first, const uint32_t * iv_count,
                                    const uint8_t * iv_chrom, uint32_t n_iv, long *n_cols, uint32_t * col_slot, int haploid, double threshold,
                                    double theta, int8_t * call, uint32_t * post_site, double *post_rows, uint64_t post_cap, uint64_t * n_post,
                                    int8_t * site_type, int32_t * allele_count, int8_t * n_pass, int32_t * denovo);
/* ---- PECaller: the rows of <outfile>.base.gz made on the device ----
 * What the host otherwise does behind a call: the per-sample text of every column (emit_rows of pecaller_main.c; in the reference
 * the gzprintf loop of pecaller.c:1760-1775).  Valid after pecall_dev_call_sites, _call_sites_sparse, _call_records or
 * pecall_dev_sites_run, for the columns of that call, until the next stage or call: it reads the calls, site types and posteriors
 * the call left on the device.  A column whose samples all have posterior exactly 1 is the template
 * "\n<contig>\t<pos>\t<ref>" + "\t<call>\t1" per sample (a call of 14 or more prints 'N'), and comes back as text; a column the
 * caller skipped (site_type < 0) has no row; a column with some posterior that is not exactly 1 -- the columns
 * pecall_dev_call_sites_sparse lists -- is a hole: the host formats its row (%g) and inserts it.
 *   names, name_off[n_contigs + 1]   the contig names one behind the other: name c = names[name_off[c] .. name_off[c + 1]),
 *                                    at most 1024 bytes each
 *   contig[], pos[], ref_char[]      per column of the last call: its contig (0 .. n_contigs - 1), the position and the reference
 *                                    letter its row prints.  9 bytes per column go up (directly from page-locked arrays).
 *   text[text_cap], *n_text          in column order the rows of every column that is neither skipped nor a hole; each row begins
 *                                    with '\n' and has no trailing newline (the bytes emit_rows appends).  It arrives in pieces of
 *                                    16 MB, directly where pecall_dev_pin_host page-locked it, else through a page-locked block.
 *   hole_site[hole_cap], hole_at[], *n_holes   ascending: the host's row of column hole_site[k] belongs at byte hole_at[k] of text
 *   kernel_ms3 (may be NULL)         HIP-event durations in ms: length, scan, fill
 * Fails (non-zero, pecall_dev_last_error says why) when no call's results are resident, for a contig outside [0, n_contigs), for
 * a position above 2^31 - 1 (the rows print (int) pos as the reference does: no parity is claimed beyond that), and when text_cap
 * or hole_cap is too small -- then *n_text and *n_holes say what is needed, as pecall_dev_call_sites_sparse does with *n_post. */
int pecall_dev_sites_base_text (pecall_dev * dev, const char *names, const uint32_t * name_off /* [n_contigs + 1] */ , int n_contigs,
                                const int32_t * contig, const uint32_t * pos, const char *ref_char /* [columns of the last call] */ ,
                                char *text, uint64_t text_cap, uint64_t * n_text, uint32_t * hole_site, uint64_t * hole_at,
                                uint64_t hole_cap, uint64_t * n_holes, float *kernel_ms3 /* may be NULL: length, scan, fill */ );
/* ---- PECaller: the same rows as gzip members, deflated on the device ----
 * Same inputs and the same validity window as pecall_dev_sites_base_text.  The text that call returns stays on the device and is
 * deflated there by the rule of pecaller_amd/csrc/pecall_gz_rule.h: the text between two holes (or a text end and a hole) is cut into
 * pieces of at most PCG_PIECE bytes, a piece becomes one complete gzip member (fixed Huffman codes, or a stored block where that is
 * no longer), no member reaches across a hole.
 *   gz[gz_cap], *n_gz                the members in text order: inflating gz[0 .. *n_gz) gives exactly the bytes
 *                                    pecall_dev_sites_base_text returns for the same arguments.  An empty text gives *n_gz = 0 and no
 *                                    member.  They arrive in pieces of 16 MB, directly where pecall_dev_pin_host page-locked the
 *                                    buffer, else through a page-locked block.
 *   hole_site[hole_cap], hole_gz_at[], *n_holes   ascending: the host's row of column hole_site[k], as a member or members of the
 *                                    host's making, belongs at byte hole_gz_at[k] of gz, which is a member boundary or *n_gz
 *   *n_text                          the inflated length
 *   kernel_ms5 (may be NULL)         HIP-event durations in ms: length, scan, fill, deflate, pack
 * Fails as pecall_dev_sites_base_text does; when gz_cap or hole_cap is too small *n_gz and *n_holes say what is needed. */
int pecall_dev_sites_base_gz (pecall_dev * dev, const char *names, const uint32_t * name_off /* [n_contigs + 1] */ , int n_contigs,
                              const int32_t * contig, const uint32_t * pos, const char *ref_char /* [columns of the last call] */ ,
                              unsigned char *gz, uint64_t gz_cap, uint64_t * n_gz, uint32_t * hole_site, uint64_t * hole_gz_at,
                              uint64_t hole_cap, uint64_t * n_holes, uint64_t * n_text,
                              float *kernel_ms5 /* may be NULL: length, scan, fill, deflate, pack */ );
/* use_pedfile = y (pecaller.c:376-392, 561-604): parents as sample indices (-1 = not sampled), sex (1 male, 2 female), and each
 * sample's kids in ped-file order: kids of i = kid_list[kid_off[i] .. kid_off[i + 1]).  denovo_rate = argv[11] (<= theta).
 * The configuration prior then carries no_denovo * ln(denovo_rate) (add_denovo, 2396-2445, tables of main 312-374).
 * dad == NULL clears the pedigree. */
int pecall_dev_set_pedigree (pecall_dev * dev, int indiv, const int *dad, const int *mom, const int *sex, const int *kid_off,
                             const int *kid_list, double denovo_rate);

#ifdef __cplusplus
}
#endif
#endif
