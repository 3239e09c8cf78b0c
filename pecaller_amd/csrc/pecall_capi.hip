// pecall_capi.hip -- C-ABI of the PECaller likelihood kernel (include/pemap_hip.h, pecall_dev_*).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <math.h>
#include <chrono>
#include <memory>
#include <vector>
#include <algorithm>
#include "../../include/pemap_hip.h"
#include "pecall_kernels.hip.h"
#include "pecall_site.hip.h"
#include "pecall_merge.hip.h"
#include "pecall_rows.hip.h"
#include "pecall_gz.hip.h"

static char g_pc_err[512] = "";
#define PCS_SLOTS 3             // staging buffers of the seam's pipeline (chunks in flight between the two host copies)
#define PCS_CALL_STREAMS 4       // streams the beam searches of consecutive chunks alternate on (each with a quarter of the waves and of the scratch)
// the 64-bit counters of a chunk, and of a list of the early beam search (pcs_chunk_ctrs, pcs_heavy_ctrs); [0]: the beam search's work counter
enum
{
  PCS_CTR_LISTED = 1,           // [1..2]: the PCS_BUCKETS 32-bit counts of listed columns
  PCS_CTR_DEEP = 3,             // columns on the deep list (32 bits)
  PCS_CTR_PIECE = 4,            // the shortcut kernel's work counter
  PCS_CTRS = 6
};

// host ranges page-locked by the caller (one table for the library: pemap_capi.hip)
bool pm_host_pin_lookup (const void *p, size_t bytes);
bool pm_host_pin_range (const void *p, size_t bytes, hipStream_t copy_stream);
int pm_host_unpin (const void *host_ptr);
void pm_par_memcpy (char *dst, const char *src, size_t bytes);

// Tuning knobs.  The environment is read ONCE, by pecall_dev_create, into the object, as the mapper reads its
// PmKnobs: nothing below calls getenv again but the two diagnostics that are documented as read per call (PECALL_LIST_STATS,
// PECALL_SEAM_TRACE).  None is needed in normal use.
struct PcKnobs
{
  int chunk_log2;               // PECALL_CHUNK_LOG2 (8 .. 24): log2 of the columns per chunk of the pipeline
  // PECALL_HEAVY_MIN: samples with variant reads from which a column's beam search is started ahead of the shortcut kernels; 0 = never
  // ... beyond 128 samples (PECALL_HEAVY_MIN_WIDE): a column's beam search costs tens of milliseconds there and the small beam settles
  // most columns whose only variant reads are errors, so the early start takes the columns with several such samples only
  int heavy_min, heavy_min_wide;
  int heavy_waves;              // PECALL_HEAVY_WAVES (1 .. 4): waves per CU of the early beam search's launch
  bool flat_priorities;         // PECALL_FLAT_PRIORITIES (diagnostic: every stream at the default priority, as before round 4)
};

static int env_int (const char *name, int dflt)
{
  const char *e = getenv (name);
  return (e && *e) ? atoi (e) : dflt;
}

static void read_knobs (PcKnobs & k)
{
  k.chunk_log2 = std::min (std::max (env_int ("PECALL_CHUNK_LOG2", 18), 8), 24);
  k.heavy_min = env_int ("PECALL_HEAVY_MIN", 1);
  k.heavy_min_wide = env_int ("PECALL_HEAVY_MIN_WIDE", 3);
  k.heavy_waves = std::min (std::max (env_int ("PECALL_HEAVY_WAVES", 3), 1), 4);
  k.flat_priorities = getenv ("PECALL_FLAT_PRIORITIES") != nullptr;
}

// release and null: every group's *_free is made of these, so that a group can be freed twice and allocated again
template < class ... T > static void pc_free (T * &... p)
{
  ((hipFree (p), p = nullptr), ...);
}

template < class ... T > static void pc_host_free (T * &... p)
{
  ((p ? (void) hipHostFree (p) : (void) 0, p = nullptr), ...);
}

// pecall_dev_site_like (fill_sample_like): reads and alpha in, likelihoods out
struct PcLike
{
  uint16_t *d_reads = nullptr;
  double *d_alpha = nullptr, *d_like = nullptr, *d_margin = nullptr;
  int8_t *d_best = nullptr;
  long cap_items = 0, cap_sites = 0;
};

static void pc_like_free (PcLike & l)
{
  pc_free (l.d_reads, l.d_alpha, l.d_like, l.d_margin, l.d_best);
  l.cap_items = l.cap_sites = 0;
}

// the per-site caller's tables: made by create (ln n!, pass 1's Dirichlet parameters), per sample count (Hardy-Weinberg), per pedigree
struct PcsTables
{
  double *d_tab = nullptr;
  uint32_t *d_ta = nullptr;     // pass 1's integer Dirichlet parameters (pcs_ta_table)
  double *d_hw = nullptr;
  int *d_hw_off = nullptr;
  int hw_indiv = 0;
  int16_t *d_ped = nullptr;     // int16: dad[MAXN] mom[MAXN] kid_off[MAXN + 8] kid_list[2 MAXN]; then bytes: sex[MAXN]
  short *d_dyad = nullptr, *d_trio = nullptr;
};

static void pcs_tables_free (PcsTables & t)
{
  pc_free (t.d_tab, t.d_ta, t.d_hw, t.d_hw_off, t.d_ped, t.d_dyad, t.d_trio);
  t.hw_indiv = 0;
}

// the column arrays: a column's reads, reference base and chromosome class in, its results out, and the lists the kernels keep of columns
struct PcsColumns
{
  uint16_t *d_sreads = nullptr;
  uint8_t *d_dom = nullptr, *d_chromy = nullptr;
  int8_t *d_call = nullptr, *d_type = nullptr, *d_npass = nullptr;
  double *d_post = nullptr;
  int32_t *d_ac = nullptr, *d_den = nullptr;
  unsigned *d_slow = nullptr;   // columns left to the beam search (PCS_BUCKETS parts per chunk, at the chunk's offset)
  unsigned *d_deep = nullptr;   // columns too deep for the head of the ln n! table (per chunk, at the chunk's offset)
  // the columns pcs_heavy_kernel lists for the beam search before the shortcut kernels start: flags, the list in PCS_BUCKETS parts
  uint8_t *d_heavy_flag = nullptr;
  unsigned *d_heavy_list = nullptr;
  long cap_sites = 0, cap_items = 0;
};

// (nothing dangles if an allocation after it fails: the next call allocates again, destroy frees nullptr)
static void pcs_columns_free (PcsColumns & c)
{
  pc_free (c.d_sreads, c.d_dom, c.d_chromy, c.d_call, c.d_type, c.d_npass, c.d_post, c.d_ac, c.d_den, c.d_slow, c.d_deep, c.d_heavy_flag, c.d_heavy_list);
  c.cap_sites = c.cap_items = 0;
}

// the beam searches' scratch: site_grid waves in PCS_CALL_STREAMS shares (the chunks' searches), behind them heavy_grid waves (the early
// search of a whole run's list); `row` = the calls-row width (64 per chunk of samples) it was sized for
struct PcsScratch
{
  char *d = nullptr;
  int row = 0, site_grid = 0, heavy_grid = 0;
};

static void pcs_scratch_free (PcsScratch & s)
{
  pc_free (s.d);
}

// pecall_dev_call_sites_sparse: the columns with a posterior that is not 1 (pcs_sparse_kernel)
struct PcsSparse
{
  unsigned *d_cols = nullptr;
  double *d_rows = nullptr;
  unsigned long long *d_n = nullptr;
  unsigned long long cap = 0;
  int indiv = 0;
};

static void pcs_sparse_free (PcsSparse & s)
{
  pc_free (s.d_cols, s.d_rows, s.d_n);
  s.cap = s.indiv = 0;
}

// pecall_dev_sites_stage_records (pecall_merge.hip.h): the samples' records one behind the other and where each sample's begin; per
// slot of the range its mark, its column, its reference letter and chromosome class; per column its slot; the blocks' counts of the
// scan.  And pecall_dev_sites_gather's pieces.
struct PcmState
{
  uint4 *d_recs = nullptr;
  size_t cap_recs = 0;
  unsigned long long *d_off = nullptr;  // [PCS_MAXN + 1]
  uint8_t *d_marks = nullptr, *d_letters = nullptr, *d_chrom = nullptr;
  unsigned *d_colof = nullptr, *d_colslot = nullptr, *d_bsum = nullptr;
  size_t cap_span = 0;
  unsigned *d_iv = nullptr;     // the guided form's intervals: first[cap_iv], count[cap_iv], then a byte each
  size_t cap_iv = 0;
  PcmCtl *d_ctl = nullptr;
  char *h_stage = nullptr;      // page-locked: what comes back (PcmCtl, col_slot), then what goes up (offsets, letters, classes, records that are not pinned)
  size_t h_stage_bytes = 0;
  hipEvent_t ev[6] = { };       // around the mark kernel, the scan's first two kernels, its third, the tile kernel
  float ms[3] = { };            // mark, scan, tile of the last pecall_dev_sites_stage_records
  char *d_gather = nullptr, *h_gather = nullptr;
  size_t cap_gather = 0;
};

static void pcm_free (PcmState & g)
{
  pc_free (g.d_recs, g.d_off, g.d_ctl, g.d_bsum, g.d_marks, g.d_letters, g.d_chrom, g.d_colof, g.d_colslot, g.d_gather, g.d_iv);
  pc_host_free (g.h_stage, g.h_gather);
  g.cap_recs = g.cap_span = g.h_stage_bytes = g.cap_gather = g.cap_iv = 0;
  for (hipEvent_t & e : g.ev)
    if (e && hipEventDestroy (e) == hipSuccess)
      e = nullptr;
}

// pecall_dev_sites_base_text (pecall_rows.hip.h): the columns' heads and the contig names as they went up; per padded column its length
// word and its byte offset; the blocks' sums of the scan; the holes; the text; and the page-locked blocks things travel through
#define PCR_PIECE ((size_t) 16 << 20)   // bytes of text per device-to-host copy
struct PcrState
{
  int32_t *d_contig = nullptr;
  uint32_t *d_pos = nullptr, *d_name_off = nullptr, *d_hole_site = nullptr;
  char *d_ref = nullptr, *d_names = nullptr, *d_text = nullptr;
  unsigned *d_len = nullptr, *d_bsum_holes = nullptr;
  unsigned long long *d_off = nullptr, *d_bsum_bytes = nullptr, *d_hole_at = nullptr;
  PcrCtl *d_ctl = nullptr;
  size_t cap_cols = 0, cap_names = 0, cap_contigs = 0, cap_text = 0;       // cap_cols: padded columns
  char *h_stage = nullptr;      // [PcrCtl][contig][pos][ref][name offsets][names][hole columns][hole offsets]
  size_t h_stage_bytes = 0;
  char *h_text[2] = { };        // PCR_PIECE each: the text's pieces on their way to a target that is not page-locked
  hipEvent_t ev_piece[2] = { };
  hipEvent_t ev[6] = { };       // around the length kernel, the scan's first two kernels, its third, the fill kernel
};

static void pcr_free (PcrState & w)
{
  pc_free (w.d_contig, w.d_pos, w.d_name_off, w.d_hole_site, w.d_ref, w.d_names, w.d_text, w.d_len, w.d_bsum_holes, w.d_off, w.d_bsum_bytes, w.d_hole_at, w.d_ctl);
  pc_host_free (w.h_stage, w.h_text[0], w.h_text[1]);
  w.cap_cols = w.cap_names = w.cap_contigs = w.cap_text = w.h_stage_bytes = 0;
  for (hipEvent_t * e : { &w.ev[0], &w.ev[1], &w.ev[2], &w.ev[3], &w.ev[4], &w.ev[5], &w.ev_piece[0], &w.ev_piece[1] })
    if (*e && hipEventDestroy (*e) == hipSuccess)
      *e = nullptr;
}

// pecall_dev_sites_base_gz (pecall_gz.hip.h): the runs' piece counts and their scan; per piece its first byte, its length and its member's
// length (scanned: its place in the packed array); the slots; the packed members; the holes' places among them
struct PcgState
{
  unsigned long long *d_run = nullptr, *d_run_sum = nullptr, *d_piece_at = nullptr, *d_member = nullptr, *d_member_sum = nullptr, *d_hole_gz_at = nullptr;
  unsigned *d_piece_len = nullptr;
  unsigned char *d_slots = nullptr, *d_gz = nullptr;
  PcgCtl *d_ctl = nullptr;
  size_t cap_runs = 0, cap_pieces = 0, cap_slots = 0, cap_holes = 0;       // cap_runs, cap_pieces: padded to PCG_SCAN_TILE
  char *h_stage = nullptr;      // [PcgCtl][hole columns][hole places]
  size_t h_stage_bytes = 0;
  hipEvent_t ev[3] = { };       // around the deflate (runs, scan, table, deflate kernel) and the pack (scan, pack, holes)
};

static void pcg_free (PcgState & g)
{
  pc_free (g.d_run, g.d_run_sum, g.d_piece_at, g.d_member, g.d_member_sum, g.d_hole_gz_at, g.d_piece_len, g.d_slots, g.d_gz, g.d_ctl);
  pc_host_free (g.h_stage);
  g.cap_runs = g.cap_pieces = g.cap_slots = g.cap_holes = g.h_stage_bytes = 0;
  for (hipEvent_t & e : g.ev)
    if (e && hipEventDestroy (e) == hipSuccess)
      e = nullptr;
}

struct PcsChunk
{
  hipEvent_t h2d, fast, call, d2h, heavy;       // a chunk's columns in, shortcut kernel done, beam search and what follows it done, results out, early beam search done
};

struct pecall_dev
{
  int device = 0;
  PcKnobs kn = { };
  hipStream_t stream = nullptr;
  char err[512] = "";
  int grid = 0;
  PcLike like;
  PcsTables tab;
  PcsColumns cols;
  PcsScratch scratch;
  PcsSparse sp;
  PcmState mg;
  PcrState rows;
  PcgState gz;
  // pedigree
  int ped_indiv = 0, ped_haploid = 0;
  double denovo_rate = 0;
  int16_t h_dad[PCS_MAXN] = { }, h_mom[PCS_MAXN] = { };
  int8_t h_sex[PCS_MAXN] = { };
  uint16_t h_kid_off[PCS_MAXN + 1] = { }, h_kid_list[2 * PCS_MAXN] = { };
  long staged_sites = 0;
  int staged_indiv = 0;
  long result_sites = 0;        // columns whose results lie in `cols` (the last call's or run's; 0 once something new is staged)
  // the caller in chunks of chunk_sites columns (pcs_chunk_kernels): the shortcut kernel of chunk k + 1 runs beside the beam search of
  // chunk k, and at the seam (pecall_dev_call_sites) beside the copies of the chunks around them.  Streams and events are made by the
  // first call that needs chunks (pcs_ensure_chunks).
  long chunk_sites = 0;
  hipStream_t stream_call[PCS_CALL_STREAMS] = { }, stream_h2d = nullptr, stream_d2h = nullptr;
  hipStream_t stream_heavy = nullptr;   // the early beam search of a whole run's list
  hipEvent_t ev_site[2] = { }, ev_heavy[2] = { };       // around a resident run (made by create); the early list made / a whole run's early beam search done
  std::vector < PcsChunk > chunks;
  size_t cap_chunks = 0;        // chunks whose events and counters are all there
  unsigned long long *d_chunk_ctr = nullptr;    // [cap_chunks][PCS_CTRS]
  unsigned long long *d_heavy_ctr = nullptr;    // [1 + cap_chunks][PCS_CTRS]: slot 0 for a whole run's list (resident columns), slot 1 + k for chunk k's (the seam)
  // pecall_dev_sites_stats: what the first pass listed in the chunks whose second pass then cleared their counters; was the early list made?
  unsigned long long run_listed_first[4] = { 0ull, 0ull, 0ull, 0ull };
  bool run_heavy = false;
  long run_stats_sites = 0;     // columns of the sites_run the counters belong to (0: the last results are a seam call's, whose chunks count for themselves)
  unsigned long long *h_ctrs = nullptr; // page-locked: the chunks' counters, behind them the sparse list's length, on their way to the host (pcs_sparse_len_at)
  char *h_in[PCS_SLOTS] = { }, *h_out[PCS_SLOTS] = { }; // pinned staging for callers whose buffers are not pinned
  size_t h_in_bytes = 0, h_out_bytes = 0;
};

static unsigned long long *pcs_chunk_ctrs (pecall_dev * d, int k)
{
  return d->d_chunk_ctr + (size_t) k * PCS_CTRS;
}

static unsigned long long *pcs_heavy_ctrs (pecall_dev * d, int slot)
{
  return d->d_heavy_ctr + (size_t) slot * PCS_CTRS;
}

// the word of h_ctrs in which the sparse list's length reaches the host: the one behind the counters of `chunks` chunks
static size_t pcs_sparse_len_at (size_t chunks)
{
  return chunks * PCS_CTRS;
}

static int pc_fail (pecall_dev * d, const char *fmt, ...)
{
  va_list ap;
  va_start (ap, fmt);
  vsnprintf (d ? d->err : g_pc_err, 512, fmt, ap);
  va_end (ap);
  return 1;
}

#define PCCHK(d, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return pc_fail (d, "%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString (e_)); } while (0)
#define PCTRY(x) do { int r_ = (x); if (r_) return r_; } while (0)

// the reference's ln n! table, pecaller.c:3163-3214, evaluated with the host libm as the reference does
static double h_gammln (double xx)
{
  static const double cof[6] = { 76.18009173, -86.50532033, 24.01409822, -1.231739516, 0.120858003e-2, -0.536382e-5 };
  double x = xx - 1.0, tmp = x + 5.5, ser = 1.0;
  tmp -= (x + 0.5) * log (tmp);
  for (int j = 0; j <= 5; j++)
    {
      x += 1.0;
      ser += cof[j] / x;
    }
  return -tmp + log (2.50662827465 * ser);
}

static double h_factln (int n)
{
  if (n <= 1)
    return 0.0;
  if (n <= 40)
    {
      double x = 1.0;
      for (int i = 2; i <= n; i++)
        x *= (double) i;
      return log (x);
    }
  return h_gammln (n + 1.0);
}

extern "C" const char *pecall_dev_last_error (const pecall_dev * d)
{
  return d ? d->err : g_pc_err;
}

extern "C" int pecall_dev_create (pecall_dev ** out, int device_id)
{
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount (&n) != hipSuccess || n <= 0)
    return pc_fail (nullptr, "no HIP device visible: this library has no CPU path");
  if (device_id < 0 || device_id >= n)
    return pc_fail (nullptr, "device %d out of range", device_id);
  std::unique_ptr < pecall_dev, void (*)(pecall_dev *) > d (new pecall_dev (), pecall_dev_destroy);
  d->device = device_id;
  PCCHK (nullptr, hipSetDevice (device_id));
  hipDeviceProp_t prop;
  PCCHK (nullptr, hipGetDeviceProperties (&prop, device_id));
  if (strncmp (prop.gcnArchName, "gfx950", 6) != 0)
    return pc_fail (nullptr, "device %d is %s: built for gfx950 only", device_id, prop.gcnArchName);
  read_knobs (d->kn);
  d->chunk_sites = 1L << d->kn.chunk_log2;
  d->grid = (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256) * 2;
  PCCHK (nullptr, hipStreamCreateWithFlags (&d->stream, hipStreamNonBlocking));
  for (hipEvent_t & e : d->ev_site)
    PCCHK (nullptr, hipEventCreate (&e));
  std::vector < double >tab (PC_TABLE);
  for (int i = 0; i < PC_TABLE; i++)
    tab[i] = h_factln (i);
  PCCHK (nullptr, hipMalloc ((void **) &d->tab.d_tab, sizeof (double) * PC_TABLE));
  PCCHK (nullptr, hipMemcpy (d->tab.d_tab, tab.data (), sizeof (double) * PC_TABLE, hipMemcpyHostToDevice));
  std::vector < uint32_t > ta ((PCS_TA_BYTES + 3) / 4);
  pcs_ta_table (ta.data ());
  PCCHK (nullptr, hipMalloc ((void **) &d->tab.d_ta, PCS_TA_BYTES));
  PCCHK (nullptr, hipMemcpy (d->tab.d_ta, ta.data (), PCS_TA_BYTES, hipMemcpyHostToDevice));
  PCCHK (nullptr, hipFuncSetAttribute ((const void *) pc_site_like_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PC_TABLE * 8));
  *out = d.release ();
  return 0;
}

extern "C" void pecall_dev_destroy (pecall_dev * d)
{
  if (!d)
    return;
  hipSetDevice (d->device);
  hipStreamSynchronize (d->stream);
  pc_like_free (d->like);
  pcs_tables_free (d->tab);
  pcs_columns_free (d->cols);
  pcs_scratch_free (d->scratch);
  pcs_sparse_free (d->sp);
  pcm_free (d->mg);
  pcr_free (d->rows);
  pcg_free (d->gz);
  pc_free (d->d_chunk_ctr, d->d_heavy_ctr);
  pc_host_free (d->h_ctrs);
  for (int i = 0; i < PCS_SLOTS; i++)
    pc_host_free (d->h_in[i], d->h_out[i]);
  for (const PcsChunk & c : d->chunks)
    for (hipEvent_t e : { c.h2d, c.fast, c.call, c.d2h, c.heavy })
      if (e)
        hipEventDestroy (e);
  for (hipEvent_t e : { d->ev_site[0], d->ev_site[1], d->ev_heavy[0], d->ev_heavy[1] })
    if (e)
      hipEventDestroy (e);
  for (hipStream_t s : { d->stream_call[0], d->stream_call[1], d->stream_call[2], d->stream_call[3], d->stream_h2d, d->stream_d2h, d->stream_heavy, d->stream })
    if (s)
      hipStreamDestroy (s);
  delete d;
}

static int pc_ensure (pecall_dev * d, long n_sites, long n_items)
{
  PcLike & l = d->like;
  if (n_items > l.cap_items)
    {
      pc_free (l.d_reads, l.d_like, l.d_margin, l.d_best);
      l.cap_items = 0;
      PCCHK (d, hipMalloc ((void **) &l.d_reads, n_items * PC_ALLELES * sizeof (uint16_t)));
      PCCHK (d, hipMalloc ((void **) &l.d_like, n_items * PC_MAX_GEN * sizeof (double)));
      PCCHK (d, hipMalloc ((void **) &l.d_margin, n_items * sizeof (double)));
      PCCHK (d, hipMalloc ((void **) &l.d_best, n_items));
      l.cap_items = n_items;
    }
  if (n_sites > l.cap_sites)
    {
      pc_free (l.d_alpha);
      l.cap_sites = 0;
      PCCHK (d, hipMalloc ((void **) &l.d_alpha, n_sites * PC_MAX_GEN * PC_ALLELES * sizeof (double)));
      l.cap_sites = n_sites;
    }
  return 0;
}

extern "C" int pecall_dev_stage (pecall_dev * d, const uint16_t * reads, const double *alpha_mean, int n_sites, int indiv)
{
  PCCHK (d, hipSetDevice (d->device));
  if (n_sites <= 0 || indiv <= 0)
    return pc_fail (d, "stage: n_sites %d indiv %d", n_sites, indiv);
  long n_items = (long) n_sites * indiv;
  PCTRY (pc_ensure (d, n_sites, n_items));
  PCCHK (d, hipMemcpy (d->like.d_reads, reads, n_items * PC_ALLELES * sizeof (uint16_t), hipMemcpyHostToDevice));
  PCCHK (d, hipMemcpy (d->like.d_alpha, alpha_mean, (long) n_sites * PC_MAX_GEN * PC_ALLELES * sizeof (double), hipMemcpyHostToDevice));
  return 0;
}

extern "C" int pecall_dev_run (pecall_dev * d, int n_sites, int indiv, int max_gen, int min_depth, double norm, int sync)
{
  PCCHK (d, hipSetDevice (d->device));
  long n_items = (long) n_sites * indiv;
  if (n_items > d->like.cap_items || n_sites > d->like.cap_sites)
    return pc_fail (d, "run: more items than staged");
  if (max_gen < 1 || max_gen > PC_MAX_GEN)
    return pc_fail (d, "run: max_gen %d", max_gen);
  hipLaunchKernelGGL (pc_site_like_kernel, dim3 (d->grid), dim3 (PC_BLOCK), PC_TABLE * sizeof (double), d->stream, d->like.d_reads, d->like.d_alpha,
                      d->tab.d_tab, n_items, indiv, max_gen, min_depth, norm, d->like.d_like, d->like.d_best, d->like.d_margin);
  PCCHK (d, hipGetLastError ());
  if (sync)
    PCCHK (d, hipStreamSynchronize (d->stream));
  return 0;
}

extern "C" int pecall_dev_collect (pecall_dev * d, int n_sites, int indiv, double *like, int8_t * best, double *margin)
{
  PCCHK (d, hipSetDevice (d->device));
  long n_items = (long) n_sites * indiv;
  PCCHK (d, hipStreamSynchronize (d->stream));
  if (like)
    PCCHK (d, hipMemcpy (like, d->like.d_like, n_items * PC_MAX_GEN * sizeof (double), hipMemcpyDeviceToHost));
  if (best)
    PCCHK (d, hipMemcpy (best, d->like.d_best, n_items, hipMemcpyDeviceToHost));
  if (margin)
    PCCHK (d, hipMemcpy (margin, d->like.d_margin, n_items * sizeof (double), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int pecall_dev_site_like (pecall_dev * d, const uint16_t * reads, const double *alpha_mean, int n_sites, int indiv,
                                     int max_gen, int min_depth, double norm, double *like, int8_t * best, double *margin)
{
  PCTRY (pecall_dev_stage (d, reads, alpha_mean, n_sites, indiv));
  PCTRY (pecall_dev_run (d, n_sites, indiv, max_gen, min_depth, norm, 1));
  return pecall_dev_collect (d, n_sites, indiv, like, best, margin);
}

// ---- per-site caller (pecall_site.hip.h)

// ln of the exact Hardy-Weinberg probabilities (fill_hardy_weinberg, pecaller.c:2791-2866) for n diploids: row = number of
// minor alleles (0 .. 2n), column = heterozygotes; built with the host libm like the reference's table
static void h_hardy_weinberg (int n, double *m)
{
  const int asize = 2 * n, cols = n + 1;
  for (long x = 0; x < (long) (asize + 1) * cols; x++)
    m[x] = 0.0;
  for (int i = 1; i <= asize; i++)
    {
      double *row = m + (long) i * cols;
      const int Na = 2 * n - i, Nb = i;
      const double p = (double) i / (double) (Na + Nb);
      const int expect = (int) ceil (i * (1.0 - p));
      const int start = ((expect & 1) == (i & 1)) ? expect : expect - 1;
      double sum = row[start] = 1.0;
      int nbb = (Nb - start) / 2, naa = (Na - start) / 2;
      for (int nab = start + 2; naa > 0 && nbb > 0; nab += 2, naa--, nbb--)
        {
          row[nab] = row[nab - 2] * 4.0 * ((double) naa * (double) nbb) / ((double) (nab) * (double) (nab - 1.0));
          sum += row[nab];
        }
      nbb = (Nb - start) / 2;
      naa = (Na - start) / 2;
      for (int nab = start - 2; nab >= 0; nab -= 2, naa++, nbb++)
        {
          row[nab] = row[nab + 2] * ((double) (nab + 2.0) * (double) (nab + 1.0)) / ((double) 4.0 * ((double) (naa + 1.0) * (nbb + 1.0)));
          sum += row[nab];
        }
      for (int j = 0; j <= n; j++)
        row[j] /= sum;
    }
  for (long x = 0; x < (long) (asize + 1) * cols; x++)
    m[x] = m[x] > 1e-50 ? log (m[x]) : -5000;
}

// chunks of 64 samples a lane of the per-site kernels stands for: 1, 2, 4 or 8 (their template argument)
static int pcs_sample_chunks (int indiv)
{
  return indiv <= 64 ? 1 : indiv <= 128 ? 2 : indiv <= 256 ? 4 : 8;
}

static size_t pcs_wave_scratch_bytes (int indiv)
{
  return 2 * PCS_BIG_BYTES_OF (64 * pcs_sample_chunks (indiv)) + PCS_BIGCAP;
}

// the share of the scratch of beam-search stream i; i = PCS_CALL_STREAMS: the early beam search's, behind them
static char *pcs_scratch_share (pecall_dev * d, int i, int indiv)
{
  return d->scratch.d + (size_t) i * (size_t) (d->scratch.site_grid / PCS_CALL_STREAMS) * pcs_wave_scratch_bytes (indiv);
}

static int pcs_heavy_min (const pecall_dev * d, int indiv)
{
  return indiv <= 128 ? d->kn.heavy_min : d->kn.heavy_min_wide;
}

static int pcs_ensure (pecall_dev * d, long n_sites, int indiv)
{
  PcsTables & t = d->tab;
  if (indiv != t.hw_indiv)
    {
      pc_free (t.d_hw, t.d_hw_off);
      std::vector < int >off ((size_t) indiv + 2, 0);
      long tot = 0;
      for (int n = 1; n <= indiv; n++)
        {
          off[n] = (int) tot;
          tot += (long) (2 * n + 1) * (n + 1);
        }
      std::vector < double >hw ((size_t) tot);
      for (int n = 1; n <= indiv; n++)
        h_hardy_weinberg (n, hw.data () + off[n]);
      PCCHK (d, hipMalloc ((void **) &t.d_hw, sizeof (double) * tot));
      PCCHK (d, hipMalloc ((void **) &t.d_hw_off, sizeof (int) * (indiv + 2)));
      PCCHK (d, hipMemcpy (t.d_hw, hw.data (), sizeof (double) * tot, hipMemcpyHostToDevice));
      PCCHK (d, hipMemcpy (t.d_hw_off, off.data (), sizeof (int) * (indiv + 2), hipMemcpyHostToDevice));
      t.hw_indiv = indiv;
    }
  PcsScratch & s = d->scratch;
  const int row = 64 * pcs_sample_chunks (indiv);
  if (!s.d || row > s.row)
    {
      PCCHK (d, hipDeviceSynchronize ());
      pcs_scratch_free (s);
      s.site_grid = d->grid * 4;        // 8 waves per CU; LDS admits 4 resident, the rest queue
      s.heavy_grid = d->grid / 2 * d->kn.heavy_waves;   // (the early beam search of the listed heavy columns: behind the site_grid shares)
      PCCHK (d, hipMalloc ((void **) &s.d, (size_t) (s.site_grid + s.heavy_grid) * pcs_wave_scratch_bytes (indiv)));
      s.row = row;
    }
  PcsColumns & c = d->cols;
  const long items = n_sites * indiv;
  if (n_sites > c.cap_sites || items > c.cap_items)
    {
      pcs_columns_free (c);
      PCCHK (d, hipMalloc ((void **) &c.d_slow, (size_t) PCS_BUCKETS * n_sites * sizeof (unsigned)));
      PCCHK (d, hipMalloc ((void **) &c.d_deep, (size_t) n_sites * sizeof (unsigned)));
      PCCHK (d, hipMalloc ((void **) &c.d_heavy_flag, (size_t) n_sites));
      PCCHK (d, hipMalloc ((void **) &c.d_heavy_list, (size_t) PCS_BUCKETS * n_sites * sizeof (unsigned)));
      PCCHK (d, hipMalloc ((void **) &c.d_sreads, items * PCS_NA * sizeof (uint16_t)));
      PCCHK (d, hipMalloc ((void **) &c.d_dom, n_sites));
      PCCHK (d, hipMalloc ((void **) &c.d_chromy, n_sites));
      PCCHK (d, hipMalloc ((void **) &c.d_call, items));
      PCCHK (d, hipMalloc ((void **) &c.d_post, items * sizeof (double)));
      PCCHK (d, hipMalloc ((void **) &c.d_type, n_sites));
      PCCHK (d, hipMalloc ((void **) &c.d_npass, n_sites));
      PCCHK (d, hipMalloc ((void **) &c.d_ac, n_sites * PCS_NA * sizeof (int32_t)));
      PCCHK (d, hipMalloc ((void **) &c.d_den, n_sites * sizeof (int32_t)));
      c.cap_sites = n_sites;
      c.cap_items = items;
    }
  return 0;
}

// get_het_alleles, pecaller.c:2191-2245
static void h_het (int g, int *a, int *b, int ref)
{
  static const int ha[6] = { 0, 0, 0, 1, 1, 2 }, hb[6] = { 1, 2, 3, 2, 3, 3 };
  if (g < PCS_NA)
    *a = *b = g;
  else if (g < 12)
    {
      *a = ha[g - 6];
      *b = hb[g - 6];
    }
  else
    {
      *a = ref;
      *b = g == 12 ? 4 : 5;
    }
}

// dyad_denovo / trio_denovo as main fills them (pecaller.c:312-374), for the four reference bases
static void h_denovo_tables (int haploid, short *dyad, short *trio)
{
  memset (dyad, 0, sizeof (short) * 4 * 225);
  memset (trio, 0, sizeof (short) * 4 * 3375);
  const int G = haploid ? 6 : PCS_NG;
  for (int r = 0; r < 4; r++)
    for (int i = 0; i < G; i++)
      for (int j = 0; j < G; j++)
        {
          if (haploid)
            {
              dyad[r * 225 + i * 15 + j] = i != j;
              continue;
            }
          int da, db, ka, kb;
          h_het (i, &da, &db, r);
          h_het (j, &ka, &kb, r);
          if (ka != da && ka != db && kb != da && kb != db)
            dyad[r * 225 + i * 15 + j] = 1;
          for (int k = 0; k < G; k++)
            {
              int ma, mb;
              h_het (k, &ma, &mb, r);
              short v;
              if ((ka == ma && (kb == da || kb == db)) || (ka == mb && (kb == da || kb == db)) || (kb == ma && (ka == da || ka == db))
                  || (kb == mb && (ka == da || ka == db)))
                v = 0;          // one allele from each parent
              else if (ka != ma && kb != db && kb != ma && ka != db && ka != mb && kb != da && kb != mb && ka != da)
                v = 2;
              else
                v = 1;
              trio[r * 3375 + (i * 15 + k) * 15 + j] = v;       // [dad][mom][kid]
            }
        }
}

extern "C" int pecall_dev_set_pedigree (pecall_dev * d, int indiv, const int *dad, const int *mom, const int *sex, const int *kid_off,
                                        const int *kid_list, double denovo_rate)
{
  if (!dad)
    {
      d->ped_indiv = 0;
      return 0;
    }
  if (indiv < 1 || indiv > PCS_MAXN)
    return pc_fail (d, "set_pedigree: %d samples (1..%d)", indiv, PCS_MAXN);
  if (!(denovo_rate >= 1e-30))
    return pc_fail (d, "set_pedigree: de-novo mutation rate %g (pecaller.c:381-385)", denovo_rate);
  if (!kid_off || !kid_list || kid_off[0] != 0 || kid_off[indiv] < 0 || kid_off[indiv] > 2 * PCS_MAXN)
    return pc_fail (d, "set_pedigree: kid_off must start at 0 and end at no more than %d parent-child links", 2 * PCS_MAXN);
  for (int i = 0; i < indiv; i++)
    if (kid_off[i + 1] < kid_off[i])
      return pc_fail (d, "set_pedigree: kid_off is not ascending at sample %d", i);
  for (int i = 0; i < kid_off[indiv]; i++)
    if (kid_list[i] < 0 || kid_list[i] >= indiv)
      return pc_fail (d, "set_pedigree: kid_list[%d] = %d is not a sample index (0..%d)", i, kid_list[i], indiv - 1);
  for (int i = 0; i < indiv; i++)
    {
      if (dad[i] >= indiv || mom[i] >= indiv)
        return pc_fail (d, "set_pedigree: parent index out of range for sample %d", i);
      d->h_dad[i] = (int16_t) (dad[i] < 0 ? -1 : dad[i]);
      d->h_mom[i] = (int16_t) (mom[i] < 0 ? -1 : mom[i]);
      d->h_sex[i] = (int8_t) sex[i];
    }
  for (int i = 0; i <= indiv; i++)
    d->h_kid_off[i] = (uint16_t) kid_off[i];
  for (int i = 0; i < kid_off[indiv]; i++)
    d->h_kid_list[i] = (uint16_t) kid_list[i];
  d->ped_indiv = indiv;
  d->denovo_rate = denovo_rate;
  d->ped_haploid = -1;          // tables are made at the next call, for its ploidy
  return 0;
}

static int pcs_ensure_ped (pecall_dev * d, int haploid)
{
  if (!d->tab.d_ped)
    {
      PCCHK (d, hipMalloc ((void **) &d->tab.d_ped, sizeof (int16_t) * (5 * PCS_MAXN + 8) + PCS_MAXN));
      PCCHK (d, hipMalloc ((void **) &d->tab.d_dyad, sizeof (short) * 4 * 225));
      PCCHK (d, hipMalloc ((void **) &d->tab.d_trio, sizeof (short) * 4 * 3375));
    }
  if (d->ped_haploid != haploid)
    {
      std::vector < short >dy (4 * 225), tr (4 * 3375);
      h_denovo_tables (haploid, dy.data (), tr.data ());
      PCCHK (d, hipMemcpy (d->tab.d_dyad, dy.data (), sizeof (short) * 4 * 225, hipMemcpyHostToDevice));
      PCCHK (d, hipMemcpy (d->tab.d_trio, tr.data (), sizeof (short) * 4 * 3375, hipMemcpyHostToDevice));
      PCCHK (d, hipMemcpy (d->tab.d_ped, d->h_dad, sizeof (int16_t) * PCS_MAXN, hipMemcpyHostToDevice));
      PCCHK (d, hipMemcpy (d->tab.d_ped + PCS_MAXN, d->h_mom, sizeof (int16_t) * PCS_MAXN, hipMemcpyHostToDevice));
      PCCHK (d, hipMemcpy (d->tab.d_ped + 2 * PCS_MAXN, d->h_kid_off, sizeof (uint16_t) * (PCS_MAXN + 1), hipMemcpyHostToDevice));
      PCCHK (d, hipMemcpy (d->tab.d_ped + 3 * PCS_MAXN + 8, d->h_kid_list, sizeof (uint16_t) * 2 * PCS_MAXN, hipMemcpyHostToDevice));
      PCCHK (d, hipMemcpy (d->tab.d_ped + 5 * PCS_MAXN + 8, d->h_sex, PCS_MAXN, hipMemcpyHostToDevice));
      d->ped_haploid = haploid;
    }
  return 0;
}

// the per-site caller in three steps (host -> device, kernel, device -> host), so that the kernel can be timed on resident
// columns; pecall_dev_call_sites is the three in a row
extern "C" int pecall_dev_sites_stage (pecall_dev * d, const uint16_t * reads, const uint8_t * ref_base, const uint8_t * chrom_type, long n_sites,
                                       int indiv)
{
  PCCHK (d, hipSetDevice (d->device));
  if (n_sites <= 0 || indiv <= 0 || indiv > PCS_MAXN)
    return pc_fail (d, "call_sites: n_sites %ld, indiv %d (1..%d samples per call)", n_sites, indiv, PCS_MAXN);
  d->result_sites = 0;
  PCTRY (pcs_ensure (d, n_sites, indiv));
  long items = n_sites * indiv;
  PCCHK (d, hipMemcpyAsync (d->cols.d_sreads, reads, items * PCS_NA * sizeof (uint16_t), hipMemcpyHostToDevice, d->stream));
  PCCHK (d, hipMemcpyAsync (d->cols.d_dom, ref_base, n_sites, hipMemcpyHostToDevice, d->stream));
  if (chrom_type)
    PCCHK (d, hipMemcpyAsync (d->cols.d_chromy, chrom_type, n_sites, hipMemcpyHostToDevice, d->stream));
  else
    PCCHK (d, hipMemsetAsync (d->cols.d_chromy, 0, n_sites, d->stream));
  PCCHK (d, hipStreamSynchronize (d->stream));
  d->staged_sites = n_sites;
  d->staged_indiv = indiv;
  return 0;
}

// the parameter block of a call, after the checks the reference makes on its command line
static int pcs_params (pecall_dev * d, int indiv, int haploid, double threshold, double theta, PcsParams & P)
{
  if (!(theta >= 1e-10 && theta <= 0.5))
    return pc_fail (d, "call_sites: theta %g outside [1e-10, 0.5] (pecaller.c:305-309)", theta);
  if (d->ped_indiv && d->ped_indiv != indiv)
    return pc_fail (d, "call_sites: the pedigree was set for %d samples, this call has %d", d->ped_indiv, indiv);
  if (d->ped_indiv && d->denovo_rate > theta)
    return pc_fail (d, "call_sites: de-novo mutation rate %g above theta %g (pecaller.c:381-385)", d->denovo_rate, theta);
  if (d->ped_indiv)
    PCTRY (pcs_ensure_ped (d, haploid ? 1 : 0));
  P.indiv = indiv;
  P.haploid = haploid ? 1 : 0;
  P.max_gen = haploid ? 6 : PCS_NG;     // pecaller.c:326-336
  P.min_depth = haploid ? 1 : 2;
  P.threshold = threshold;
  P.ln_theta = log (theta);
  P.tab = d->tab.d_tab;
  P.hw = d->tab.d_hw;
  P.hw_off = d->tab.d_hw_off;
  P.use_ped = d->ped_indiv ? 1 : 0;
  P.ln_denovo = d->ped_indiv ? log (d->denovo_rate) : 0.0;
  P.dad = d->tab.d_ped;
  P.mom = d->tab.d_ped + PCS_MAXN;
  P.kid_off = (const uint16_t *) (d->tab.d_ped + 2 * PCS_MAXN);
  P.kid_list = (const uint16_t *) (d->tab.d_ped + 3 * PCS_MAXN + 8);
  P.sex = (const int8_t *) (d->tab.d_ped + 5 * PCS_MAXN + 8);
  P.dyad = d->tab.d_dyad;
  P.trio = d->tab.d_trio;
  return 0;
}

// streams, per-chunk events and counters for n_sites columns
static int pcs_ensure_chunks (pecall_dev * d, long n_sites)
{
  if (!d->stream_h2d)
    {
      for (int i = 0; i < PCS_CALL_STREAMS; i++)
        // (a stream priority for the beam searches was tried: 64 -> 60 M columns/s, the shortcut kernels wait for them then)
        PCCHK (d, hipStreamCreateWithFlags (&d->stream_call[i], hipStreamNonBlocking));
      // Which streams share one of the runtime's 4 hardware queues (per priority level) is settled when they are made and depends on every
      // stream the process made before: with the early beam search's stream on the queue of the shortcut kernels' stream a resident run of
      // 2 M columns took 23.4 ms instead of 19.2, with a copy stream on a beam-search stream's queue the seam did 25 M columns/s instead
      // of 43 -- the FIRST object of a process had the one, every later object the other (profiles/r04_ab_sweeps.txt; the order the
      // streams are first used in changes nothing).  Streams of another priority take queues of their own: the copies' streams high,
      // the early beam search's low, the shortcut kernels' and the chunks' beam searches' streams at the default.
      int prio_low = 0, prio_high = 0;
      PCCHK (d, hipDeviceGetStreamPriorityRange (&prio_low, &prio_high));
      if (d->kn.flat_priorities)
        prio_low = prio_high = 0;
      PCCHK (d, hipStreamCreateWithPriority (&d->stream_h2d, hipStreamNonBlocking, prio_high));
      PCCHK (d, hipStreamCreateWithPriority (&d->stream_d2h, hipStreamNonBlocking, prio_high));
      PCCHK (d, hipStreamCreateWithPriority (&d->stream_heavy, hipStreamNonBlocking, prio_low));
      PCCHK (d, hipEventCreateWithFlags (&d->ev_heavy[0], hipEventDisableTiming));
      PCCHK (d, hipEventCreateWithFlags (&d->ev_heavy[1], hipEventDisableTiming));
      PCCHK (d, hipFuncSetAttribute ((const void *) pcs_fast_kernel < PC_TABLE, 1 >, hipFuncAttributeMaxDynamicSharedMemorySize, PCS_FAST_LDS_BYTES_OF (PC_TABLE)));
      PCCHK (d, hipFuncSetAttribute ((const void *) pcs_fast_kernel < PC_TABLE, 2 >, hipFuncAttributeMaxDynamicSharedMemorySize, PCS_FAST_LDS_BYTES_OF (PC_TABLE)));
      PCCHK (d, hipFuncSetAttribute ((const void *) pcs_call_kernel < 4 >, hipFuncAttributeMaxDynamicSharedMemorySize, (int) sizeof (PcsShared < 4 >)));
      PCCHK (d, hipFuncSetAttribute ((const void *) pcs_call_kernel < 8 >, hipFuncAttributeMaxDynamicSharedMemorySize, (int) sizeof (PcsShared < 8 >)));
    }
  const size_t nch = (size_t) ((n_sites + d->chunk_sites - 1) / d->chunk_sites);
  if (nch > d->cap_chunks)
    {
      PCCHK (d, hipDeviceSynchronize ());
      pc_free (d->d_chunk_ctr, d->d_heavy_ctr);
      pc_host_free (d->h_ctrs);
      PCCHK (d, hipMalloc ((void **) &d->d_chunk_ctr, nch * PCS_CTRS * sizeof (unsigned long long)));
      PCCHK (d, hipMalloc ((void **) &d->d_heavy_ctr, (nch + 1) * PCS_CTRS * sizeof (unsigned long long)));
      PCCHK (d, hipHostMalloc ((void **) &d->h_ctrs, (pcs_sparse_len_at (nch) + 1) * sizeof (unsigned long long), hipHostMallocDefault));
      d->chunks.resize (std::max (nch, d->chunks.size ()), PcsChunk { });        // (a call that failed in here left chunks without events: the missing ones are made)
      for (PcsChunk & c : d->chunks)
        for (hipEvent_t * e : { &c.h2d, &c.fast, &c.call, &c.d2h, &c.heavy })
          if (!*e)
            PCCHK (d, hipEventCreateWithFlags (e, hipEventDisableTiming));
      d->cap_chunks = nch;
    }
  return 0;
}

static int pcs_n_chunks (const pecall_dev * d)
{
  return (int) ((d->staged_sites + d->chunk_sites - 1) / d->chunk_sites);
}

// the column arrays of the staged columns [off, off + m), as the kernels and the seam's copies take them
struct PcsView
{
  long off, m;
  uint16_t *reads;
  uint8_t *dom, *chromy, *heavy_flag;
  int8_t *call, *type, *npass;
  double *post;
  int32_t *ac, *den;
  unsigned *slow, *deep, *heavy_list;
};

static PcsView pcs_view (pecall_dev * d, long off, long m)
{
  const PcsColumns & c = d->cols;
  const long N = d->staged_indiv;
  return { off, m, c.d_sreads + off * N * PCS_NA, c.d_dom + off, c.d_chromy + off, c.d_heavy_flag + off, c.d_call + off * N, c.d_type + off, c.d_npass + off,
    c.d_post + off * N, c.d_ac + off * PCS_NA, c.d_den + off, c.d_slow + (size_t) PCS_BUCKETS * off, c.d_deep + off, c.d_heavy_list + (size_t) PCS_BUCKETS * off };
}

static PcsView pcs_chunk_view (pecall_dev * d, int k)
{
  const long off = (long) k * d->chunk_sites, left = d->staged_sites - off;
  return pcs_view (d, off, left < d->chunk_sites ? left : d->chunk_sites);
}

// The beam search (pcs_call_kernel) of the columns of `list` -- PCS_BUCKETS parts whose lengths stand in `ctr`, heaviest part first -- on
// stream s with at most `waves` waves; `scratch` holds a wave's scratch for each of them.  A lane stands for a sample of each chunk of 64.
static void pcs_beam_search (const PcsParams & P, const PcsView & v, hipStream_t s, char *scratch, unsigned long long *ctr, const unsigned *list, long waves)
{
  static const decltype (&pcs_call_kernel < 1 >) kernel[4] = { pcs_call_kernel < 1 >, pcs_call_kernel < 2 >, pcs_call_kernel < 4 >, pcs_call_kernel < 8 > };
  // (257 .. 512 samples: 124 KB of LDS, one wave per CU at a time)
  static const size_t lds[4] = { sizeof (PcsShared < 1 >), sizeof (PcsShared < 2 >), sizeof (PcsShared < 4 >), sizeof (PcsShared < 8 >) };
  const int nch = pcs_sample_chunks (P.indiv), i = nch == 8 ? 3 : nch / 2;
  hipLaunchKernelGGL (kernel[i], dim3 ((unsigned) (v.m < waves ? v.m : waves)), dim3 (64), lds[i], s, P, v.reads, v.dom, v.chromy, v.m, v.call, v.post, v.type,
                      v.ac, v.npass, v.den, scratch, ctr, list, (const unsigned *) (ctr + PCS_CTR_LISTED));
}

// pcs_heavy_kernel over the columns of v on the object's stream, then -- on stream hs, with scratch of its own for `waves` waves -- the
// beam search of what it listed, heaviest part first; `done` closes it.  slot: the list's counters (0: a whole run, 1 + k: chunk k).
static int pcs_heavy_start (pecall_dev * d, const PcsParams & P, const PcsView & v, int slot, hipEvent_t done, hipStream_t hs, char *scratch, long waves)
{
  unsigned long long *ctr = pcs_heavy_ctrs (d, slot);
  PCCHK (d, hipMemsetAsync (ctr, 0, PCS_CTRS * sizeof (unsigned long long), d->stream));
  PCCHK (d, hipMemsetAsync (v.heavy_flag, 0, (size_t) v.m, d->stream));
  const long hgrid = std::min ((v.m + 3) / 4, (long) d->grid * 4);
  hipLaunchKernelGGL (pcs_heavy_kernel, dim3 ((unsigned) hgrid), dim3 (256), 0, d->stream, v.reads, v.dom, v.m, P.indiv, pcs_heavy_min (d, P.indiv), v.heavy_list,
                      (unsigned *) (ctr + PCS_CTR_LISTED), v.heavy_flag);
  PCCHK (d, hipEventRecord (d->ev_heavy[0], d->stream));
  PCCHK (d, hipStreamWaitEvent (hs, d->ev_heavy[0], 0));
  pcs_beam_search (P, v, hs, scratch, ctr, v.heavy_list, waves);
  PCCHK (d, hipGetLastError ());
  PCCHK (d, hipEventRecord (done, hs));
  return 0;
}

// Chunk k: the shortcut kernel (with the small beam) on the object's stream, and the beam search of the columns it lists on one of
// PCS_CALL_STREAMS streams, so that it runs beside the next chunks' shortcut kernels.  (The chunk's counters are zero: the callers see to it.)
// The shortcut kernel has two forms: the head of the ln n! table in LDS (three workgroups per CU), or the whole table (one per CU).
// Which one a column needs depends on its deepest sample.  Nothing here waits for the device: the form with the table's head runs
// over every chunk and puts the columns that are too deep for it -- beyond ~1,400 reads in one sample, rare -- on a list of the chunk;
// the host looks at the lists' lengths once, when all chunks are through, and gives the chunks with a list a second pass
// (whole_table = true: the other form over the listed columns, and the beam search of what that lists).
// (History: a kernel of its own looked for the deepest sample of a chunk first, 0.12 ms and the chunk's 200 MB a second time per
// chunk; before that the host waited for each chunk's depth, which cost the seam half its rate -- the 4-byte copy queued behind
// the chunks' 150 MB copies.)
// heavy: 0 no early beam search; 1 the run made its list already (pcs_heavy_start over all columns): the shortcut kernel passes the flagged
// columns over; 2 the chunk makes its own list here (the seam: columns arrive chunk by chunk) and its results wait for that beam search too
static int pcs_chunk_kernels (pecall_dev * d, const PcsParams & P, int k, bool whole_table, bool sparse, int heavy)
{
  const PcsView v = pcs_chunk_view (d, k);
  const PcsChunk & ev = d->chunks[k];
  unsigned long long *ctr = pcs_chunk_ctrs (d, k);
  unsigned *n_slow = (unsigned *) (ctr + PCS_CTR_LISTED), *n_deep = (unsigned *) (ctr + PCS_CTR_DEEP), *next_piece = (unsigned *) (ctr + PCS_CTR_PIECE);
  const int N = P.indiv, nch = pcs_sample_chunks (N);
  // (a chunk lists a few hundred columns for the beam search, a handful of them heavy -- milliseconds on one wave: behind each other
  // on one stream the chunks' searches were the caller's time, 8 x 5.5 ms.  They alternate on PCS_CALL_STREAMS streams.)
  const int share = k % PCS_CALL_STREAMS;
  hipStream_t sc = d->stream_call[share];
  const long cgrid = d->scratch.site_grid / PCS_CALL_STREAMS;
  // (second pass: behind the first pass's beam search of the chunk, which shares these counters; the deep list's length stays)
  if (whole_table)
    {
      PCCHK (d, hipStreamWaitEvent (d->stream, ev.call, 0));
      PCCHK (d, hipMemsetAsync (ctr, 0, PCS_CTR_DEEP * sizeof (unsigned long long), d->stream));
      PCCHK (d, hipMemsetAsync (ctr + PCS_CTR_PIECE, 0, sizeof (unsigned long long), d->stream));
    }
  if (heavy == 2 && !whole_table)
    {
      // (on the chunk's own beam-search stream, in front of the search of what the shortcut kernel lists: the chunks' early searches
      // then alternate on PCS_CALL_STREAMS streams like the others -- on the one stream of the resident form they ran one behind the
      // other, 8 x 5 ms, and every chunk's results waited for its own)
      PCTRY (pcs_heavy_start (d, P, v, 1 + k, ev.heavy, sc, pcs_scratch_share (d, share, N), cgrid));
    }
  if (whole_table && nch > 2)
    return 0;                   // (more than 128 samples: no second pass, a column too deep for the table's head was listed for the beam search)
  // the shortcut kernel: a lane per sample up to 64 samples, two samples per lane up to 128 (round 4); beyond that a chunk of 64
  // samples at a time, the unsettled samples' likelihoods parked in LDS for the small beam: what it cannot write goes to the beam
  // search's list (no second pass with the whole table: too deep = listed)
  typedef decltype (&pcs_fast_kernel < PCS_FAST_TAB, 1 >) fast_kernel_t;
  static const fast_kernel_t head[4] = { pcs_fast_kernel < PCS_FAST_TAB, 1 >, pcs_fast_kernel < PCS_FAST_TAB, 2 >, pcs_fast_kernel < PCS_FAST_TAB, 4 >,
    pcs_fast_kernel < PCS_FAST_TAB, 8 > };
  static const fast_kernel_t whole[2] = { pcs_fast_kernel < PC_TABLE, 1 >, pcs_fast_kernel < PC_TABLE, 2 > };
  const int tab = whole_table ? PC_TABLE : PCS_FAST_TAB, B = PCS_FAST_BLOCK_OF (tab);
  // the table's head: three workgroups of 4 waves per CU (two with two samples per lane: the registers); the whole ln n! table takes half
  // a CU's LDS: one workgroup per CU
  const long cap = whole_table ? d->grid / 2 : nch == 1 ? (long) d->grid / 2 * 3 : (long) d->grid;
  const long fgrid = std::min ((v.m + B / 64 - 1) / (B / 64), cap);
  hipLaunchKernelGGL ((whole_table ? whole : head)[nch == 8 ? 3 : nch / 2], dim3 ((unsigned) fgrid), dim3 (B), PCS_FAST_LDS_BYTES_OF2 (tab, nch), d->stream, P, v.reads,
                      v.dom, v.chromy, v.m, v.call, v.post, v.type, v.ac, v.npass, v.den, v.slow, n_slow, v.deep, n_deep, next_piece, d->tab.d_ta,
                      heavy ? (const uint8_t *) v.heavy_flag : (const uint8_t *) nullptr);
  // (the beam search's kernel takes the columns the shortcut kernel listed)
  PCCHK (d, hipEventRecord (ev.fast, d->stream));
  PCCHK (d, hipStreamWaitEvent (sc, ev.fast, 0));
  pcs_beam_search (P, v, sc, pcs_scratch_share (d, share, N), ctr, v.slow, cgrid);
  if (heavy == 2)
    PCCHK (d, hipStreamWaitEvent (sc, ev.heavy, 0));    // (the chunk's results are whole when its early beam search is through too)
  if (sparse)
    {
      // behind the beam search, on its stream: the chunk's columns with a posterior that is not 1 (second pass: of the deep list only)
      const long sgrid = whole_table ? d->grid : std::min ((v.m + 3) / 4, (long) d->grid * 4);
      hipLaunchKernelGGL (pcs_sparse_kernel, dim3 ((unsigned) (sgrid > 0 ? sgrid : 1)), dim3 (256), 0, sc, v.post, v.m,
                          whole_table ? (const unsigned *) v.deep : (const unsigned *) nullptr, (const unsigned *) n_deep, N, (unsigned) v.off, d->sp.d_cols, d->sp.d_rows,
                          d->sp.cap, d->sp.d_n);
    }
  PCCHK (d, hipGetLastError ());
  PCCHK (d, hipEventRecord (ev.call, sc));
  return 0;
}

// the chunks whose depth asks for the whole table (to be called when the first pass is through on the device)
static int pcs_deep_chunks (pecall_dev * d, const PcsParams & P, int nch, std::vector < int >&deep)
{
  if (P.indiv > 128)
    return 0;                   // (no shortcut kernel, no deep list)
  // (into page-locked memory of the object's own: a pageable target that shares a page with an array the caller registered is refused)
  PCCHK (d, hipMemcpy (d->h_ctrs, d->d_chunk_ctr, (size_t) nch * PCS_CTRS * sizeof (unsigned long long), hipMemcpyDeviceToHost));
  for (int k = 0; k < nch; k++)
    if ((unsigned) d->h_ctrs[(size_t) k * PCS_CTRS + PCS_CTR_DEEP] > 0u)
      deep.push_back (k);
  return 0;
}

// PECALL_LIST_STATS: how many columns the shortcut left to the beam search, by part of the list
static void pcs_list_stats (pecall_dev * d, int nch, bool heavy)
{
  unsigned long long tot[PCS_BUCKETS] = { 0ull, 0ull, 0ull, 0ull };
  for (int q = 0; q < nch; q++)
    {
      unsigned c[PCS_BUCKETS];
      if (hipMemcpy (c, pcs_chunk_ctrs (d, q) + PCS_CTR_LISTED, sizeof c, hipMemcpyDeviceToHost) == hipSuccess)
        for (int b = 0; b < PCS_BUCKETS; b++)
          tot[b] += c[b];
    }
  fprintf (stderr, "[pecall] %ld columns, listed for the beam by unsettled samples <3 / <8 / <20 / more: %llu %llu %llu %llu\n", d->staged_sites, tot[0], tot[1], tot[2], tot[3]);
#ifdef PECALL_TIMING_PROBES
  {
    // the beam search's phase probes (pecall_site.hip.h): wave cycles summed over the run's launches
    (void) hipDeviceSynchronize ();
    unsigned long long pr[16], z[16] = { 0ull };
    if (hipMemcpyFromSymbol (pr, HIP_SYMBOL (pcs_probe), sizeof pr) == hipSuccess)
      {
        static const char *nm[13] = { "set-up, likelihoods, re-estimation", "expand: duplicates", "expand: pricing", "expand: acceptance + rows", "clean: sort", "clean: end",
          "below-floor samples", "posteriors + marginals", "before write", "write", "clean: cut + homozygous?", "clean: fallback's configuration", "clean: its sort" };
        double tot_c = 0;
        for (int i = 0; i < 13; i++)
          tot_c += (double) pr[i];
        fprintf (stderr, "[pcs_probe]");
        for (int i = 0; i < 13; i++)
          fprintf (stderr, " %s %.1f%%", nm[i], tot_c > 0 ? 100.0 * (double) pr[i] / tot_c : 0.0);
        fprintf (stderr, " | total %.3f G wave-cycles\n", tot_c / 1e9);
        (void) hipMemcpyToSymbol (HIP_SYMBOL (pcs_probe), z, sizeof z);
      }
  }
#endif
  unsigned hc[PCS_BUCKETS] = { 0u, 0u, 0u, 0u };
  if (heavy && hipMemcpy (hc, pcs_heavy_ctrs (d, 0) + PCS_CTR_LISTED, sizeof hc, hipMemcpyDeviceToHost) == hipSuccess)
    fprintf (stderr, "[pecall] started ahead of the shortcut kernels, by samples with variant reads <12 / <20 / <32 / more: %u %u %u %u\n", hc[0], hc[1], hc[2], hc[3]);
}

// the object's stream ends behind every chunk's beam search and the early one: ev_site[1] closes the interval of all streams
static int pcs_run_join (pecall_dev * d, int nch, bool heavy)
{
  for (int q = 0; q < nch; q++)
    PCCHK (d, hipStreamWaitEvent (d->stream, d->chunks[q].call, 0));
  if (heavy)
    PCCHK (d, hipStreamWaitEvent (d->stream, d->ev_heavy[1], 0));
  PCCHK (d, hipEventRecord (d->ev_site[1], d->stream));
  PCCHK (d, hipStreamSynchronize (d->stream));
  return 0;
}

extern "C" int pecall_dev_sites_run (pecall_dev * d, int haploid, double threshold, double theta, float *kernel_ms)
{
  PCCHK (d, hipSetDevice (d->device));
  const int indiv = d->staged_indiv;
  if (d->staged_sites <= 0)
    return pc_fail (d, "sites_run: nothing staged");
  d->result_sites = 0;
  d->run_stats_sites = 0;
  PcsParams P;
  PCTRY (pcs_params (d, indiv, haploid, threshold, theta, P));
  PCTRY (pcs_ensure_chunks (d, d->staged_sites));
  PCCHK (d, hipEventRecord (d->ev_site[0], d->stream));
  const int nch = pcs_n_chunks (d);
  // the long beam searches first (pcs_heavy_kernel): listed from the resident columns, started on a stream of their own beside everything
  // that follows -- a launch of the beam search ends with its slowest column, and the last chunk's used to be the run's last 8 ms
  const bool heavy = pcs_heavy_min (d, indiv) > 0;
  if (heavy)
    PCTRY (pcs_heavy_start (d, P, pcs_view (d, 0, d->staged_sites), 0, d->ev_heavy[1], d->stream_heavy, pcs_scratch_share (d, PCS_CALL_STREAMS, indiv),
                            d->scratch.heavy_grid));
  // (the counters of all chunks first)
  for (int q = 0; q < nch; q++)
    PCCHK (d, hipMemsetAsync (pcs_chunk_ctrs (d, q), 0, PCS_CTRS * sizeof (unsigned long long), d->stream));
  for (int q = 0; q < nch; q++)
    PCTRY (pcs_chunk_kernels (d, P, q, false, false, heavy ? 1 : 0));
  PCTRY (pcs_run_join (d, nch, heavy));
  std::vector < int >deep;
  PCTRY (pcs_deep_chunks (d, P, nch, deep));
  for (int b = 0; b < PCS_BUCKETS; b++)
    d->run_listed_first[b] = 0ull;
  d->run_heavy = heavy;
  if (!deep.empty ())
    {
      // (deep chunks: the second pass is part of the run; its interval ends behind it.  It clears the chunk's counts of listed columns, which
      // pcs_deep_chunks has just brought to the host: kept for pecall_dev_sites_stats)
      for (int q : deep)
        for (int b = 0; b < PCS_BUCKETS; b++)
          d->run_listed_first[b] += ((const unsigned *) (d->h_ctrs + (size_t) q * PCS_CTRS + PCS_CTR_LISTED))[b];
      for (int q : deep)
        PCTRY (pcs_chunk_kernels (d, P, q, true, false, heavy ? 1 : 0));
      PCTRY (pcs_run_join (d, nch, heavy));
    }
  if (kernel_ms)
    PCCHK (d, hipEventElapsedTime (kernel_ms, d->ev_site[0], d->ev_site[1]));
  if (getenv ("PECALL_LIST_STATS"))
    pcs_list_stats (d, nch, heavy);
  d->result_sites = d->staged_sites;
  d->run_stats_sites = d->staged_sites;
  return 0;
}

// what PECALL_LIST_STATS prints, as numbers (the layout is described at the declaration)
extern "C" int pecall_dev_sites_stats (pecall_dev * d, uint64_t * out)
{
  PCCHK (d, hipSetDevice (d->device));
  if (!out)
    return pc_fail (d, "sites_stats: no array");
  if (d->staged_sites <= 0 || d->result_sites != d->staged_sites || d->run_stats_sites != d->staged_sites)
    return pc_fail (d, "sites_stats: valid after sites_run only");
  const int nch = pcs_n_chunks (d);
  for (int i = 0; i < 2 + 2 * PCS_BUCKETS; i++)
    out[i] = 0;
  out[0] = (uint64_t) d->staged_sites;
  PCCHK (d, hipMemcpy (d->h_ctrs, d->d_chunk_ctr, (size_t) nch * PCS_CTRS * sizeof (unsigned long long), hipMemcpyDeviceToHost));
  for (int q = 0; q < nch; q++)
    {
      const unsigned *c = (const unsigned *) (d->h_ctrs + (size_t) q * PCS_CTRS + PCS_CTR_LISTED);
      for (int b = 0; b < PCS_BUCKETS; b++)
        out[1 + b] += c[b];
      out[1 + PCS_BUCKETS] += (unsigned) d->h_ctrs[(size_t) q * PCS_CTRS + PCS_CTR_DEEP];
    }
  for (int b = 0; b < PCS_BUCKETS; b++)
    out[1 + b] += d->run_listed_first[b];
  if (d->run_heavy)
    {
      unsigned hc[PCS_BUCKETS];
      PCCHK (d, hipMemcpy (hc, pcs_heavy_ctrs (d, 0) + PCS_CTR_LISTED, sizeof hc, hipMemcpyDeviceToHost));
      for (int b = 0; b < PCS_BUCKETS; b++)
        out[2 + PCS_BUCKETS + b] = hc[b];
    }
  return 0;
}

extern "C" int pecall_dev_sites_collect (pecall_dev * d, int8_t * call, double *posterior, int8_t * site_type, int32_t * allele_count,
                                         int8_t * n_pass, int32_t * denovo)
{
  PCCHK (d, hipSetDevice (d->device));
  const long n_sites = d->staged_sites;
  const long items = n_sites * d->staged_indiv;
  if (n_sites <= 0)
    return pc_fail (d, "sites_collect: nothing staged");
  PCCHK (d, hipMemcpyAsync (call, d->cols.d_call, items, hipMemcpyDeviceToHost, d->stream));
  PCCHK (d, hipMemcpyAsync (posterior, d->cols.d_post, items * sizeof (double), hipMemcpyDeviceToHost, d->stream));
  if (site_type)
    PCCHK (d, hipMemcpyAsync (site_type, d->cols.d_type, n_sites, hipMemcpyDeviceToHost, d->stream));
  if (allele_count)
    PCCHK (d, hipMemcpyAsync (allele_count, d->cols.d_ac, n_sites * PCS_NA * sizeof (int32_t), hipMemcpyDeviceToHost, d->stream));
  if (n_pass)
    PCCHK (d, hipMemcpyAsync (n_pass, d->cols.d_npass, n_sites, hipMemcpyDeviceToHost, d->stream));
  if (denovo)
    PCCHK (d, hipMemcpyAsync (denovo, d->cols.d_den, n_sites * sizeof (int32_t), hipMemcpyDeviceToHost, d->stream));
  PCCHK (d, hipStreamSynchronize (d->stream));
  return 0;
}

extern "C" int pecall_dev_pin_host (pecall_dev * d, const void *host_ptr, uint64_t n_bytes)
{
  PCCHK (d, hipSetDevice (d->device));
  if (!host_ptr || !n_bytes)
    return pc_fail (d, "pin_host: empty range");
  if (!pm_host_pin_range (host_ptr, (size_t) n_bytes, d->stream_h2d))
    return pc_fail (d, "pin_host: hipHostRegister of %llu bytes failed", (unsigned long long) n_bytes);
  return 0;
}

extern "C" int pecall_dev_unpin_host (pecall_dev * d, const void *host_ptr)
{
  PCCHK (d, hipSetDevice (d->device));
  if (d->stream_h2d)
    {
      PCCHK (d, hipStreamSynchronize (d->stream_h2d));
      PCCHK (d, hipStreamSynchronize (d->stream_d2h));
    }
  const int rc = pm_host_unpin (host_ptr);
  if (rc == 1)
    return pc_fail (d, "unpin_host: %p is not inside a range pinned through pecall_dev_pin_host", host_ptr);
  if (rc == 2)
    return pc_fail (d, "unpin_host: hipHostUnregister failed");
  return 0;
}

// The seam: host columns in, calls and posteriors out.  The columns travel in chunks: the host-to-device copy of chunk k + 1, the
// kernels of chunk k and the device-to-host copy of chunk k - 1 run side by side (three streams behind each other through events).
// Buffers the caller pinned (pecall_dev_pin_host) are copied from and to directly; others pass through PCS_SLOTS pinned staging
// buffers, filled and emptied by a few host threads (one core moves ~10 GB/s; a 64-sample column is 768 bytes in, ~620 out).

struct PcsIo
{
  const uint16_t *reads;
  const uint8_t *ref_base, *chrom_type;
  int8_t *call;                 // (the results in the order of pecall_dev_call_sites' arguments)
  double *posterior;
  int8_t *site_type;
  int32_t *allele_count;
  int8_t *n_pass;
  int32_t *denovo;
  // sparse = the posteriors come back as the list of the columns in which one differs from 1 (post_site / post_rows / post_cap / n_post)
  // instead of the dense array `posterior`
  bool sparse;
  uint32_t *post_site;
  double *post_rows;
  uint64_t post_cap;
  uint64_t *n_post;
  bool resident;                // the columns are on the device already (pecall_dev_sites_stage_records): no host arrays, no host-to-device copies
  bool in_direct, out_direct;   // every input / every result array lies in a range the caller pinned
};

static int pcs_ensure_sparse (pecall_dev * d, unsigned long long post_cap, int indiv)
{
  PcsSparse & s = d->sp;
  if (s.cap >= post_cap && s.indiv >= indiv)
    return 0;
  PCCHK (d, hipDeviceSynchronize ());
  pc_free (s.d_cols, s.d_rows);
  s.cap = 0;                    // (and so the list is made for post_cap rows, also where that is fewer than it had)
  const int wide = indiv > s.indiv ? indiv : s.indiv;
  PCCHK (d, hipMalloc ((void **) &s.d_cols, (size_t) post_cap * sizeof (unsigned)));
  PCCHK (d, hipMalloc ((void **) &s.d_rows, (size_t) post_cap * (size_t) wide * sizeof (double)));
  if (!s.d_n)
    PCCHK (d, hipMalloc ((void **) &s.d_n, sizeof (unsigned long long)));
  s.cap = post_cap;
  s.indiv = wide;
  return 0;
}

// PCS_SLOTS page-locked buffers of `bytes` each, made when `need` is more than they have
static int pcs_ensure_slots (pecall_dev * d, char *(&slot)[PCS_SLOTS], size_t &have, size_t need, size_t bytes)
{
  if (have >= need)
    return 0;
  have = 0;
  for (int i = 0; i < PCS_SLOTS; i++)
    {
      pc_host_free (slot[i]);
      PCCHK (d, hipHostMalloc ((void **) &slot[i], bytes, hipHostMallocDefault));
    }
  have = bytes;
  return 0;
}

// a chunk's results in the order of their staging layout ([call][posterior][type][passes][allele counts][de-novo]); big = never NULL, copied by threads
struct PcsResult
{
  char *host;
  const void *dev;
  size_t bytes;
  bool big;
};

static int pcs_results (const PcsIo & io, const PcsView & v, size_t N, PcsResult (&r)[6])
{
  const size_t m = (size_t) v.m, off = (size_t) v.off;
  int n = 0;
  r[n++] = { (char *) (io.call + off * N), v.call, m * N, true };
  if (!io.sparse)
    r[n++] = { (char *) (io.posterior + off * N), v.post, m * N * 8, true };
  r[n++] = { io.site_type ? (char *) (io.site_type + off) : nullptr, v.type, m, false };
  r[n++] = { io.n_pass ? (char *) (io.n_pass + off) : nullptr, v.npass, m, false };
  r[n++] = { io.allele_count ? (char *) (io.allele_count + off * PCS_NA) : nullptr, v.ac, m * PCS_NA * 4, false };
  r[n++] = { io.denovo ? (char *) (io.denovo + off) : nullptr, v.den, m * 4, false };
  return n;
}

// chunk k's columns on their way to the device (staging layout of a chunk of m columns: [reads][ref][chrom]).  A staging slot is free again
// when the chunk that used it PCS_SLOTS chunks ago has been copied to the device.
static int pcs_stage_in (pecall_dev * d, const PcsIo & io, int k, const PcsView & v, size_t N)
{
  const size_t m = (size_t) v.m;
  const uint16_t *src_r = io.reads + v.off * N * PCS_NA;
  const uint8_t *src_b = io.ref_base + v.off, *src_c = io.chrom_type ? io.chrom_type + v.off : nullptr;
  if (!io.in_direct)
    {
      if (k >= PCS_SLOTS)
        PCCHK (d, hipEventSynchronize (d->chunks[k - PCS_SLOTS].h2d));
      char *st = d->h_in[k % PCS_SLOTS];
      pm_par_memcpy (st, (const char *) src_r, m * N * PCS_NA * 2);
      src_r = (const uint16_t *) st;
      st += m * N * PCS_NA * 2;
      memcpy (st, src_b, m);
      src_b = (const uint8_t *) st;
      st += m;
      if (src_c)
        {
          memcpy (st, src_c, m);
          src_c = (const uint8_t *) st;
        }
    }
  PCCHK (d, hipMemcpyAsync (v.reads, src_r, m * N * PCS_NA * 2, hipMemcpyHostToDevice, d->stream_h2d));
  PCCHK (d, hipMemcpyAsync (v.dom, src_b, m, hipMemcpyHostToDevice, d->stream_h2d));
  if (src_c)
    PCCHK (d, hipMemcpyAsync (v.chromy, src_c, m, hipMemcpyHostToDevice, d->stream_h2d));
  else
    PCCHK (d, hipMemsetAsync (v.chromy, 0, m, d->stream_h2d));
  return 0;
}

// chunk j's kernels, and its results on their way out behind its beam search (which follows its shortcut kernel)
static int pcs_queue_chunk (pecall_dev * d, const PcsParams & P, const PcsIo & io, int j, bool whole_table)
{
  if (!whole_table)
    PCCHK (d, hipMemsetAsync (pcs_chunk_ctrs (d, j), 0, PCS_CTRS * sizeof (unsigned long long), d->stream));
  PCTRY (pcs_chunk_kernels (d, P, j, whole_table, io.sparse, pcs_heavy_min (d, P.indiv) > 0 ? 2 : 0));
  PCCHK (d, hipStreamWaitEvent (d->stream_d2h, d->chunks[j].call, 0));
  PcsResult r[6];
  const int n = pcs_results (io, pcs_chunk_view (d, j), (size_t) P.indiv, r);
  size_t at = 0;                // (in the staging slot)
  for (int i = 0; i < n; at += r[i].bytes, i++)
    if (char *dst = io.out_direct ? r[i].host : d->h_out[j % PCS_SLOTS] + at)
      PCCHK (d, hipMemcpyAsync (dst, r[i].dev, r[i].bytes, hipMemcpyDeviceToHost, d->stream_d2h));
  PCCHK (d, hipEventRecord (d->chunks[j].d2h, d->stream_d2h));
  return 0;
}

// chunk j's results are on the host: from the staging slot to the caller's arrays
static int pcs_hand_over (pecall_dev * d, const PcsIo & io, int j)
{
  PCCHK (d, hipEventSynchronize (d->chunks[j].d2h));
  if (io.out_direct)
    return 0;
  PcsResult r[6];
  const int n = pcs_results (io, pcs_chunk_view (d, j), (size_t) d->staged_indiv, r);
  const char *o = d->h_out[j % PCS_SLOTS];
  for (int i = 0; i < n; o += r[i].bytes, i++)
    if (r[i].big)
      pm_par_memcpy (r[i].host, o, r[i].bytes);
    else if (r[i].host)
      memcpy (r[i].host, o, r[i].bytes);
  return 0;
}

// the sparse list to the caller: the listed columns in ascending order of their numbers (the kernels appended them as they came)
static int pcs_collect_sparse (pecall_dev * d, const PcsIo & io, size_t N)
{
  unsigned long long *len = d->h_ctrs + pcs_sparse_len_at (d->cap_chunks);
  PCCHK (d, hipMemcpy (len, d->sp.d_n, sizeof (unsigned long long), hipMemcpyDeviceToHost));
  const unsigned long long n = *len;
  *io.n_post = n;
  if (n > io.post_cap)
    return pc_fail (d, "call_sites_sparse: %llu columns have a posterior that is not 1, the list holds %llu (n_post says how many are needed)", n,
                    (unsigned long long) io.post_cap);
  if (n == 0)
    return 0;
  // (through a page-locked block of this call's own: a copy into pageable memory that shares a page with one of the caller's
  // registered arrays is refused by the runtime -- tools/micro/hostreg.hip -- and a small heap block may well do that)
  char *blk = nullptr;
  const size_t rows_bytes = (size_t) n * N * sizeof (double), cols_bytes = ((size_t) n * sizeof (unsigned) + 63) & ~(size_t) 63;
  PCCHK (d, hipHostMalloc ((void **) &blk, rows_bytes + cols_bytes, hipHostMallocDefault));
  const double *rows = (const double *) blk;
  const unsigned *cols = (const unsigned *) (blk + rows_bytes);
  hipError_t e1 = hipMemcpy ((void *) cols, d->sp.d_cols, (size_t) n * sizeof (unsigned), hipMemcpyDeviceToHost);
  hipError_t e2 = hipMemcpy ((void *) rows, d->sp.d_rows, rows_bytes, hipMemcpyDeviceToHost);
  if (e1 != hipSuccess || e2 != hipSuccess)
    {
      hipHostFree (blk);
      return pc_fail (d, "call_sites_sparse: copying the list back: %s", hipGetErrorString (e1 != hipSuccess ? e1 : e2));
    }
  std::vector < unsigned >order ((size_t) n);
  for (size_t i = 0; i < (size_t) n; i++)
    order[i] = (unsigned) i;
  std::sort (order.begin (), order.end (), [&] (unsigned a, unsigned b) { return cols[a] < cols[b]; });
  for (size_t i = 0; i < (size_t) n; i++)
    {
      io.post_site[i] = cols[order[i]];
      memcpy (io.post_rows + i * N, rows + (size_t) order[i] * N, N * sizeof (double));
    }
  hipHostFree (blk);
  return 0;
}

static int pcs_call_sites_impl (pecall_dev * d, PcsIo io, long n_sites, int indiv, int haploid, double threshold, double theta)
{
  PCCHK (d, hipSetDevice (d->device));
  if (n_sites <= 0 || indiv <= 0 || indiv > PCS_MAXN)
    return pc_fail (d, "call_sites: n_sites %ld, indiv %d (1..%d samples per call)", n_sites, indiv, PCS_MAXN);
  if ((!io.resident && (!io.reads || !io.ref_base)) || !io.call || (!io.sparse && !io.posterior))
    return pc_fail (d, "call_sites: a required pointer is NULL");
  if (io.sparse && (!io.post_site || !io.post_rows || !io.n_post || io.post_cap == 0))
    return pc_fail (d, "call_sites_sparse: the list of posteriors needs post_site, post_rows, a capacity and n_post");
  d->result_sites = 0;
  d->run_stats_sites = 0;
  if (io.sparse)
    {
      *io.n_post = 0;
      PCTRY (pcs_ensure_sparse (d, io.post_cap, indiv));
      PCCHK (d, hipMemsetAsync (d->sp.d_n, 0, sizeof (unsigned long long), d->stream));
    }
  // (the tables first: the parameter block carries their device addresses)
  PCTRY (pcs_ensure (d, n_sites, indiv));
  PcsParams P;
  PCTRY (pcs_params (d, indiv, haploid, threshold, theta, P));
  PCTRY (pcs_ensure_chunks (d, n_sites));
  d->staged_sites = n_sites;
  d->staged_indiv = indiv;
  const long C = d->chunk_sites;
  const int nch = pcs_n_chunks (d);
  const size_t N = (size_t) indiv, S = (size_t) n_sites;
  io.in_direct = io.resident || (pm_host_pin_lookup (io.reads, S * N * PCS_NA * 2) && pm_host_pin_lookup (io.ref_base, S)
                                 && (!io.chrom_type || pm_host_pin_lookup (io.chrom_type, S)));
  io.out_direct = pm_host_pin_lookup (io.call, S * N) && (io.sparse || pm_host_pin_lookup (io.posterior, S * N * 8))
    && (!io.site_type || pm_host_pin_lookup (io.site_type, S)) && (!io.allele_count || pm_host_pin_lookup (io.allele_count, S * PCS_NA * 4))
    && (!io.n_pass || pm_host_pin_lookup (io.n_pass, S)) && (!io.denovo || pm_host_pin_lookup (io.denovo, S * 4));
  // per column: in = reads + reference base + chromosome class; out = calls + posteriors + type + passes + allele counts + de-novo count
  const size_t in_col = N * PCS_NA * 2 + 2, out_col = N * (io.sparse ? 1 : 9) + 2 + PCS_NA * 4 + 4, cmax = (size_t) (n_sites < C ? n_sites : C);
  if (!io.in_direct)
    PCTRY (pcs_ensure_slots (d, d->h_in, d->h_in_bytes, cmax * in_col, (size_t) C * in_col));
  if (!io.out_direct)
    PCTRY (pcs_ensure_slots (d, d->h_out, d->h_out_bytes, cmax * out_col, (size_t) C * out_col));
  const bool trace = getenv ("PECALL_SEAM_TRACE") != nullptr;
  const auto t_start = std::chrono::steady_clock::now ();
  auto since = [&] () { return std::chrono::duration < double, std::milli > (std::chrono::steady_clock::now () - t_start).count (); };
  for (int k = 0; k < nch; k++)
    {
      const double t0 = since ();
      if (!io.resident)
        PCTRY (pcs_stage_in (d, io, k, pcs_chunk_view (d, k), N));
      PCCHK (d, hipEventRecord (d->chunks[k].h2d, d->stream_h2d));
      // ---- the chunk's kernels behind its copy, its results behind its kernels: all queued, the host goes on to the next chunk
      //      (the result slot of its number is free when the results of the chunk PCS_SLOTS chunks ago have been handed over)
      PCCHK (d, hipStreamWaitEvent (d->stream, d->chunks[k].h2d, 0));
      if (!io.out_direct && k >= PCS_SLOTS)
        PCTRY (pcs_hand_over (d, io, k - PCS_SLOTS));
      PCTRY (pcs_queue_chunk (d, P, io, k, false));
      if (trace)
        fprintf (stderr, "[pecall seam] chunk %d: host at %.2f ms, enqueued by %.2f ms (direct in %d out %d)\n", k, t0, since (), (int) io.in_direct, (int) io.out_direct);
    }
  for (int j = (io.out_direct || nch < PCS_SLOTS) ? 0 : nch - PCS_SLOTS; j < nch; j++)
    PCTRY (pcs_hand_over (d, io, j));
  if (trace)
    fprintf (stderr, "[pecall seam] first pass on the host by %.2f ms\n", since ());
  // ---- chunks too deep for the table's head: once more, with the whole table (their columns are on the device)
  std::vector < int >deep;
  PCCHK (d, hipStreamSynchronize (d->stream));
  PCTRY (pcs_deep_chunks (d, P, nch, deep));
  for (int j : deep)
    {
      PCTRY (pcs_queue_chunk (d, P, io, j, true));
      PCTRY (pcs_hand_over (d, io, j));
    }
  PCCHK (d, hipStreamSynchronize (d->stream));
  for (int i = 0; i < PCS_CALL_STREAMS; i++)
    PCCHK (d, hipStreamSynchronize (d->stream_call[i]));
  d->result_sites = n_sites;    // (also where the list below turns out too short: the columns' results are whole)
  if (io.sparse)
    PCTRY (pcs_collect_sparse (d, io, N));
  if (trace)
    fprintf (stderr, "[pecall seam] done at %.2f ms\n", since ());
  return 0;
}

// ---- columns from record streams (pecall_merge.hip.h)

static inline size_t pcm_up64 (size_t x)
{
  return (x + 63) & ~(size_t) 63;
}

static int pcm_ensure (pecall_dev * d, size_t total, size_t span_pad, size_t stage_bytes, size_t n_iv)
{
  PcmState & g = d->mg;
  if (n_iv > g.cap_iv)
    {
      pc_free (g.d_iv);
      g.cap_iv = 0;
      const size_t cap = pcm_up64 (n_iv + n_iv / 4);
      PCCHK (d, hipMalloc ((void **) &g.d_iv, cap * 9));
      g.cap_iv = cap;
    }
  if (!g.d_bsum)
    {
      for (hipEvent_t & e : g.ev)
        if (!e)
          PCCHK (d, hipEventCreate (&e));
      pc_free (g.d_off, g.d_ctl);
      PCCHK (d, hipMalloc ((void **) &g.d_off, sizeof (unsigned long long) * (PCS_MAXN + 1)));
      PCCHK (d, hipMalloc ((void **) &g.d_ctl, sizeof (PcmCtl)));
      PCCHK (d, hipMalloc ((void **) &g.d_bsum, sizeof (unsigned) * PCM_MAX_SCAN_BLOCKS));
    }
  if (total > g.cap_recs)
    {
      pc_free (g.d_recs);
      g.cap_recs = 0;
      PCCHK (d, hipMalloc ((void **) &g.d_recs, total * 16));
      g.cap_recs = total;
    }
  if (span_pad > g.cap_span)
    {
      pc_free (g.d_marks, g.d_letters, g.d_chrom, g.d_colof, g.d_colslot);
      g.cap_span = 0;
      PCCHK (d, hipMalloc ((void **) &g.d_marks, span_pad));
      PCCHK (d, hipMalloc ((void **) &g.d_letters, span_pad));
      PCCHK (d, hipMalloc ((void **) &g.d_chrom, span_pad));
      PCCHK (d, hipMalloc ((void **) &g.d_colof, span_pad * sizeof (unsigned)));
      PCCHK (d, hipMalloc ((void **) &g.d_colslot, span_pad * sizeof (unsigned)));
      g.cap_span = span_pad;
    }
  if (stage_bytes > g.h_stage_bytes)
    {
      pc_host_free (g.h_stage);
      g.h_stage_bytes = 0;
      PCCHK (d, hipHostMalloc ((void **) &g.h_stage, stage_bytes + stage_bytes / 4, hipHostMallocDefault));
      g.h_stage_bytes = stage_bytes + stage_bytes / 4;
    }
  return 0;
}

// Replaces the host's k-way merge of the pileup streams (find_lowest and the per-column loop, pecaller.c:865-923, 1820-1833) for a
// range of positions: the samples' records go up as they are, the kernels of pecall_merge.hip.h make the columns.  The host waits
// twice: for the number of columns (the column arrays are sized by it) and for the end.
//
// The guided form (gd: the intervals; the guide-file loop, pecaller.c:941-1039): the marks come from the intervals, the records are only
// checked, and the slots' chromosome bytes are made on the device.  Everything behind the marks is the same code.
struct PcmGuide
{
  const uint32_t *first, *count;
  const uint8_t *chrom;         // may be nullptr: 0
  uint32_t n;
};

static int pcm_stage_impl (pecall_dev * d, const void *const *recs, const uint64_t * n_recs, int indiv, uint32_t p0, uint32_t span, const char *ref_letters,
                           uint32_t ref_len, const uint8_t * chrom_by_slot, const PcmGuide * gd, long *n_cols, uint32_t * col_slot)
{
  PCCHK (d, hipSetDevice (d->device));
  if (n_cols)
    *n_cols = 0;
  if (!recs || !n_recs || !n_cols)
    return pc_fail (d, "stage_records: recs, n_recs and n_cols are required");
  if (indiv < 1 || indiv > PCS_MAXN || span < 1 || span > PCM_MAX_SPAN)
    return pc_fail (d, "stage_records: indiv %d (1..%d), span %u (1..%u)", indiv, PCS_MAXN, span, PCM_MAX_SPAN);
  if (ref_len > span || (ref_len && !ref_letters))
    return pc_fail (d, "stage_records: %u reference letters for a range of %u positions", ref_len, span);
  if (gd)
    {
      // the intervals become addresses on the device: none empty, all inside the span, ascending and disjoint
      if (gd->n && (!gd->first || !gd->count))
        return pc_fail (d, "stage_records_guided: %u intervals and no arrays", gd->n);
      if (gd->n > span)
        return pc_fail (d, "stage_records_guided: %u intervals in a range of %u positions", gd->n, span);
      unsigned long long next = 0;
      for (uint32_t k = 0; k < gd->n; k++)
        {
          const unsigned long long f = gd->first[k], c = gd->count[k];
          if (c < 1 || f + c > span || f < next)
            return pc_fail (d, "stage_records_guided: interval %u (slots %llu .. %llu of %u) is empty, leaves the range or does not lie beyond its predecessor",
                            k, f, f + c, span);
          next = f + c;
        }
    }
  // (a stream of more than span records has a record out of order or out of range among its first span + 1: those go up)
  unsigned long long off[PCS_MAXN + 1];
  size_t staged_bytes = 0;
  off[0] = 0;
  for (int i = 0; i < indiv; i++)
    {
      const unsigned long long n = n_recs[i] > (uint64_t) span + 1 ? (unsigned long long) span + 1 : (unsigned long long) n_recs[i];
      if (n && !recs[i])
        return pc_fail (d, "stage_records: sample %d has %llu records and no array", i, (unsigned long long) n_recs[i]);
      off[i + 1] = off[i] + n;
      if (n && !pm_host_pin_lookup (recs[i], (size_t) n * 16))
        staged_bytes += (size_t) n * 16;
    }
  d->staged_sites = d->result_sites = 0;
  const size_t total = (size_t) off[indiv];
  if (gd ? gd->n == 0 : total == 0)
    return 0;
  const size_t n_iv = gd ? gd->n : 0;
  const size_t span_pad = ((size_t) span + PCM_SCAN_TILE - 1) / PCM_SCAN_TILE * PCM_SCAN_TILE;
  const unsigned nb = (unsigned) (span_pad / PCM_SCAN_TILE);
  // staging: [PcmCtl][col_slot span][offsets][letters][classes, or the guided form's intervals][records of ranges that are not pinned]
  const size_t at_slot = 64, at_off = at_slot + pcm_up64 ((size_t) span * 4), at_let = at_off + pcm_up64 (sizeof off), at_chr = at_let + pcm_up64 (span),
    at_rec = at_chr + (gd ? pcm_up64 (n_iv * 9) : pcm_up64 (span)), need = at_rec + staged_bytes;
  PCTRY (pcm_ensure (d, total, span_pad, need, n_iv));
  char *st = d->mg.h_stage;
  memcpy (st + at_off, off, sizeof (unsigned long long) * (size_t) (indiv + 1));
  PCCHK (d, hipMemcpyAsync (d->mg.d_off, st + at_off, sizeof (unsigned long long) * (size_t) (indiv + 1), hipMemcpyHostToDevice, d->stream));
  if (ref_len)
    {
      memcpy (st + at_let, ref_letters, ref_len);
      PCCHK (d, hipMemcpyAsync (d->mg.d_letters, st + at_let, ref_len, hipMemcpyHostToDevice, d->stream));
    }
  if (gd)
    {
      // on the device: first[cap_iv], count[cap_iv], then the bytes
      const size_t cap = d->mg.cap_iv;
      char *iv = st + at_chr;
      memcpy (iv, gd->first, n_iv * 4);
      memcpy (iv + n_iv * 4, gd->count, n_iv * 4);
      if (gd->chrom)
        memcpy (iv + n_iv * 8, gd->chrom, n_iv);
      PCCHK (d, hipMemcpyAsync (d->mg.d_iv, iv, n_iv * 4, hipMemcpyHostToDevice, d->stream));
      PCCHK (d, hipMemcpyAsync (d->mg.d_iv + cap, iv + n_iv * 4, n_iv * 4, hipMemcpyHostToDevice, d->stream));
      if (gd->chrom)
        PCCHK (d, hipMemcpyAsync (d->mg.d_iv + 2 * cap, iv + n_iv * 8, n_iv, hipMemcpyHostToDevice, d->stream));
    }
  else if (chrom_by_slot)
    {
      memcpy (st + at_chr, chrom_by_slot, span);
      PCCHK (d, hipMemcpyAsync (d->mg.d_chrom, st + at_chr, span, hipMemcpyHostToDevice, d->stream));
    }
  {
    char *sr = st + at_rec;
    for (int i = 0; i < indiv; i++)
      {
        const size_t bytes = (size_t) (off[i + 1] - off[i]) * 16;
        if (!bytes)
          continue;
        const void *src = recs[i];
        if (!pm_host_pin_lookup (src, bytes))
          {
            pm_par_memcpy (sr, (const char *) src, bytes);
            src = sr;
            sr += bytes;
          }
        PCCHK (d, hipMemcpyAsync (d->mg.d_recs + off[i], src, bytes, hipMemcpyHostToDevice, d->stream));
      }
  }
  if (!gd)
    PCCHK (d, hipMemsetAsync (d->mg.d_marks, 0, span_pad, d->stream));
  PCCHK (d, hipMemsetAsync (&d->mg.d_ctl->bad, 0xff, sizeof (unsigned long long), d->stream));
  PCCHK (d, hipMemsetAsync (&d->mg.d_ctl->n_cols, 0, 2 * sizeof (unsigned), d->stream));
  // ---- stage 1: the marks; stage 2's first half: the number of columns
  unsigned long long most = 0;
  for (int i = 0; i < indiv; i++)
    if (off[i + 1] - off[i] > most)
      most = off[i + 1] - off[i];
  const unsigned gx = (unsigned) ((most + PCM_BLOCK - 1) / PCM_BLOCK < 1024 ? (most + PCM_BLOCK - 1) / PCM_BLOCK : 1024);
  PCCHK (d, hipEventRecord (d->mg.ev[0], d->stream));
  if (gd)
    {
      const unsigned n16 = (unsigned) (span_pad / 16);
      const unsigned *iv = d->mg.d_iv;
      hipLaunchKernelGGL (pcm_guide_marks_kernel, dim3 ((n16 + PCM_BLOCK - 1) / PCM_BLOCK), dim3 (PCM_BLOCK), 0, d->stream, iv, iv + d->mg.cap_iv,
                          gd->chrom ? (const uint8_t *) (iv + 2 * d->mg.cap_iv) : (const uint8_t *) nullptr, gd->n, n16, (uint4 *) d->mg.d_marks, (uint4 *) d->mg.d_chrom);
    }
  if (gx)                       // (the guided form may come without any record)
    hipLaunchKernelGGL (pcm_mark_kernel, dim3 (gx, (unsigned) indiv), dim3 (PCM_BLOCK), 0, d->stream, (const uint4 *) d->mg.d_recs, (const unsigned long long *) d->mg.d_off, p0,
                        span, gd ? (uint8_t *) nullptr : d->mg.d_marks, d->mg.d_ctl);
  PCCHK (d, hipEventRecord (d->mg.ev[1], d->stream));
  hipLaunchKernelGGL (pcm_scan_reduce_kernel, dim3 (nb), dim3 (PCM_BLOCK), 0, d->stream, (const uint4 *) d->mg.d_marks, d->mg.d_bsum);
  hipLaunchKernelGGL (pcm_scan_top_kernel, dim3 (1), dim3 (PCM_MAX_SCAN_BLOCKS), 0, d->stream, d->mg.d_bsum, nb, d->mg.d_ctl);
  PCCHK (d, hipGetLastError ());
  PCCHK (d, hipEventRecord (d->mg.ev[2], d->stream));
  PCCHK (d, hipMemcpyAsync (st, d->mg.d_ctl, sizeof (PcmCtl), hipMemcpyDeviceToHost, d->stream));
  PCCHK (d, hipStreamSynchronize (d->stream));
  const PcmCtl ctl = *(const PcmCtl *) st;
  if (ctl.bad != PCM_NO_BAD)
    {
      const int bs = (int) (ctl.bad >> PCM_BAD_SHIFT);
      const unsigned long long bj = ctl.bad & ((1ull << PCM_BAD_SHIFT) - 1);
      uint32_t bp = 0;
      memcpy (&bp, (const char *) recs[bs] + (size_t) bj * 16, 4);
      snprintf (d->err, sizeof d->err, "stage_records: sample %d, record %llu (position %u) is not beyond its predecessor or lies outside [%u, %llu): "
                "the streams must ascend strictly inside the range", bs, bj, bp, p0, (unsigned long long) p0 + span);
      return PECALL_RC_UNORDERED;
    }
  const long n = (long) ctl.n_cols;
  PCTRY (pcs_ensure (d, n, indiv));
  // ---- stage 2's second half: the slots' columns; stage 3: the columns' reads
  PCCHK (d, hipEventRecord (d->mg.ev[3], d->stream));
  hipLaunchKernelGGL (pcm_scan_apply_kernel, dim3 (nb), dim3 (PCM_BLOCK), 0, d->stream, (const uint4 *) d->mg.d_marks, (const unsigned *) d->mg.d_bsum, span,
                      (const uint8_t *) d->mg.d_letters, ref_len, gd || chrom_by_slot ? (const uint8_t *) d->mg.d_chrom : (const uint8_t *) nullptr, d->mg.d_colof, d->mg.d_colslot,
                      d->cols.d_dom, d->cols.d_chromy);
  PCCHK (d, hipEventRecord (d->mg.ev[4], d->stream));
  const int S = pcm_tile_slots (indiv);
  const size_t lds = (size_t) S * indiv * 12 + (size_t) S * 4 + (size_t) indiv * 4;
  hipLaunchKernelGGL (pcm_tile_kernel, dim3 ((span + (unsigned) S - 1) / (unsigned) S), dim3 (PCM_BLOCK), lds, d->stream, (const uint4 *) d->mg.d_recs,
                      (const unsigned long long *) d->mg.d_off, indiv, p0, span, S, (const uint8_t *) d->mg.d_marks, (const unsigned *) d->mg.d_colof, (const PcmCtl *) d->mg.d_ctl,
                      d->cols.d_sreads);
  PCCHK (d, hipGetLastError ());
  PCCHK (d, hipEventRecord (d->mg.ev[5], d->stream));
  if (col_slot)
    PCCHK (d, hipMemcpyAsync (st + at_slot, d->mg.d_colslot, (size_t) n * 4, hipMemcpyDeviceToHost, d->stream));
  PCCHK (d, hipStreamSynchronize (d->stream));
  if (col_slot)
    memcpy (col_slot, st + at_slot, (size_t) n * 4);
  float a = 0, b = 0;
  PCCHK (d, hipEventElapsedTime (&d->mg.ms[0], d->mg.ev[0], d->mg.ev[1]));
  PCCHK (d, hipEventElapsedTime (&a, d->mg.ev[1], d->mg.ev[2]));
  PCCHK (d, hipEventElapsedTime (&b, d->mg.ev[3], d->mg.ev[4]));
  d->mg.ms[1] = a + b;
  PCCHK (d, hipEventElapsedTime (&d->mg.ms[2], d->mg.ev[4], d->mg.ev[5]));
  d->staged_sites = n;
  d->staged_indiv = indiv;
  *n_cols = n;
  return 0;
}

extern "C" int pecall_dev_sites_stage_records (pecall_dev * d, const void *const *recs, const uint64_t * n_recs, int indiv, uint32_t p0, uint32_t span,
                                               const char *ref_letters, uint32_t ref_len, const uint8_t * chrom_by_slot, long *n_cols, uint32_t * col_slot)
{
  return pcm_stage_impl (d, recs, n_recs, indiv, p0, span, ref_letters, ref_len, chrom_by_slot, nullptr, n_cols, col_slot);
}

extern "C" int pecall_dev_sites_stage_records_guided (pecall_dev * d, const void *const *recs, const uint64_t * n_recs, int indiv, uint32_t p0, uint32_t span,
                                                      const char *ref_letters, uint32_t ref_len, const uint32_t * iv_first, const uint32_t * iv_count,
                                                      const uint8_t * iv_chrom, uint32_t n_iv, long *n_cols, uint32_t * col_slot)
{
  const PcmGuide gd = { iv_first, iv_count, iv_chrom, n_iv };
  return pcm_stage_impl (d, recs, n_recs, indiv, p0, span, ref_letters, ref_len, nullptr, &gd, n_cols, col_slot);
}

extern "C" int pecall_dev_sites_merge_ms (pecall_dev * d, float *ms3)
{
  if (!ms3)
    return pc_fail (d, "sites_merge_ms: no array");
  memcpy (ms3, d->mg.ms, sizeof d->mg.ms);
  return 0;
}

extern "C" int pecall_dev_sites_gather (pecall_dev * d, const uint32_t * cols, uint64_t n, uint16_t * reads_out, uint8_t * ref_base_out, uint8_t * chrom_out)
{
  PCCHK (d, hipSetDevice (d->device));
  const long staged = d->staged_sites;
  const size_t N = (size_t) d->staged_indiv;
  if (staged <= 0)
    return pc_fail (d, "sites_gather: nothing staged");
  if (!cols && n > (uint64_t) staged)
    return pc_fail (d, "sites_gather: %llu columns asked for, %ld staged", (unsigned long long) n, staged);
  for (uint64_t i = 0; cols && i < n; i++)
    if (cols[i] >= (uint64_t) staged)
      return pc_fail (d, "sites_gather: cols[%llu] = %u, %ld columns are staged", (unsigned long long) i, cols[i], staged);
  if (n == 0)
    return 0;
  // a piece of the columns at a time: [column numbers][reads][reference bytes][chromosome bytes], the last three in one copy
  const size_t row = N * PCS_NA * 2, per_col = 4 + row + 2;
  const size_t piece = n * per_col <= ((size_t) 64 << 20) ? (size_t) n : (((size_t) 64 << 20) / per_col > 0 ? ((size_t) 64 << 20) / per_col : 1);
  const size_t need = piece * per_col;
  if (need > d->mg.cap_gather)
    {
      PCCHK (d, hipStreamSynchronize (d->stream));
      pc_free (d->mg.d_gather);
      pc_host_free (d->mg.h_gather);
      d->mg.cap_gather = 0;
      PCCHK (d, hipMalloc ((void **) &d->mg.d_gather, need));
      PCCHK (d, hipHostMalloc ((void **) &d->mg.h_gather, need, hipHostMallocDefault));
      d->mg.cap_gather = need;
    }
  for (size_t at = 0; at < (size_t) n; at += piece)
    {
      const size_t m = (size_t) n - at < piece ? (size_t) n - at : piece;
      const size_t o_reads = piece * 4, o_ref = o_reads + m * row, o_chr = o_ref + m;
      if (cols)
        {
          memcpy (d->mg.h_gather, cols + at, m * 4);
          PCCHK (d, hipMemcpyAsync (d->mg.d_gather, d->mg.h_gather, m * 4, hipMemcpyHostToDevice, d->stream));
        }
      const unsigned grid = (unsigned) (m < (size_t) d->grid * 8 ? m : (size_t) d->grid * 8);
      // (cols == nullptr: columns at .. at + m - 1, the arrays offset instead)
      hipLaunchKernelGGL (pcm_gather_kernel, dim3 (grid), dim3 (PCM_BLOCK), 0, d->stream, (const uint16_t *) d->cols.d_sreads + (cols ? 0 : at * N * PCS_NA),
                          (const uint8_t *) d->cols.d_dom + (cols ? 0 : at), (const uint8_t *) d->cols.d_chromy + (cols ? 0 : at), cols ? staged : staged - (long) at, (int) N,
                          cols ? (const unsigned *) d->mg.d_gather : (const unsigned *) nullptr, (unsigned long long) m, (unsigned *) (d->mg.d_gather + o_reads),
                          (uint8_t *) d->mg.d_gather + o_ref, (uint8_t *) d->mg.d_gather + o_chr);
      PCCHK (d, hipGetLastError ());
      PCCHK (d, hipMemcpyAsync (d->mg.h_gather + o_reads, d->mg.d_gather + o_reads, m * (row + 2), hipMemcpyDeviceToHost, d->stream));
      PCCHK (d, hipStreamSynchronize (d->stream));
      if (reads_out)
        pm_par_memcpy ((char *) reads_out + at * row, d->mg.h_gather + o_reads, m * row);
      if (ref_base_out)
        memcpy (ref_base_out + at, d->mg.h_gather + o_ref, m);
      if (chrom_out)
        memcpy (chrom_out + at, d->mg.h_gather + o_chr, m);
    }
  return 0;
}

// ---- the rows of <outfile>.base.gz (pecall_rows.hip.h)

static int pcr_ensure (pecall_dev * d, size_t pad, size_t n_contigs, size_t names_bytes, size_t stage_bytes)
{
  PcrState & w = d->rows;
  if (!w.d_ctl)
    {
      for (hipEvent_t & e : w.ev)
        if (!e)
          PCCHK (d, hipEventCreate (&e));
      for (hipEvent_t & e : w.ev_piece)
        if (!e)
          PCCHK (d, hipEventCreateWithFlags (&e, hipEventDisableTiming));
      PCCHK (d, hipMalloc ((void **) &w.d_ctl, sizeof (PcrCtl)));
    }
  if (pad > w.cap_cols)
    {
      pc_free (w.d_contig, w.d_pos, w.d_ref, w.d_len, w.d_off, w.d_hole_site, w.d_hole_at, w.d_bsum_bytes, w.d_bsum_holes);
      w.cap_cols = 0;
      PCCHK (d, hipMalloc ((void **) &w.d_contig, pad * sizeof (int32_t)));
      PCCHK (d, hipMalloc ((void **) &w.d_pos, pad * sizeof (uint32_t)));
      PCCHK (d, hipMalloc ((void **) &w.d_ref, pad));
      PCCHK (d, hipMalloc ((void **) &w.d_len, pad * sizeof (unsigned)));
      PCCHK (d, hipMalloc ((void **) &w.d_off, pad * sizeof (unsigned long long)));
      PCCHK (d, hipMalloc ((void **) &w.d_hole_site, pad * sizeof (uint32_t)));
      PCCHK (d, hipMalloc ((void **) &w.d_hole_at, pad * sizeof (unsigned long long)));
      PCCHK (d, hipMalloc ((void **) &w.d_bsum_bytes, pad / PCR_SCAN_TILE * sizeof (unsigned long long)));
      PCCHK (d, hipMalloc ((void **) &w.d_bsum_holes, pad / PCR_SCAN_TILE * sizeof (unsigned)));
      w.cap_cols = pad;
    }
  if (n_contigs + 1 > w.cap_contigs)
    {
      pc_free (w.d_name_off);
      w.cap_contigs = 0;
      PCCHK (d, hipMalloc ((void **) &w.d_name_off, (n_contigs + 1) * sizeof (uint32_t)));
      w.cap_contigs = n_contigs + 1;
    }
  if (names_bytes + 1 > w.cap_names)
    {
      pc_free (w.d_names);
      w.cap_names = 0;
      PCCHK (d, hipMalloc ((void **) &w.d_names, names_bytes + 1));
      w.cap_names = names_bytes + 1;
    }
  if (stage_bytes > w.h_stage_bytes)
    {
      pc_host_free (w.h_stage);
      w.h_stage_bytes = 0;
      PCCHK (d, hipHostMalloc ((void **) &w.h_stage, stage_bytes + stage_bytes / 4, hipHostMallocDefault));
      w.h_stage_bytes = stage_bytes + stage_bytes / 4;
    }
  return 0;
}

// `bytes` of a per-column array on their way up: from where they lie if the caller page-locked them, else through the staging block
static int pcr_upload (pecall_dev * d, void *dev, const void *host, char *stage, size_t bytes)
{
  if (!pm_host_pin_lookup (host, bytes))
    {
      pm_par_memcpy (stage, (const char *) host, bytes);
      host = stage;
    }
  PCCHK (d, hipMemcpyAsync (dev, host, bytes, hipMemcpyHostToDevice, d->stream));
  return 0;
}

// the text (or the members made of it) back, PCR_PIECE at a time on the device-to-host stream, behind event `filled`
static int pcr_text_back (pecall_dev * d, hipEvent_t filled, const char *d_text, char *text, size_t total)
{
  PcrState & w = d->rows;
  PCCHK (d, hipStreamWaitEvent (d->stream_d2h, filled, 0));
  if (pm_host_pin_lookup (text, total))
    {
      for (size_t at = 0; at < total; at += PCR_PIECE)
        PCCHK (d, hipMemcpyAsync (text + at, d_text + at, std::min (PCR_PIECE, total - at), hipMemcpyDeviceToHost, d->stream_d2h));
      PCCHK (d, hipStreamSynchronize (d->stream_d2h));
      return 0;
    }
  for (char *&h : w.h_text)
    if (!h)
      PCCHK (d, hipHostMalloc ((void **) &h, PCR_PIECE, hipHostMallocDefault));
  // (piece k travels while piece k - 1 is copied out of the other block)
  const size_t pieces = (total + PCR_PIECE - 1) / PCR_PIECE;
  for (size_t k = 0; k <= pieces; k++)
    {
      if (k < pieces)
        {
          PCCHK (d, hipMemcpyAsync (w.h_text[k & 1], d_text + k * PCR_PIECE, std::min (PCR_PIECE, total - k * PCR_PIECE), hipMemcpyDeviceToHost, d->stream_d2h));
          PCCHK (d, hipEventRecord (w.ev_piece[k & 1], d->stream_d2h));
        }
      if (k > 0)
        {
          const size_t at = (k - 1) * PCR_PIECE;
          PCCHK (d, hipEventSynchronize (w.ev_piece[(k - 1) & 1]));
          pm_par_memcpy (text + at, w.h_text[(k - 1) & 1], std::min (PCR_PIECE, total - at));
        }
    }
  return 0;
}

// Replaces the .base half of the row formatting (emit_rows of pecaller_main.c; the per-sample gzprintf loop of pecaller.c:1760-1775)
// for the columns whose posteriors are all exactly 1.  The host waits twice: for the text's length and the number of holes (the
// caller's buffers are checked against them, the device text is sized by it), and for the end.
// want_text false (pecall_dev_sites_base_gz): the text and the holes' offsets stay on the device, the capacities are the caller's to check.
static int pcr_base_impl (pecall_dev * d, const char *who, bool want_text, const char *names, const uint32_t * name_off, int n_contigs, const int32_t * contig,
                          const uint32_t * pos, const char *ref_char, char *text, uint64_t text_cap, uint64_t * n_text, uint32_t * hole_site, uint64_t * hole_at,
                          uint64_t hole_cap, uint64_t * n_holes, float *kernel_ms3)
{
  PCCHK (d, hipSetDevice (d->device));
  if (n_text)
    *n_text = 0;
  if (n_holes)
    *n_holes = 0;
  if (kernel_ms3)
    kernel_ms3[0] = kernel_ms3[1] = kernel_ms3[2] = 0.0f;
  const long n = d->result_sites;
  const int N = d->staged_indiv;
  if (n <= 0)
    return pc_fail (d, "%s: no call's results are on the device (call_sites, call_sites_sparse, call_records or sites_run first)", who);
  if (!names || !name_off || n_contigs < 1 || !contig || !pos || !ref_char || !n_text || !n_holes)
    return pc_fail (d, "%s: names, name_off, at least one contig, contig, pos, ref_char, n_text and n_holes are required", who);
  if ((text_cap && !text) || (hole_cap && (!hole_site || !hole_at)))
    return pc_fail (d, "%s: a capacity without its array", who);
  // ---- the small things, before a kernel turns them into addresses
  unsigned max_name = 0;
  for (int c = 0; c < n_contigs; c++)
    {
      if (name_off[c + 1] < name_off[c] || name_off[c + 1] - name_off[c] > PCR_MAX_NAME)
        return pc_fail (d, "%s: name_off[%d..%d] = %u, %u: the offsets ascend and a name has at most %u bytes", who, c, c + 1, name_off[c], name_off[c + 1], PCR_MAX_NAME);
      max_name = std::max (max_name, name_off[c + 1] - name_off[c]);
    }
  for (long s = 0; s < n; s++)
    {
      if (contig[s] < 0 || contig[s] >= n_contigs)
        return pc_fail (d, "%s: contig[%ld] = %d, there are %d contigs", who, s, contig[s], n_contigs);
      if (pos[s] > PCR_MAX_POS)
        return pc_fail (d, "%s: pos[%ld] = %u is beyond %u (the rows print (int) pos)", who, s, pos[s], PCR_MAX_POS);
    }
  const size_t S = (size_t) n, pad = (S + 1 + PCR_SCAN_TILE - 1) / PCR_SCAN_TILE * PCR_SCAN_TILE, names_bytes = name_off[n_contigs] - name_off[0];
  const unsigned nb = (unsigned) (pad / PCR_SCAN_TILE);
  const size_t at_contig = 64, at_pos = at_contig + pcm_up64 (S * 4), at_ref = at_pos + pcm_up64 (S * 4), at_noff = at_ref + pcm_up64 (S),
    at_names = at_noff + pcm_up64 ((size_t) (n_contigs + 1) * 4), at_hsite = at_names + pcm_up64 (names_bytes + 1), at_hat = at_hsite + pcm_up64 (S * 4),
    need = at_hat + pcm_up64 (S * 8);
  PCTRY (pcr_ensure (d, pad, (size_t) n_contigs, names_bytes, need));
  PcrState & w = d->rows;
  char *st = w.h_stage;
  PCTRY (pcr_upload (d, w.d_contig, contig, st + at_contig, S * 4));
  PCTRY (pcr_upload (d, w.d_pos, pos, st + at_pos, S * 4));
  PCTRY (pcr_upload (d, w.d_ref, ref_char, st + at_ref, S));
  {
    // (the names' offsets from 0 on: the blob that goes up begins at the first name)
    uint32_t *o = (uint32_t *) (st + at_noff);
    for (int c = 0; c <= n_contigs; c++)
      o[c] = name_off[c] - name_off[0];
    memcpy (st + at_names, names + name_off[0], names_bytes);
    PCCHK (d, hipMemcpyAsync (w.d_name_off, o, (size_t) (n_contigs + 1) * 4, hipMemcpyHostToDevice, d->stream));
    if (names_bytes)
      PCCHK (d, hipMemcpyAsync (w.d_names, st + at_names, names_bytes, hipMemcpyHostToDevice, d->stream));
  }
  PCCHK (d, hipMemsetAsync (w.d_len + S, 0, (pad - S) * sizeof (unsigned), d->stream));
  // ---- lengths; the scan's first half: the text's length and the number of holes
  const long lgrid = std::min ((n + 3) / 4, (long) d->grid * 8);
  PCCHK (d, hipEventRecord (w.ev[0], d->stream));
  hipLaunchKernelGGL (pcr_len_kernel, dim3 ((unsigned) lgrid), dim3 (PCR_BLOCK), 0, d->stream, (const int8_t *) d->cols.d_type, (const double *) d->cols.d_post,
                      (const int32_t *) w.d_contig, (const uint32_t *) w.d_pos, (const uint32_t *) w.d_name_off, n, N, w.d_len);
  PCCHK (d, hipGetLastError ());
  PCCHK (d, hipEventRecord (w.ev[1], d->stream));
  hipLaunchKernelGGL (pcr_scan_reduce_kernel, dim3 (nb), dim3 (PCR_BLOCK), 0, d->stream, (const uint4 *) w.d_len, w.d_bsum_bytes, w.d_bsum_holes);
  PCCHK (d, hipGetLastError ());
  hipLaunchKernelGGL (pcr_scan_top_kernel, dim3 (1), dim3 (PCR_TOP), 0, d->stream, w.d_bsum_bytes, w.d_bsum_holes, nb, w.d_ctl);
  PCCHK (d, hipGetLastError ());
  PCCHK (d, hipEventRecord (w.ev[2], d->stream));
  PCCHK (d, hipMemcpyAsync (st, w.d_ctl, sizeof (PcrCtl), hipMemcpyDeviceToHost, d->stream));
  PCCHK (d, hipStreamSynchronize (d->stream));
  const PcrCtl ctl = *(const PcrCtl *) st;
  const size_t total = (size_t) ctl.n_text, holes = (size_t) ctl.n_holes;
  *n_text = ctl.n_text;
  *n_holes = ctl.n_holes;
  if (want_text && (ctl.n_text > text_cap || ctl.n_holes > hole_cap))
    return pc_fail (d, "%s: the text has %llu bytes and %llu rows are left to the host, the arrays hold %llu and %llu (n_text and n_holes say what is needed)", who,
                    ctl.n_text, ctl.n_holes, (unsigned long long) text_cap, (unsigned long long) hole_cap);
  float ms[3] = { 0.0f, 0.0f, 0.0f }, a = 0.0f;
  PCCHK (d, hipEventElapsedTime (&ms[0], w.ev[0], w.ev[1]));
  PCCHK (d, hipEventElapsedTime (&ms[1], w.ev[1], w.ev[2]));
  if (total || holes)
    {
      if (total + 16 > w.cap_text)
        {
          pc_free (w.d_text);
          w.cap_text = 0;
          PCCHK (d, hipMalloc ((void **) &w.d_text, total + total / 8 + 16));
          w.cap_text = total + total / 8 + 16;
        }
      // ---- the scan's second half: the columns' offsets and the holes; the text
      PCCHK (d, hipEventRecord (w.ev[3], d->stream));
      hipLaunchKernelGGL (pcr_scan_apply_kernel, dim3 (nb), dim3 (PCR_BLOCK), 0, d->stream, (const uint4 *) w.d_len, (const unsigned long long *) w.d_bsum_bytes,
                          (const unsigned *) w.d_bsum_holes, w.d_off, w.d_hole_site, w.d_hole_at);
      PCCHK (d, hipGetLastError ());
      PCCHK (d, hipEventRecord (w.ev[4], d->stream));
      if (total)
        {
          const int R = pcr_fill_run (max_name, N);
          const unsigned tile_bytes = pcr_fill_tile_bytes (max_name, N);
          hipLaunchKernelGGL (pcr_fill_kernel, dim3 ((unsigned) ((n + R - 1) / R)), dim3 (PCR_BLOCK), tile_bytes + (size_t) R * 4, d->stream, (const unsigned *) w.d_len,
                              (const unsigned long long *) w.d_off, (const int8_t *) d->cols.d_call, (const int32_t *) w.d_contig, (const uint32_t *) w.d_pos,
                              (const char *) w.d_ref, (const char *) w.d_names, (const uint32_t *) w.d_name_off, n, N, R, tile_bytes, w.d_text);
          PCCHK (d, hipGetLastError ());
        }
      PCCHK (d, hipEventRecord (w.ev[5], d->stream));
      if (holes && want_text)
        {
          PCCHK (d, hipMemcpyAsync (st + at_hsite, w.d_hole_site, holes * 4, hipMemcpyDeviceToHost, d->stream));
          PCCHK (d, hipMemcpyAsync (st + at_hat, w.d_hole_at, holes * 8, hipMemcpyDeviceToHost, d->stream));
        }
      if (total && want_text)
        PCTRY (pcr_text_back (d, w.ev[5], w.d_text, text, total));
      PCCHK (d, hipStreamSynchronize (d->stream));
      if (holes && want_text)
        {
          memcpy (hole_site, st + at_hsite, holes * 4);
          memcpy (hole_at, st + at_hat, holes * 8);
        }
      PCCHK (d, hipEventElapsedTime (&a, w.ev[3], w.ev[4]));
      ms[1] += a;
      PCCHK (d, hipEventElapsedTime (&ms[2], w.ev[4], w.ev[5]));
    }
  if (kernel_ms3)
    memcpy (kernel_ms3, ms, sizeof ms);
  return 0;
}

extern "C" int pecall_dev_sites_base_text (pecall_dev * d, const char *names, const uint32_t * name_off, int n_contigs, const int32_t * contig, const uint32_t * pos,
                                           const char *ref_char, char *text, uint64_t text_cap, uint64_t * n_text, uint32_t * hole_site, uint64_t * hole_at,
                                           uint64_t hole_cap, uint64_t * n_holes, float *kernel_ms3)
{
  return pcr_base_impl (d, "sites_base_text", true, names, name_off, n_contigs, contig, pos, ref_char, text, text_cap, n_text, hole_site, hole_at, hole_cap, n_holes,
                        kernel_ms3);
}

// ---- the same rows as gzip members (pecall_gz.hip.h)

static int pcg_ensure (pecall_dev * d, size_t pad_runs, size_t pad_pieces, size_t slot_bytes, size_t holes)
{
  PcgState & g = d->gz;
  if (!g.d_ctl)
    {
      for (hipEvent_t & e : g.ev)
        if (!e)
          PCCHK (d, hipEventCreate (&e));
      PCCHK (d, hipMalloc ((void **) &g.d_ctl, sizeof (PcgCtl)));
    }
  if (pad_runs > g.cap_runs)
    {
      pc_free (g.d_run, g.d_run_sum);
      g.cap_runs = 0;
      PCCHK (d, hipMalloc ((void **) &g.d_run, pad_runs * sizeof (unsigned long long)));
      PCCHK (d, hipMalloc ((void **) &g.d_run_sum, pad_runs / PCG_SCAN_TILE * sizeof (unsigned long long)));
      g.cap_runs = pad_runs;
    }
  if (pad_pieces > g.cap_pieces)
    {
      pc_free (g.d_piece_at, g.d_member, g.d_member_sum, g.d_piece_len);
      g.cap_pieces = 0;
      PCCHK (d, hipMalloc ((void **) &g.d_piece_at, pad_pieces * sizeof (unsigned long long)));
      PCCHK (d, hipMalloc ((void **) &g.d_member, pad_pieces * sizeof (unsigned long long)));
      PCCHK (d, hipMalloc ((void **) &g.d_member_sum, pad_pieces / PCG_SCAN_TILE * sizeof (unsigned long long)));
      PCCHK (d, hipMalloc ((void **) &g.d_piece_len, pad_pieces * sizeof (unsigned)));
      g.cap_pieces = pad_pieces;
    }
  if (slot_bytes > g.cap_slots)
    {
      pc_free (g.d_slots, g.d_gz);
      g.cap_slots = 0;
      PCCHK (d, hipMalloc ((void **) &g.d_slots, slot_bytes + slot_bytes / 8));
      PCCHK (d, hipMalloc ((void **) &g.d_gz, slot_bytes + slot_bytes / 8));
      g.cap_slots = slot_bytes + slot_bytes / 8;
    }
  if (holes + 1 > g.cap_holes)
    {
      pc_free (g.d_hole_gz_at);
      pc_host_free (g.h_stage);
      g.cap_holes = g.h_stage_bytes = 0;
      const size_t cap = holes + holes / 4 + 1;
      PCCHK (d, hipMalloc ((void **) &g.d_hole_gz_at, cap * sizeof (unsigned long long)));
      PCCHK (d, hipHostMalloc ((void **) &g.h_stage, 64 + pcm_up64 (cap * 4) + cap * 8, hipHostMallocDefault));
      g.cap_holes = cap;
      g.h_stage_bytes = 64 + pcm_up64 (cap * 4) + cap * 8;
    }
  return 0;
}

// exclusive prefix sum of val[0 .. pad) in place, pad a multiple of PCG_SCAN_TILE; the sum of all goes to *total
static int pcg_scan (pecall_dev * d, unsigned long long *val, unsigned long long *sum, size_t pad, unsigned long long *total)
{
  const unsigned nb = (unsigned) (pad / PCG_SCAN_TILE);
  hipLaunchKernelGGL (pcg_scan_reduce_kernel, dim3 (nb), dim3 (PCG_BLOCK), 0, d->stream, (const ulonglong4 *) val, sum);
  PCCHK (d, hipGetLastError ());
  hipLaunchKernelGGL (pcg_scan_top_kernel, dim3 (1), dim3 (PCG_TOP), 0, d->stream, sum, nb, total);
  PCCHK (d, hipGetLastError ());
  hipLaunchKernelGGL (pcg_scan_apply_kernel, dim3 (nb), dim3 (PCG_BLOCK), 0, d->stream, (ulonglong4 *) val, (const unsigned long long *) sum);
  PCCHK (d, hipGetLastError ());
  return 0;
}

// The text of pecall_dev_sites_base_text for the same arguments, deflated where it lies: complete gzip members in text order, none
// across a hole.  The host waits where that call waits, and once more for the packed length.
extern "C" int pecall_dev_sites_base_gz (pecall_dev * d, const char *names, const uint32_t * name_off, int n_contigs, const int32_t * contig, const uint32_t * pos,
                                         const char *ref_char, unsigned char *gz, uint64_t gz_cap, uint64_t * n_gz, uint32_t * hole_site, uint64_t * hole_gz_at,
                                         uint64_t hole_cap, uint64_t * n_holes, uint64_t * n_text, float *kernel_ms5)
{
  PCCHK (d, hipSetDevice (d->device));
  if (n_gz)
    *n_gz = 0;
  if (kernel_ms5)
    kernel_ms5[0] = kernel_ms5[1] = kernel_ms5[2] = kernel_ms5[3] = kernel_ms5[4] = 0.0f;
  if (!n_gz)
    {
      if (n_text)
        *n_text = 0;
      if (n_holes)
        *n_holes = 0;
      return pc_fail (d, "sites_base_gz: n_gz is required");
    }
  if ((gz_cap && !gz) || (hole_cap && (!hole_site || !hole_gz_at)))
    {
      if (n_text)
        *n_text = 0;
      if (n_holes)
        *n_holes = 0;
      return pc_fail (d, "sites_base_gz: a capacity without its array");
    }
  float ms[5] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
  PCTRY (pcr_base_impl (d, "sites_base_gz", false, names, name_off, n_contigs, contig, pos, ref_char, nullptr, 0, n_text, nullptr, nullptr, 0, n_holes, ms));
  const size_t total = (size_t) * n_text, holes = (size_t) * n_holes;
  if (total || holes)
    {
      PcrState & w = d->rows;
      const size_t max_pieces = total / PCG_PIECE + holes + 1;
      const size_t pad_runs = (holes + 2 + PCG_SCAN_TILE - 1) / PCG_SCAN_TILE * PCG_SCAN_TILE, pad_pieces = (max_pieces + 1 + PCG_SCAN_TILE - 1) / PCG_SCAN_TILE * PCG_SCAN_TILE;
      PCTRY (pcg_ensure (d, pad_runs, pad_pieces, pcg_slot_bytes (total, max_pieces), holes));
      PcgState & g = d->gz;
      PCCHK (d, hipEventRecord (g.ev[0], d->stream));
      hipLaunchKernelGGL (pcg_runs_kernel, dim3 ((unsigned) (pad_runs / PCG_BLOCK)), dim3 (PCG_BLOCK), 0, d->stream, (const unsigned long long *) w.d_hole_at,
                          (unsigned long long) holes, (unsigned long long) total, (unsigned long long) pad_runs, g.d_run);
      PCCHK (d, hipGetLastError ());
      PCTRY (pcg_scan (d, g.d_run, g.d_run_sum, pad_runs, &g.d_ctl->n_pieces));
      hipLaunchKernelGGL (pcg_table_kernel, dim3 ((unsigned) ((max_pieces + PCG_BLOCK - 1) / PCG_BLOCK)), dim3 (PCG_BLOCK), 0, d->stream,
                          (const unsigned long long *) w.d_hole_at, (unsigned long long) holes, (unsigned long long) total, (const unsigned long long *) g.d_run,
                          (const PcgCtl *) g.d_ctl, (unsigned long long) max_pieces, g.d_piece_at, g.d_piece_len);
      PCCHK (d, hipGetLastError ());
      PCCHK (d, hipMemsetAsync (g.d_member, 0, pad_pieces * sizeof (unsigned long long), d->stream));
      hipLaunchKernelGGL (pcg_deflate_kernel, dim3 ((unsigned) max_pieces), dim3 (PCG_BLOCK), 0, d->stream, (const char *) w.d_text, (unsigned long long) total,
                          (unsigned long long) (w.cap_text & ~(size_t) 15), (const unsigned long long *) g.d_piece_at, (const unsigned *) g.d_piece_len, (const PcgCtl *) g.d_ctl,
                          g.d_slots, (unsigned long long) g.cap_slots, g.d_member);
      PCCHK (d, hipGetLastError ());
      PCCHK (d, hipEventRecord (g.ev[1], d->stream));
      PCTRY (pcg_scan (d, g.d_member, g.d_member_sum, pad_pieces, &g.d_ctl->n_gz));
      hipLaunchKernelGGL (pcg_pack_kernel, dim3 ((unsigned) max_pieces), dim3 (PCG_BLOCK), 0, d->stream, (const unsigned char *) g.d_slots, (unsigned long long) g.cap_slots,
                          (const unsigned long long *) g.d_piece_at, (const unsigned long long *) g.d_member, (const PcgCtl *) g.d_ctl, g.d_gz,
                          (unsigned long long) g.cap_slots);
      PCCHK (d, hipGetLastError ());
      if (holes)
        {
          hipLaunchKernelGGL (pcg_holes_kernel, dim3 ((unsigned) ((holes + PCG_BLOCK - 1) / PCG_BLOCK)), dim3 (PCG_BLOCK), 0, d->stream, (const unsigned long long *) g.d_run,
                              (const unsigned long long *) g.d_member, (unsigned long long) holes, (unsigned long long) max_pieces, g.d_hole_gz_at);
          PCCHK (d, hipGetLastError ());
        }
      PCCHK (d, hipEventRecord (g.ev[2], d->stream));
      char *st = g.h_stage;
      const size_t at_site = 64, at_place = at_site + pcm_up64 (g.cap_holes * 4);
      PCCHK (d, hipMemcpyAsync (st, g.d_ctl, sizeof (PcgCtl), hipMemcpyDeviceToHost, d->stream));
      if (holes)
        {
          PCCHK (d, hipMemcpyAsync (st + at_site, w.d_hole_site, holes * 4, hipMemcpyDeviceToHost, d->stream));
          PCCHK (d, hipMemcpyAsync (st + at_place, g.d_hole_gz_at, holes * 8, hipMemcpyDeviceToHost, d->stream));
        }
      PCCHK (d, hipStreamSynchronize (d->stream));
      const PcgCtl ctl = *(const PcgCtl *) st;
      *n_gz = ctl.n_gz;
      PCCHK (d, hipEventElapsedTime (&ms[3], g.ev[0], g.ev[1]));
      PCCHK (d, hipEventElapsedTime (&ms[4], g.ev[1], g.ev[2]));
      if (ctl.n_gz > gz_cap || holes > hole_cap)
        return pc_fail (d, "sites_base_gz: the members have %llu bytes and %llu rows are left to the host, the arrays hold %llu and %llu (n_gz and n_holes say what is needed)",
                        ctl.n_gz, (unsigned long long) holes, (unsigned long long) gz_cap, (unsigned long long) hole_cap);
      if (holes)
        {
          memcpy (hole_site, st + at_site, holes * 4);
          memcpy (hole_gz_at, st + at_place, holes * 8);
        }
      if (ctl.n_gz)
        PCTRY (pcr_text_back (d, g.ev[2], (const char *) g.d_gz, (char *) gz, (size_t) ctl.n_gz));
    }
  if (kernel_ms5)
    memcpy (kernel_ms5, ms, sizeof ms);
  return 0;
}

// the chunk pipeline of pecall_dev_call_sites_sparse over the columns a stage of records left on the device
static int pcs_call_resident (pecall_dev * d, int8_t * call, uint32_t * post_site, double *post_rows, uint64_t post_cap, uint64_t * n_post, int8_t * site_type,
                              int32_t * allele_count, int8_t * n_pass, int32_t * denovo, long n, int indiv, int haploid, double threshold, double theta)
{
  return pcs_call_sites_impl (d, { nullptr, nullptr, nullptr, call, nullptr, site_type, allele_count, n_pass, denovo, true, post_site, post_rows, post_cap, n_post, true },
                              n, indiv, haploid, threshold, theta);
}

extern "C" int pecall_dev_call_records (pecall_dev * d, const void *const *recs, const uint64_t * n_recs, int indiv, uint32_t p0, uint32_t span, const char *ref_letters,
                                        uint32_t ref_len, const uint8_t * chrom_by_slot, long *n_cols, uint32_t * col_slot, int haploid, double threshold, double theta,
                                        int8_t * call, uint32_t * post_site, double *post_rows, uint64_t post_cap, uint64_t * n_post, int8_t * site_type,
                                        int32_t * allele_count, int8_t * n_pass, int32_t * denovo)
{
  if (n_post)
    *n_post = 0;
  const int rc = pcm_stage_impl (d, recs, n_recs, indiv, p0, span, ref_letters, ref_len, chrom_by_slot, nullptr, n_cols, col_slot);
  if (rc || *n_cols == 0)
    return rc;
  return pcs_call_resident (d, call, post_site, post_rows, post_cap, n_post, site_type, allele_count, n_pass, denovo, *n_cols, indiv, haploid, threshold, theta);
}

extern "C" int pecall_dev_call_records_guided (pecall_dev * d, const void *const *recs, const uint64_t * n_recs, int indiv, uint32_t p0, uint32_t span,
                                               const char *ref_letters, uint32_t ref_len, const uint32_t * iv_first, const uint32_t * iv_count, const uint8_t * iv_chrom,
                                               uint32_t n_iv, long *n_cols, uint32_t * col_slot, int haploid, double threshold, double theta, int8_t * call,
                                               uint32_t * post_site, double *post_rows, uint64_t post_cap, uint64_t * n_post, int8_t * site_type, int32_t * allele_count,
                                               int8_t * n_pass, int32_t * denovo)
{
  if (n_post)
    *n_post = 0;
  const PcmGuide gd = { iv_first, iv_count, iv_chrom, n_iv };
  const int rc = pcm_stage_impl (d, recs, n_recs, indiv, p0, span, ref_letters, ref_len, nullptr, &gd, n_cols, col_slot);
  if (rc || *n_cols == 0)
    return rc;
  return pcs_call_resident (d, call, post_site, post_rows, post_cap, n_post, site_type, allele_count, n_pass, denovo, *n_cols, indiv, haploid, threshold, theta);
}

extern "C" int pecall_dev_call_sites (pecall_dev * d, const uint16_t * reads, const uint8_t * ref_base, const uint8_t * chrom_type, long n_sites,
                                      int indiv, int haploid, double threshold, double theta, int8_t * call, double *posterior,
                                      int8_t * site_type, int32_t * allele_count, int8_t * n_pass, int32_t * denovo)
{
  return pcs_call_sites_impl (d, { reads, ref_base, chrom_type, call, posterior, site_type, allele_count, n_pass, denovo, false, nullptr, nullptr, 0, nullptr, false },
                              n_sites, indiv, haploid, threshold, theta);
}

extern "C" int pecall_dev_call_sites_sparse (pecall_dev * d, const uint16_t * reads, const uint8_t * ref_base, const uint8_t * chrom_type, long n_sites,
                                             int indiv, int haploid, double threshold, double theta, int8_t * call, uint32_t * post_site,
                                             double *post_rows, uint64_t post_cap, uint64_t * n_post, int8_t * site_type, int32_t * allele_count,
                                             int8_t * n_pass, int32_t * denovo)
{
  return pcs_call_sites_impl (d, { reads, ref_base, chrom_type, call, nullptr, site_type, allele_count, n_pass, denovo, true, post_site, post_rows, post_cap, n_post,
                                   false }, n_sites, indiv, haploid, threshold, theta);
}
