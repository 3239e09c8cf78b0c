/*
 * pecaller_main.c -- host program (plain C) with the command line and on-disk formats of the reference's pecaller,
 * calling the MI355X per-site caller through the C-ABI of include/pemap_hip.h (pecall_dev_call_sites).
 *
 *   pecaller_hip pileup_ext sdx no_files outfile Prob_to_call theta haploid[y,n] no_threads use_pedfile[y,n] [pedfile denovo_rate] [guide.bed]
 *
 * (src/pecaller.c:227-257.)  It runs in the directory that holds the binary pileups, like the reference: every file
 * whose name contains `pileup_ext` is a sample, in directory order, named by its file name up to the first '.'
 * (pecaller.c:495-515).  Outputs, in the reference's formats: <outfile>.base.gz (a call and a posterior per sample and
 * column), <outfile>.snp and <outfile>.piles.gz (the variant columns), <outfile>.dist (coverage statistics).
 *
 * What replaces what: the dispatcher loop of main (pecaller.c:865-923: the 64-way merge of the pileup streams by
 * position, the reference base and contig of the column) stays here on the host and fills tiles of columns; the worker
 * threads' call_single_base (1207-1691) is one pecall_dev_call_sites per tile; the worker's sprintf block (1564-1690) is
 * emit_rows below.  Rows are written in genome order (the reference's order depends on thread timing).
 *
 * With a BED guide file (the last argument, pecaller.c:925-1068) every position of the listed intervals is called, covered
 * or not, and columns on chrY / chrMT are called with HAPLOID forced (955-957).
 * PECALLER_DEVICE_GUIDE=1 (off by default): runs of BED lines go to the device as ranges of intervals and the columns are made
 * there (pecall_dev_call_records_guided; fill_guide_range below) instead of one position at a time.
 *
 * Not supported (an error, not a silent difference): more than 512 samples (up to 64 is the device caller's fast case).  `no_threads` - 1 threads (as many as the host has CPUs, at most 128) walk the pileup streams, format the rows and deflate <outfile>.base.gz.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ctype.h>
#include <stdint.h>
#include <dirent.h>
#include <errno.h>
#include <math.h>
#include <zlib.h>
#include <unistd.h>
#include <time.h>
#include "../../include/pemap_hip.h"
#include "host_io.h"
#include "pecall_row_len.h"
#include "pecall_gz_rule.h"

/* (weak: the program links against a library without this entry too -- an older build, or the tests' host-only stand-in -- and
   PECALLER_DEVICE_ROWS=1 then ends the run with a message) */
extern __typeof__ (pecall_dev_sites_base_text) pecall_dev_sites_base_text __attribute__ ((weak));
/* (weak for the same reason: PECALLER_DEVICE_GZ=1 ends the run with a message where the library lacks the entry) */
extern __typeof__ (pecall_dev_sites_base_gz) pecall_dev_sites_base_gz __attribute__ ((weak));
/* (weak for the same reason: PECALLER_DEVICE_GUIDE=1 ends the run with a message where the library lacks the entry) */
extern __typeof__ (pecall_dev_call_records_guided) pecall_dev_call_records_guided __attribute__ ((weak));

#define MAX_SAMPLES 512         /* PCS_MAXN of the device caller */
#define NA 6
#define MAX_DIST 501            /* pecaller.c:222 */
#define MAX_MT 128               /* threads of the merge and of the row formatting at most */

static void
die (const char *fmt, const char *arg)
{
  printf (fmt, arg);
  printf ("\n");
  exit (1);
}

static const char GEN[16] = "ACGTDIMRWSYKEHN";  /* int_to_gen, pecaller.c:2910-2943 */
static const char *TYPE_NAME[7] = { "", "SNP", "DEL", "INS", "LOW", "MULTIALLELIC", "MESS" };  /* pecaller.c:523-528 */

static int
gen_to_int (char c)             /* pecaller.c:2869-2907: an unknown letter ends the run */
{
  const char *p = c ? strchr (GEN, c) : NULL;
  if (!p)
    {
      printf ("\n This is impossible\n Illegal character in gen_to_int %c\n\n", c);
      exit (1);
    }
  return (int) (p - GEN);
}

/* pecaller's own find_chrom, pecaller.c:1793-1816 (not pemapper's) */
static int
find_chrom (const unsigned int *pos, int first, int last, int try, unsigned this)
{
  if (first == last)
    return first;
  if (first >= try)
    return this > pos[first] ? first + 1 : first;
  if (last <= try)
    return last;
  if (pos[try] < this)
    return find_chrom (pos, try, last, (last + try) / 2, this);
  if (pos[try] > this)
    return find_chrom (pos, first, try, (try + first) / 2, this);
  return try + 1;
}

typedef struct
{
  zreader f;                    /* the stream is inflated by a thread of its own (host_io.h) */
  unsigned int cur;             /* position of the pending record, 0 = exhausted (pecaller.c:840-849) */
  unsigned short data[NA];
  char name[256], file[256];
  /* .dist statistics, pecaller.c:884-889, 1077-1140 */
  double mean;
  unsigned int base_count, max_coverage, counts[MAX_DIST];
} sample_t;

/* the pending record consumed: read the next one (pecaller.c:891-907) -> 1 when the stream ended with this call */
static inline int
advance (sample_t * s)
{
  /* (gzeof / gzread of 4 then 12 bytes in the reference: the end of the stream is a read of nothing) */
  zreader *z = &s->f;
  if (z->pos + 16 <= z->cur_len)
    {
      const char *q = z->ring[z->head] + z->pos;
      memcpy (&s->cur, q, sizeof (unsigned int));
      memcpy (s->data, q + 4, sizeof (unsigned short) * NA);
      z->pos += 16;
      return 0;
    }
  if (zr_read (&s->f, &s->cur, sizeof (unsigned int)) != 0)
    {
      zr_read (&s->f, s->data, sizeof (unsigned short) * NA);
      return 0;
    }
  s->cur = 0;
  return 1;
}

typedef struct
{
  /* one tile of columns (T = the run's tile size) */
  uint16_t *reads;              /* [T][indiv][6] */
  uint8_t *ref_base, *chrom;
  char *ref_char;
  int *contig;
  unsigned int *pos;
  int8_t *call, *type;
  /* the posteriors that are not 1: the columns that have one (ascending) and their samples' posteriors (pecall_dev_call_sites_sparse) */
  uint32_t *post_site;
  double *post_rows;
  uint64_t n_post, post_cap;
  int32_t *ac, *denovo;
  long n;
  /* PECALLER_DEVICE_MERGE=1 (NULL otherwise): the range's records as the streams gave them, per sample, for pecall_dev_call_records;
     the columns come back with their slots, and `reads` holds the variant columns' rows only: column s has row vrow[s] */
  char *recs;                   /* [indiv][T] records of 16 bytes */
  uint64_t *n_recs;             /* [indiv] */
  uint8_t *chrom_slot;          /* [T]: chromosome class of position p0 + slot */
  uint32_t *col_slot, *vrow, *vlist;    /* [T] */
  unsigned int p0;
  int from_records;             /* this tile's columns are made on the device from `recs` (every tile under PECALLER_DEVICE_MERGE=1) */
  /* PECALLER_DEVICE_GUIDE=1 (NULL otherwise): a range of guide intervals for pecall_dev_call_records_guided -- interval k holds the
     slots [iv_first[k], iv_first[k] + iv_count[k]) of the range [p0, p0 + span) on contig iv_which[k]; `recs` holds the records at
     those slots only.  n_iv = 0: not such a tile (a line left to the per-position path fills `reads` as without the switch) */
  uint32_t *iv_first, *iv_count;        /* [T] */
  uint8_t *iv_chrom;
  int *iv_which;
  uint32_t n_iv, span;
  /* PECALLER_DEVICE_ROWS=1 (dtext NULL otherwise): the rows of <outfile>.base.gz as the device made them (pecall_dev_sites_base_text)
     -- those of the columns whose posteriors are all 1 -- and the holes: the host's row of column hole_site[k] (= post_site[k])
     belongs at byte hole_at[k] of dtext.  The rows stage notes where its row of hole k lies (hole_off: in the formatting thread's
     buffer; hole_src, hole_len) and how many bytes of host rows lie in front of it (hole_pre, one more entry than holes). */
  /* PECALLER_DEVICE_GZ=1 on top of it: dtext holds that text as the gzip members the device made of it (pecall_dev_sites_base_gz),
     n_dtext their bytes, n_inflated the text's; hole_at[k] is a member boundary of dtext, where the host's member of hole k belongs */
  char *dtext;
  uint64_t dtext_cap, n_dtext, n_inflated;
  int dtext_pinned;
  uint32_t *hole_site, *hole_len;
  uint64_t *hole_at, *hole_off, *hole_pre;
  const char **hole_src;
  uint64_t hole_cap, n_holes;
  /* the arrays that are page-locked (pecall_dev_pin_host took them): released before they are freed */
  const void *pinned[8];
  int n_pinned;
} tile_t;

/* The rows of <outfile>.base.gz are put together in memory and handed to the parallel gz writer tile by tile (host_io.h: gzip
   members, the same bytes after inflation as gzprintf would have produced, pecaller.c:1760-1775).  A posterior of exactly 1 --
   nearly all of them -- prints as "1" under %g and is written without going through printf. */
typedef struct
{
  char *p;
  size_t n, cap;
} sbuf;

static inline char *
sb_room (sbuf * b, size_t k)
{
  if (b->n + k > b->cap)
    {
      b->cap = 2 * (b->n + k) + (1 << 20);
      b->p = (char *) realloc (b->p, b->cap);
      if (!b->p)
        die ("\n pecaller_hip: out of memory for %s", "the output rows");
    }
  return b->p + b->n;
}

/* the row of column s in <outfile>.base.gz, appended to ob; p: the column's posteriors, NULL: all 1 */
static void
emit_base_row (const tile_t * t, long s, const double *p, int indiv, const char *frag, size_t fl, sbuf * ob)
{
  const int8_t *call = t->call + s * indiv;
  char *w = sb_room (ob, fl + 32 + (size_t) indiv * 32);
  char *w0 = w;
  *w++ = '\n';
  memcpy (w, frag, fl);
  w += fl;
  *w++ = '\t';
  w += sprintf (w, "%d", (int) t->pos[s]);
  *w++ = '\t';
  *w++ = t->ref_char[s];
  for (int i = 0; i < indiv; i++)
    {
      *w++ = '\t';
      if (call[i] < 14)
        {
          *w++ = GEN[call[i]];
          *w++ = '\t';
          if (!p || p[i] == 1.0)
            *w++ = '1';
          else
            w += sprintf (w, "%g", p[i]);
        }
      else
        {
          *w++ = 'N';
          *w++ = '\t';
          *w++ = '1';
        }
    }
  ob->n += (size_t) (w - w0);
}

/* rows of columns [s0, s1): <outfile>.base.gz text into ob, <outfile>.snp text into sb, <outfile>.piles.gz text into pb -> the number
   of columns that have a row in <outfile>.base.gz.  With the device's text (t->dtext) ob takes the holes' rows only. */
static long
emit_rows (const tile_t * t, long s0, long s1, int indiv, char **contig_names, sbuf * ob, sbuf * sb, sbuf * pb)
{
  char minor[80], am_count[80], tmp[64];
  long base_rows = 0;
  /* the first listed column at or behind s0 */
  uint64_t lp = 0, hi = t->n_post;
  while (lp < hi)
    {
      const uint64_t mid = (lp + hi) / 2;
      if ((long) t->post_site[mid] < s0)
        lp = mid + 1;
      else
        hi = mid;
    }
  for (long s = s0; s < s1; s++)
    {
      /* the column's posteriors: a row of the list, or all 1 (p = NULL) */
      const double *p = NULL;
      if (lp < t->n_post && (long) t->post_site[lp] == s)
        p = t->post_rows + (size_t) lp++ * indiv;
      if (t->type[s] < 0)
        continue;               /* reference base not A/C/G/T: the worker skips the column (pecaller.c:1208, 1718) */
      const char *frag = contig_names[t->contig[s]];
      const int8_t *call = t->call + s * indiv;
      const size_t fl = strlen (frag);
      base_rows++;
      if (!t->dtext)
        emit_base_row (t, s, p, indiv, frag, fl, ob);
      else if (p)
        {
          /* a hole of the device's text: list entry lp - 1 */
          t->hole_off[lp - 1] = ob->n;
          emit_base_row (t, s, p, indiv, frag, fl, ob);
          t->hole_len[lp - 1] = (uint32_t) (ob->n - t->hole_off[lp - 1]);
        }
      if (t->type[s] == 0)
        continue;
      minor[0] = am_count[0] = '\0';
      for (int a = 0; a < NA; a++)
        if (t->ac[s * NA + a] > 0)
          {
            sprintf (tmp, "%c,", GEN[a]);
            strcat (minor, tmp);
            sprintf (tmp, "%d,", t->ac[s * NA + a]);
            strcat (am_count, tmp);
          }
      if (minor[0])
        {
          minor[strlen (minor) - 1] = '\0';
          am_count[strlen (am_count) - 1] = '\0';
        }
      sb->n += (size_t) sprintf (sb_room (sb, fl + 256), "\n%s\t%d\t%c\t%s\t%s\t%s%s", frag, (int) t->pos[s], t->ref_char[s], minor, am_count,
                                 t->denovo[s] > 0 ? "DENOVO_" : "", TYPE_NAME[t->type[s]]);
      pb->n += (size_t) sprintf (sb_room (pb, fl + 64), "\n%s\t%d\t%c", frag, (int) t->pos[s], t->ref_char[s]);
      for (int i = 0; i < indiv; i++)
        {
          sb->n += (size_t) sprintf (sb_room (sb, 64), "\t%c\t%g", GEN[call[i]], p ? p[i] : 1.0);
          const uint16_t *r = t->reads + ((size_t) (t->from_records ? t->vrow[s] : (uint32_t) s) * indiv + i) * NA;
          for (int a = 0; a < NA; a++)
            pb->n += (size_t) sprintf (sb_room (pb, 16), "\t%d", (int) r[a]);
        }
    }
  return base_rows;
}

/* ---- what a run is made of.  The reference, read-only once the .sdx and the .seq are loaded: the merge threads and both stages of
        the pipeline point to this one description */
typedef struct
{
  const unsigned int *frag_pos; /* [-1 .. no_contigs): contig ends in .seq coordinates (length + 15 each), [-1] = 0 */
  char **contig_names;
  uint8_t *chrom_type;          /* AUTO 0, CHRX 1, CHRY 2, CHRMT 3 (pecaller.c:98-101) */
  char *genome;                 /* the whole .seq */
  size_t gsize;
  int no_contigs, start_chrom;  /* start_chrom: find_chrom's first try */
} ref_t;

typedef struct run_s run_t;
typedef struct
{
  const run_t *r;
  const tile_t *t;
  long s0, s1, base_rows;
  sbuf ob, sb, pb;              /* (kept from tile to tile) */
  /* the splice of the device's text and the holes' rows: bytes [lo, hi) of the text and the holes that belong in front of them (the
     last job: also those at the text's end), to their places in out */
  uint64_t lo, hi;
  int last;
  char *out;
} emit_job;

/* a merge thread's view of the range being walked */
typedef struct
{
  run_t *r;
  tile_t *t;                    /* the tile the main thread fills */
  int k;
  unsigned int p0;              /* the range of genome positions [p0, p1) */
  unsigned long long p1;
  int guide, gwhich;            /* a stretch of a BED interval (pecaller.c:941-1039): EVERY position is a column, on contig gwhich */
  long col0;                    /* the range's columns are appended to the tile from col0 on */
  /* out: the last slot at which one of this thread's streams, live when the walk began, came to its end (-1: none did) */
  long end_slot;
} merge_ctx;

/* ---- the device call of a tile and its text run on a thread each while the main thread merges the next tile: three sets of tile
        arrays go round (merge -> device -> rows -> free) */
#define N_TILES 3
typedef struct
{
  pthread_mutex_t mu;
  pthread_cond_t cv;
  tile_t free_tile[N_TILES];
  int n_free;
} tile_pool;

typedef struct
{
  pthread_t th;
  pthread_mutex_t mu;
  pthread_cond_t cv;
  int has_job, busy, stop;
  tile_t job;
  int role;                     /* 0: the device call, then on to the rows' stage; 1: the rows, then back to the pool */
  run_t *r;
  double sec;                   /* spent on its tiles */
} stage_t;

#define RC_UNORDERED 77
struct run_s
{
  /* the command line */
  int argc;
  char **argv;
  int no_threads, use_ped, haploid;
  double threshold, theta, denovo_rate;
  FILE *guide_file;
  /* serial_merge: the streams are merged the reference's way, one column at a time from the lowest pending position of all streams
     (find_lowest, pecaller.c:865-923, 1820-1833), whatever order the records come in; otherwise by the parallel walk.  device_merge
     (PECALLER_DEVICE_MERGE=1): a range's columns are made on the device from the streams' records; not with a guide file or serial_merge */
  int serial_merge, device_merge;
  /* device_guide (PECALLER_DEVICE_GUIDE=1, with a guide file, not under serial_merge): runs of BED lines go to the device as ranges of
     intervals (fill_guide_range).  gline: BED lines read so far; gline_judged / gline_host: the line at hand has been looked at, and
     is left to the per-position path; gline_taken: the last line counted in dg_ivs; gbad: the line names no contig of the .sdx (the
     run ends with the reference's message when the walk gets to it); guide_done: the file has no further line */
  int device_guide, gline_host, gbad, guide_done;
  long gline, gline_judged, gline_taken;
  char gbad_name[256];
  long dg_cols, dg_ivs, dg_ranges;
  /* device_rows (PECALLER_DEVICE_ROWS=1): the rows of <outfile>.base.gz whose posteriors are all 1 are made on the device behind each
     tile's call (pecall_dev_sites_base_text); names / name_off: the contig names as that call takes them */
  int device_rows;
  char *names;
  uint32_t *name_off;
  size_t max_name;
  long rows_dev, rows_hole;
  /* device_gz (PECALLER_DEVICE_GZ=1, with device_rows): that text is deflated on the device too and goes to the file as it comes back;
     the host's rows of the holes go in between as members of stored blocks (gzb: the one being put together) */
  int device_gz;
  unsigned long long gz_text, gz_bytes;
  /* set once (start_pipeline).  tile: columns per device call, and genome positions per range of the stream merge -- a call has a fixed
     part (two kernel launches, the transfers' latencies), so tiles are large.  mg_chunk: slots per work item of the column pass.
     guide_range_min: positions of a guide interval left from which the streams are walked in parallel.  post_cap: a tile's first list */
  size_t tile, mg_chunk;
  unsigned long long guide_range_min;
  uint64_t post_cap;
  /* the outputs */
  pgz outfile;
  FILE *snpfile, *distfile;
  gzFile pilefile;
  sbuf ob;                      /* rows of <outfile>.base.gz on their way to the gz writer */
  sbuf gzb;
  ref_t ref;
  sample_t *sm;
  int indiv;
  pecall_dev *pc;
  tile_pool pool;
  stage_t dev_stage, row_stage;
  int MT;                       /* the threads of the merge and of the row formatting */
  merge_ctx mc[MAX_MT];
  emit_job jobs[MAX_MT];
  uint16_t *planes;             /* [indiv][tile][NA] */
  uint8_t *marks;               /* [MT][tile]: a stream of thread k has a record at the slot */
  long *chunk_base;             /* column of the first marked slot of each chunk of mg_chunk slots */
  /* set by the stream walk (and by the device stage, on the library's word) when a stream does not ascend: the run is abandoned */
  volatile int unordered;
  /* the walk: streams still open; guide mode: the current interval [lowest, gend] of contig gwhich (pecaller.c:927-953, 1040-1066) */
  int running, gwhich;
  unsigned int lowest, gend, tot_bases;
  long tot_cols, dev_cols, dev_ranges;
  double sec_merge, sec_wait;
  struct timespec tstart;
};

static double
seconds_between (const struct timespec *a, const struct timespec *b)
{
  return (double) (b->tv_sec - a->tv_sec) + 1e-9 * (double) (b->tv_nsec - a->tv_nsec);
}

static void *
emit_thread (void *arg)
{
  emit_job *j = (emit_job *) arg;
  j->base_rows = emit_rows (j->t, j->s0, j->s1, j->r->indiv, j->r->ref.contig_names, &j->ob, &j->sb, &j->pb);
  return NULL;
}

/* bytes [lo, hi) of the device's text go to out, each behind the host rows that belong in front of it; the rows of the holes at
   lo <= hole_at < hi (the last job: <= hi) go in between */
static void *
splice_thread (void *arg)
{
  const emit_job *j = (const emit_job *) arg;
  const tile_t *t = j->t;
  uint64_t k = 0, top = t->n_holes, cur = j->lo;
  while (k < top)               /* the first hole at or behind lo */
    {
      const uint64_t mid = (k + top) / 2;
      if (t->hole_at[mid] < j->lo)
        k = mid + 1;
      else
        top = mid;
    }
  for (; k < t->n_holes && (t->hole_at[k] < j->hi || (j->last && t->hole_at[k] == j->hi)); k++)
    {
      memcpy (j->out + cur + t->hole_pre[k], t->dtext + cur, (size_t) (t->hole_at[k] - cur));
      cur = t->hole_at[k];
      memcpy (j->out + cur + t->hole_pre[k], t->hole_src[k], t->hole_len[k]);
    }
  memcpy (j->out + cur + t->hole_pre[k], t->dtext + cur, (size_t) (j->hi - cur));
  return NULL;
}

static void
run_jobs (void *(*fn) (void *), emit_job * jobs, int threads)
{
  pthread_t th[MAX_MT];
  for (int k = 1; k < threads; k++)
    if (pthread_create (&th[k], NULL, fn, &jobs[k]))
      die ("\n pecaller_hip: can not start %s", "a formatting thread");
  fn (&jobs[0]);
  for (int k = 1; k < threads; k++)
    pthread_join (th[k], NULL);
}

/* <outfile>.base.gz text of a tile whose template rows came from the device: the device's text with the rows the formatting threads
   made of the holes put in at their places, appended to r->ob.  With device_gz: the holes' rows are found and counted, nothing is
   copied. */
static void
splice_tile (run_t * r, const tile_t * t, int threads)
{
  emit_job *jobs = r->jobs;
  if (t->n_holes != t->n_post)
    die ("\n pecaller_hip: %s", "the device's text leaves other rows to the host than the call listed");
  uint64_t pre = 0;
  int j = 0;
  for (uint64_t k = 0; k < t->n_holes; k++)
    {
      if (t->hole_site[k] != t->post_site[k])
        die ("\n pecaller_hip: %s", "the device's text leaves other rows to the host than the call listed");
      while (j < threads - 1 && (long) t->hole_site[k] >= jobs[j].s1)
        j++;
      t->hole_src[k] = jobs[j].ob.p + t->hole_off[k];
      t->hole_pre[k] = pre;
      pre += t->hole_len[k];
    }
  t->hole_pre[t->n_holes] = pre;
  if (r->device_gz)
    {
      /* (the members and the holes' rows go to the file one behind the other: write_tile) */
      long base_rows = 0;
      for (int k = 0; k < threads; k++)
        base_rows += jobs[k].base_rows;
      r->rows_hole += (long) t->n_holes;
      r->rows_dev += base_rows - (long) t->n_holes;
      return;
    }
  const uint64_t total = t->n_dtext + pre;
  char *out = sb_room (&r->ob, (size_t) total);
  for (int k = 0; k < threads; k++)
    {
      jobs[k].out = out;
      jobs[k].lo = t->n_dtext * (uint64_t) k / (uint64_t) threads;
      jobs[k].hi = t->n_dtext * (uint64_t) (k + 1) / (uint64_t) threads;
      jobs[k].last = k == threads - 1;
    }
  run_jobs (splice_thread, jobs, threads);
  r->ob.n += (size_t) total;
  long base_rows = 0;
  for (int k = 0; k < threads; k++)
    base_rows += jobs[k].base_rows;
  r->rows_hole += (long) t->n_holes;
  r->rows_dev += base_rows - (long) t->n_holes;
}

/* the rows of a tile, formatted by the run's MT threads (contiguous runs of columns, put together in column order) */
static void
emit_tile (run_t * r, const tile_t * t)
{
  emit_job *jobs = r->jobs;
  const int threads = t->n < 4096 ? 1 : r->MT;
  for (int k = 0; k < threads; k++)
    {
      jobs[k].r = r;
      jobs[k].t = t;
      jobs[k].s0 = t->n * k / threads;
      jobs[k].s1 = t->n * (k + 1) / threads;
      jobs[k].ob.n = jobs[k].sb.n = jobs[k].pb.n = 0;
    }
  run_jobs (emit_thread, jobs, threads);
  if (t->dtext)
    splice_tile (r, t, threads);
  for (int k = 0; k < threads; k++)
    {
      if (!t->dtext)
        {
          memcpy (sb_room (&r->ob, jobs[k].ob.n), jobs[k].ob.p, jobs[k].ob.n);
          r->ob.n += jobs[k].ob.n;
        }
      if (jobs[k].sb.n)
        fwrite (jobs[k].sb.p, 1, jobs[k].sb.n, r->snpfile);
      if (jobs[k].pb.n)
        gzwrite (r->pilefile, jobs[k].pb.p, (unsigned) jobs[k].pb.n);
    }
}

/* ---- a column's head: reference letter and its number, contig (which, or looked up when which < 0) and position in the contig */
static inline void
column_header (const ref_t * g, tile_t * t, long col, unsigned int lowest, int which)
{
  if (which < 0)
    which = find_chrom (g->frag_pos, 0, g->no_contigs - 1, g->start_chrom, lowest);
  const char ref = lowest < g->gsize ? g->genome[lowest] : '\0';
  t->ref_char[col] = ref;
  t->ref_base[col] = (uint8_t) gen_to_int (ref);
  t->contig[col] = which;
  t->pos[col] = 1 + lowest - g->frag_pos[which - 1];
}

/* the chromosome class the caller gets; with a guide file chrY / chrMT columns are called with HAPLOID forced (+ 16, pecaller.c:955-957) */
static inline uint8_t
chrom_class (const ref_t * g, int which, int guide)
{
  const uint8_t c = g->chrom_type[which];
  return c | ((guide && (c == 2 || c == 3)) ? 16 : 0);
}

/* ---- the merge of the pileup streams without a guide file, a range of genome positions at a time.  The reference's dispatcher
        (find_lowest / the per-column loop, pecaller.c:891-1039, 1820-1833) takes the lowest pending position of all streams, makes
        a column of it from the streams that have a record there, and advances those: for streams in ascending order (as pemapper
        writes them) the columns are the union of the positions, each sample's counts where it has a record and zeros where it
        has none.  Here every stream is walked on its own over the positions [p0, p0 + tile) into a plane of its own (a thread
        takes several streams; the statistics of <outfile>.dist are per stream and see the same records in the same order), and
        the planes are put together column by column, positions without any record left out.

        walk_streams is that walk for one thread's streams, in two forms chosen at compile time; both keep the stream's own part (the
        statistics of <outfile>.dist, the pending record, the end of the stream, the check of the order).  to_records = 0: the counters
        go to the stream's plane, zeros between them, and their slots are marked.  to_records = 1 (PECALLER_DEVICE_MERGE=1): the records
        are appended to the sample's buffer of the tile as they are; the columns are made on the device (pecall_dev_call_records).
        to_records = 2 (PECALLER_DEVICE_GUIDE=1): the same over a range of guide intervals (the tile's iv_first / iv_count), from the
        first guided position p0 to the last one, p1 - 1.  The reference's loop (pecaller.c:975-1029) is the specification: records in
        front of a guided position are read past without a word, so only the records at guided positions are appended and feed the
        statistics; those in the gaps between the range's intervals are passed over (still checked for their order); those behind p1
        stay pending, for the next range's leading skip.  The positions seen (base_count) are the range's columns for every sample,
        open or not: fill_guide_range adds them, behind the cut at the end of the streams. */
static inline __attribute__ ((always_inline)) void
walk_streams (merge_ctx * c, const int mode)
{
  const int to_records = mode != 0, guided = mode == 2;
  run_t *r = c->r;
  const size_t tile = r->tile;
  const unsigned int p0 = c->p0;
  const unsigned long long p1 = c->p1;
  uint8_t *mark = NULL;
  if (!to_records)
    {
      mark = r->marks + (size_t) c->k * tile;
      memset (mark, 0, tile);
      if (c->guide && c->k == 0)
        memset (mark, 1, (size_t) (p1 - p0));
    }
  c->end_slot = -1;
  for (int i = c->k; i < r->indiv; i += r->MT)
    {
      sample_t *s = &r->sm[i];
      uint16_t *plane = to_records ? NULL : r->planes + (size_t) i * tile * NA;
      char *out = to_records ? c->t->recs + (size_t) i * tile * 16 : NULL;
      size_t done = 0;          /* slots of the range passed so far: the next record lies at p0 + done or behind */
      const int live = s->cur != 0;
      if (c->guide)
        {
          /* records in front of the interval are passed over (pecaller.c:975-976); every position of the stretch counts as seen */
          while (s->cur != 0 && s->cur < p0)
            advance (s);
          if (!to_records)
            s->base_count += (unsigned int) (p1 - p0);
        }
      const uint32_t *iv_first = guided ? c->t->iv_first : NULL, *iv_count = guided ? c->t->iv_count : NULL;
      const uint32_t n_iv = guided ? c->t->n_iv : 0;
      uint32_t iv = 0;          /* guided: the first interval that ends behind the slot at hand */
      /* The records of the range.  The pending one first (s->cur / s->data); then straight out of the inflater's block as long as whole
         records lie in it -- 64 of these loops are the merge's time: one load of the position, the six counters copied as 8 + 4
         bytes, their sum for the stream's statistics.  (The coverage total is a sum of integers: it is kept in an integer and added
         to the double once per range; every partial sum is far below 2^53, so the double is the same.) */
      unsigned long long cov_sum = 0;
      unsigned int cov_max = s->max_coverage;
      size_t n_rec = 0;
      zreader *z = &s->f;
      while (s->cur != 0 && (unsigned long long) s->cur < p1)
        {
          unsigned int pos = s->cur;
          const char *rec = NULL;       /* NULL: the counters are in s->data */
          for (;;)
            {
              if ((unsigned long long) pos < (unsigned long long) p0 + done)
                {
                  /* a record at or in front of the stream's previous one: the parallel walk rests on ascending streams (as pemapper
                     writes them); the run starts over with the reference's own dispatcher, which takes what comes (main) */
                  r->unordered = 1;
                  return;
                }
              const size_t slot = (size_t) (pos - p0);
              int take = 1;
              if (guided)
                {
                  while (iv < n_iv && (size_t) iv_first[iv] + iv_count[iv] <= slot)
                    iv++;
                  take = iv < n_iv && slot >= iv_first[iv];
                }
              if (take)
                {
                  uint16_t cnt[NA];
                  memcpy (cnt, rec ? (const void *) (rec + 4) : (const void *) s->data, sizeof cnt);
                  if (to_records)
                    {
                      char *dst = out + n_rec * 16;
                      memcpy (dst, &pos, sizeof pos);
                      memcpy (dst + 4, cnt, sizeof cnt);
                    }
                  else
                    {
                      if (slot != done)
                        memset (plane + done * NA, 0, (slot - done) * NA * sizeof (uint16_t));
                      memcpy (plane + slot * NA, cnt, sizeof cnt);
                      mark[slot] = 1;
                    }
                  const unsigned int cov = (unsigned int) cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4] + cnt[5];
                  cov_sum += cov;
                  if (cov > cov_max)
                    cov_max = cov;
                  s->counts[cov < MAX_DIST - 1 ? cov : MAX_DIST - 1]++;
                  n_rec++;
                }
              done = slot + 1;
              /* the next record, if it lies whole in the block at hand and belongs to the range */
              if (z->pos + 16 > z->cur_len)
                break;
              rec = z->ring[z->head] + z->pos;
              memcpy (&pos, rec, sizeof pos);
              if (pos == 0 || (unsigned long long) pos >= p1)
                break;          /* (left where it is: advance below reads it as the pending record) */
              z->pos += 16;
            }
          advance (s);
        }
      s->mean += (double) cov_sum;
      s->max_coverage = cov_max;
      if (!c->guide)
        s->base_count += (unsigned int) n_rec;
      if (to_records)
        {
          c->t->n_recs[i] = n_rec;
          /* guided: the stream ended inside this range, at the column of the first guided position at or behind its last record
             (pecaller.c:975-1023: read past in front of that position, or taken at it) -- all its records lying in front of the range,
             at the range's first position.  There is such a position: the record lies in front of p1, the last one's successor */
          if (guided && live && s->cur == 0)
            {
              const size_t at = done ? done - 1 : 0;
              uint32_t k = 0;
              while (k + 1 < n_iv && (size_t) iv_first[k] + iv_count[k] <= at)
                k++;
              const long col_at = at > iv_first[k] ? (long) at : (long) iv_first[k];
              if (col_at > c->end_slot)
                c->end_slot = col_at;
            }
          continue;
        }
      memset (plane + done * NA, 0, (tile - done) * NA * sizeof (uint16_t));
      /* the stream ended inside this range: at the slot of its last record, or -- all its records lying in front of the range -- at
         the range's first position, where the reference reads past them (pecaller.c:975-993) */
      if (live && s->cur == 0)
        {
          const long at = done ? (long) done - 1 : 0;
          if (at > c->end_slot)
            c->end_slot = at;
        }
    }
}

static void *
merge_streams (void *arg)
{
  walk_streams ((merge_ctx *) arg, 0);
  return NULL;
}

static void *
merge_streams_dev (void *arg)
{
  walk_streams ((merge_ctx *) arg, 1);
  return NULL;
}

static void *
merge_streams_guided (void *arg)
{
  walk_streams ((merge_ctx *) arg, 2);
  return NULL;
}

static int
slot_marked (const run_t * r, size_t slot)
{
  for (int k = 0; k < r->MT; k++)
    if (r->marks[(size_t) k * r->tile + slot])
      return 1;
  return 0;
}

static void *
merge_count (void *arg)
{
  merge_ctx *c = (merge_ctx *) arg;
  const run_t *r = c->r;
  for (size_t ch = (size_t) c->k; ch < r->tile / r->mg_chunk; ch += (size_t) r->MT)
    {
      long n = 0;
      for (size_t slot = ch * r->mg_chunk; slot < (ch + 1) * r->mg_chunk; slot++)
        n += slot_marked (r, slot);
      r->chunk_base[ch] = n;
    }
  return NULL;
}

static void *
merge_columns (void *arg)
{
  merge_ctx *c = (merge_ctx *) arg;
  const run_t *r = c->r;
  tile_t *t = c->t;
  for (size_t ch = (size_t) c->k; ch < r->tile / r->mg_chunk; ch += (size_t) r->MT)
    {
      long col = c->col0 + r->chunk_base[ch];
      for (size_t slot = ch * r->mg_chunk; slot < (ch + 1) * r->mg_chunk; slot++)
        if (slot_marked (r, slot))
          {
            column_header (&r->ref, t, col, c->p0 + (unsigned int) slot, c->guide ? c->gwhich : -1);
            t->chrom[col] = chrom_class (&r->ref, t->contig[col], c->guide);
            uint16_t *dst = t->reads + (size_t) col * r->indiv * NA;
            for (int i = 0; i < r->indiv; i++)
              memcpy (dst + (size_t) i * NA, r->planes + ((size_t) i * r->tile + slot) * NA, NA * sizeof (uint16_t));
            col++;
          }
    }
  return NULL;
}

static void
run_threads (void *(*fn) (void *), run_t * r)
{
  pthread_t th[MAX_MT];
  for (int k = 1; k < r->MT; k++)
    if (pthread_create (&th[k], NULL, fn, &r->mc[k]))
      die ("\n pecaller_hip: can not start %s", "a merge thread");
  fn (&r->mc[0]);
  for (int k = 1; k < r->MT; k++)
    pthread_join (th[k], NULL);
}

/* the columns of the range the streams were just walked over, appended to the tile: count, running sum, columns */
static void
walked_columns (run_t * r, tile_t * t)
{
  run_threads (merge_count, r);
  long ncol = 0;
  for (size_t ch = 0; ch < r->tile / r->mg_chunk; ch++)
    {
      const long n = r->chunk_base[ch];
      r->chunk_base[ch] = ncol;
      ncol += n;
    }
  run_threads (merge_columns, r);
  t->n += ncol;
  r->tot_bases += (unsigned int) ncol;
}

static void
pool_put (tile_pool * p, tile_t t)
{
  pthread_mutex_lock (&p->mu);
  p->free_tile[p->n_free++] = t;
  pthread_cond_broadcast (&p->cv);
  pthread_mutex_unlock (&p->mu);
}

static tile_t
pool_get (tile_pool * p)
{
  pthread_mutex_lock (&p->mu);
  while (p->n_free == 0)
    pthread_cond_wait (&p->cv, &p->mu);
  tile_t t = p->free_tile[--p->n_free];
  pthread_mutex_unlock (&p->mu);
  t.n = 0;
  t.n_iv = 0;
  t.from_records = 0;
  return t;
}

static void
stage_wait_idle (stage_t * c)
{
  pthread_mutex_lock (&c->mu);
  while (c->has_job || c->busy)
    pthread_cond_wait (&c->cv, &c->mu);
  pthread_mutex_unlock (&c->mu);
}

/* hand a tile to a stage (waits until the stage has given its previous one away) */
static void
stage_give (stage_t * c, tile_t t)
{
  stage_wait_idle (c);
  pthread_mutex_lock (&c->mu);
  c->job = t;
  c->has_job = 1;
  pthread_cond_broadcast (&c->cv);
  pthread_mutex_unlock (&c->mu);
}

static int
device_call (run_t * r, tile_t * t)
{
  if (!t->from_records)
    return pecall_dev_call_sites_sparse (r->pc, t->reads, t->ref_base, t->chrom, t->n, r->indiv, r->haploid, r->threshold, r->theta, t->call,
                                         t->post_site, t->post_rows, t->post_cap, &t->n_post, t->type, t->ac, NULL, t->denovo);
  const void *ptr[MAX_SAMPLES];
  for (int i = 0; i < r->indiv; i++)
    ptr[i] = t->recs + (size_t) i * r->tile * 16;
  const size_t left = (size_t) t->p0 < r->ref.gsize ? r->ref.gsize - t->p0 : 0;
  t->n = 0;
  if (t->n_iv)
    return pecall_dev_call_records_guided (r->pc, ptr, t->n_recs, r->indiv, t->p0, t->span, r->ref.genome + (left ? t->p0 : 0), (uint32_t) (left < t->span ? left : t->span),
                                           t->iv_first, t->iv_count, t->iv_chrom, t->n_iv, &t->n, t->col_slot, r->haploid, r->threshold, r->theta, t->call, t->post_site,
                                           t->post_rows, t->post_cap, &t->n_post, t->type, t->ac, NULL, t->denovo);
  return pecall_dev_call_records (r->pc, ptr, t->n_recs, r->indiv, t->p0, (uint32_t) r->tile, r->ref.genome + (left ? t->p0 : 0),
                                  (uint32_t) (left < r->tile ? left : r->tile), t->chrom_slot, &t->n, t->col_slot, r->haploid, r->threshold, r->theta,
                                  t->call, t->post_site, t->post_rows, t->post_cap, &t->n_post, t->type, t->ac, NULL, t->denovo);
}

/* behind pecall_dev_call_records: the columns' heads from their slots (what merge_columns fills on the host path; an illegal
   reference letter ends the run here as it does there), and the variant columns' reads for the rows of <outfile>.piles.gz.
   Behind pecall_dev_call_records_guided the contig is the interval's (the BED line's, pecaller.c:964-965), found by a walk along
   the range's intervals beside the columns. */
static void
device_merge_columns (run_t * r, tile_t * t)
{
  long nv = 0;
  uint32_t k = 0;
  for (long col = 0; col < t->n; col++)
    {
      while (k + 1 < t->n_iv && t->col_slot[col] >= t->iv_first[k] + t->iv_count[k])
        k++;
      column_header (&r->ref, t, col, t->p0 + t->col_slot[col], t->n_iv ? t->iv_which[k] : -1);
      if (t->type[col] > 0)
        {
          t->vrow[col] = (uint32_t) nv;
          t->vlist[nv++] = (uint32_t) col;
        }
    }
  if (nv && pecall_dev_sites_gather (r->pc, t->vlist, (uint64_t) nv, t->reads, NULL, NULL))
    die ("\n pecaller_hip: %s", pecall_dev_last_error (r->pc));
  if (t->n_iv)
    {
      r->dg_cols += t->n;
      r->dg_ranges++;
      return;
    }
  r->dev_cols += t->n;
  r->dev_ranges++;
}

/* the tile's page-locked text buffer, and its hole lists with what the rows stage notes per hole: made anew for `cap` (the arrays
   hold nothing that is still needed when they grow) */
static void
tile_text_alloc (run_t * r, tile_t * t, uint64_t cap)
{
  if (t->dtext_pinned)
    (void) pecall_dev_unpin_host (r->pc, t->dtext);
  free (t->dtext);
  t->dtext = (char *) malloc ((size_t) cap);
  if (!t->dtext)
    die ("\n pecaller_hip: out of memory for %s", "the device's text");
  t->dtext_cap = cap;
  t->dtext_pinned = pecall_dev_pin_host (r->pc, t->dtext, cap) == 0;
}

static void
tile_holes_alloc (tile_t * t, uint64_t cap)
{
  void *old[] = { t->hole_site, t->hole_len, t->hole_at, t->hole_off, t->hole_pre, (void *) t->hole_src };
  for (size_t k = 0; k < sizeof old / sizeof old[0]; k++)
    free (old[k]);
  t->hole_site = (uint32_t *) malloc ((size_t) cap * sizeof (uint32_t));
  t->hole_len = (uint32_t *) malloc ((size_t) cap * sizeof (uint32_t));
  t->hole_at = (uint64_t *) malloc ((size_t) cap * sizeof (uint64_t));
  t->hole_off = (uint64_t *) malloc ((size_t) cap * sizeof (uint64_t));
  t->hole_pre = (uint64_t *) malloc ((size_t) (cap + 1) * sizeof (uint64_t));
  t->hole_src = (const char **) malloc ((size_t) cap * sizeof (const char *));
  if (!t->hole_site || !t->hole_len || !t->hole_at || !t->hole_off || !t->hole_pre || !t->hole_src)
    die ("\n pecaller_hip: out of memory for %s", "the list of rows left to the host");
  t->hole_cap = cap;
}

/* behind the tile's call, its heads filled: the template rows of <outfile>.base.gz from the device.  A buffer that is too small is
   made anew with the size the call asked for, and once more (as call_tile does with the list of posteriors) */
static void
device_text (run_t * r, tile_t * t)
{
  t->n_dtext = t->n_holes = t->n_inflated = 0;
  if (t->n <= 0)
    return;
  for (int again = 0;; again++)
    {
      const int rc = r->device_gz
        ? pecall_dev_sites_base_gz (r->pc, r->names, r->name_off, r->ref.no_contigs, t->contig, t->pos, t->ref_char, (unsigned char *) t->dtext, t->dtext_cap, &t->n_dtext,
                                    t->hole_site, t->hole_at, t->hole_cap, &t->n_holes, &t->n_inflated, NULL)
        : pecall_dev_sites_base_text (r->pc, r->names, r->name_off, r->ref.no_contigs, t->contig, t->pos, t->ref_char, t->dtext, t->dtext_cap, &t->n_dtext,
                                      t->hole_site, t->hole_at, t->hole_cap, &t->n_holes, NULL);
      if (!rc)
        return;
      if (again || (t->n_dtext <= t->dtext_cap && t->n_holes <= t->hole_cap))
        die ("\n pecaller_hip: %s", pecall_dev_last_error (r->pc));
      if (t->n_holes > t->hole_cap)
        tile_holes_alloc (t, t->n_holes + t->n_holes / 8 + 1024);
      if (t->n_dtext > t->dtext_cap)
        tile_text_alloc (r, t, t->n_dtext + t->n_dtext / 8 + 4096);
    }
}

static void
call_tile (run_t * r, tile_t * t)
{
  int rc = device_call (r, t);
  if (rc && t->n_post > t->post_cap)
    {
      /* more columns with a posterior that is not 1 than the list holds (one per 8 columns to begin with): a list of the size
         the call asked for, and once more */
      t->post_cap = t->n_post + t->n_post / 8 + 1024;
      t->post_site = (uint32_t *) realloc (t->post_site, t->post_cap * sizeof (uint32_t));
      t->post_rows = (double *) realloc (t->post_rows, t->post_cap * (size_t) r->indiv * sizeof (double));
      if (!t->post_site || !t->post_rows)
        die ("\n pecaller_hip: out of memory for %s", "the list of posteriors");
      rc = device_call (r, t);
    }
  if (rc == PECALL_RC_UNORDERED && t->from_records)
    {
      /* (the walk's own check comes first: this is the library's word for the same thing) */
      r->unordered = 1;
      t->n = 0;
      t->n_post = 0;
    }
  else if (rc)
    die ("\n pecaller_hip: %s", pecall_dev_last_error (r->pc));
  else if (t->from_records)
    device_merge_columns (r, t);
  if (r->device_rows)
    device_text (r, t);
}

/* the rows of holes [k0, k1), which belong at one place, as one gzip member of stored blocks (pecall_gz_rule.h's ten bytes in front,
   zlib's crc32 behind): no deflateInit per hole */
static void
hole_member (run_t * r, const tile_t * t, uint64_t k0, uint64_t k1)
{
  sbuf *b = &r->gzb;
  uint64_t bytes = 0;
  uLong crc = crc32 (0L, Z_NULL, 0);
  for (uint64_t k = k0; k < k1; k++)
    bytes += t->hole_len[k];
  b->n = 0;
  unsigned char *w = (unsigned char *) sb_room (b, (size_t) (PCG_HEAD + bytes + 5u * (bytes / 65535u + 1u) + PCG_TAIL));
  for (uint32_t k = 0; k < PCG_HEAD; k++)
    *w++ = pcg_head_byte (k);
  /* stored blocks of 65,535 bytes at most, filled from the rows one behind the other */
  uint64_t left = bytes, k = k0;
  uint32_t in_row = 0;
  do
    {
      const uint32_t n = left > 65535u ? 65535u : (uint32_t) left;
      *w++ = left == n;
      *w++ = (unsigned char) n;
      *w++ = (unsigned char) (n >> 8);
      *w++ = (unsigned char) ~n;
      *w++ = (unsigned char) (~n >> 8);
      for (uint32_t have = 0; have < n;)
        {
          if (in_row == t->hole_len[k])
            {
              k++;
              in_row = 0;
              continue;
            }
          const uint32_t m = t->hole_len[k] - in_row < n - have ? t->hole_len[k] - in_row : n - have;
          memcpy (w, t->hole_src[k] + in_row, m);
          crc = crc32 (crc, (const Bytef *) w, m);
          w += m;
          in_row += m;
          have += m;
        }
      left -= n;
    }
  while (left);
  for (int x = 0; x < 4; x++)
    *w++ = (unsigned char) (crc >> (8 * x));
  for (int x = 0; x < 4; x++)
    *w++ = (unsigned char) (bytes >> (8 * x));
  b->n = (size_t) (w - (unsigned char *) b->p);
  if (fwrite (b->p, 1, b->n, r->outfile.f) != b->n)
    die ("\n pecaller_hip: write to %s.base.gz failed", r->argv[4]);
}

/* device_gz: the device's members to the file as they are, the holes' rows as members of the host's making at their places */
static void
write_tile_gz (run_t * r, const tile_t * t)
{
  uint64_t cur = 0;
  for (uint64_t k = 0; k < t->n_holes;)
    {
      uint64_t k1 = k + 1;
      while (k1 < t->n_holes && t->hole_at[k1] == t->hole_at[k])
        k1++;
      if (t->hole_at[k] < cur || t->hole_at[k] > t->n_dtext)
        die ("\n pecaller_hip: %s", "a hole's place among the device's members descends or lies beyond them");
      if (t->hole_at[k] > cur && fwrite (t->dtext + cur, 1, (size_t) (t->hole_at[k] - cur), r->outfile.f) != t->hole_at[k] - cur)
        die ("\n pecaller_hip: write to %s.base.gz failed", r->argv[4]);
      cur = t->hole_at[k];
      hole_member (r, t, k, k1);
      k = k1;
    }
  if (t->n_dtext > cur && fwrite (t->dtext + cur, 1, (size_t) (t->n_dtext - cur), r->outfile.f) != t->n_dtext - cur)
    die ("\n pecaller_hip: write to %s.base.gz failed", r->argv[4]);
  if (t->n_dtext || t->n_holes)
    r->outfile.wrote_any = 1;
  r->gz_text += t->n_inflated;
  r->gz_bytes += t->n_dtext;
}

static void
write_tile (run_t * r, tile_t * t)
{
  emit_tile (r, t);
  /* (with device_gz: the header line, in front of the first tile) */
  if (pgz_write (&r->outfile, r->ob.p, r->ob.n))
    die ("\n pecaller_hip: write to %s.base.gz failed", r->argv[4]);
  r->ob.n = 0;
  if (r->device_gz && t->dtext)
    write_tile_gz (r, t);
  r->tot_cols += t->n;
}

static void *
stage_main (void *arg)
{
  stage_t *c = (stage_t *) arg;
  for (;;)
    {
      pthread_mutex_lock (&c->mu);
      while (!c->has_job && !c->stop)
        pthread_cond_wait (&c->cv, &c->mu);
      if (!c->has_job && c->stop)
        {
          pthread_mutex_unlock (&c->mu);
          return NULL;
        }
      c->has_job = 0;
      c->busy = 1;
      pthread_mutex_unlock (&c->mu);
      struct timespec a, b;
      clock_gettime (CLOCK_MONOTONIC, &a);
      (c->role == 0 ? call_tile : write_tile) (c->r, &c->job);
      clock_gettime (CLOCK_MONOTONIC, &b);
      c->sec += seconds_between (&a, &b);
      if (c->role == 0)
        stage_give (&c->r->row_stage, c->job);
      else
        pool_put (&c->r->pool, c->job);
      pthread_mutex_lock (&c->mu);
      c->busy = 0;
      pthread_cond_broadcast (&c->cv);
      pthread_mutex_unlock (&c->mu);
    }
}

static void
stage_init (stage_t * c, run_t * r, int role)
{
  *c = (stage_t) { .r = r, .role = role };
  pthread_mutex_init (&c->mu, NULL);
  pthread_cond_init (&c->cv, NULL);
}

/* the stage's last tile done and passed on, its thread ended */
static void
stage_stop (stage_t * c)
{
  stage_wait_idle (c);
  pthread_mutex_lock (&c->mu);
  c->stop = 1;
  pthread_cond_broadcast (&c->cv);
  pthread_mutex_unlock (&c->mu);
  pthread_join (c->th, NULL);
}

/* The tiles are handed to the device calls again and again: page-locked once, their columns and results move by DMA straight from and to
   them (a refusal only means staged copies).  The list of posteriors is filled by plain copies: not page-locked, so it can be re-allocated. */
static void
tile_pin (run_t * r, tile_t * t, const void *p, uint64_t bytes)
{
  if (pecall_dev_pin_host (r->pc, p, bytes) == 0)
    t->pinned[t->n_pinned++] = p;
}

static void
tile_alloc (run_t * r, tile_t * t)
{
  const size_t T = r->tile, indiv = (size_t) r->indiv;
  memset (t, 0, sizeof *t);
  if (r->device_guide)
    {
      t->iv_first = (uint32_t *) malloc (T * sizeof (uint32_t));
      t->iv_count = (uint32_t *) malloc (T * sizeof (uint32_t));
      t->iv_chrom = (uint8_t *) malloc (T);
      t->iv_which = (int *) malloc (T * sizeof (int));
      if (!t->iv_first || !t->iv_count || !t->iv_chrom || !t->iv_which)
        die ("\n pecaller_hip: out of memory for %s", "a tile's intervals");
    }
  if (r->device_merge || r->device_guide)
    {
      t->recs = (char *) malloc (indiv * T * 16);
      t->n_recs = (uint64_t *) calloc (indiv, sizeof (uint64_t));
      t->chrom_slot = (uint8_t *) malloc (T);
      t->col_slot = (uint32_t *) malloc (T * sizeof (uint32_t));
      t->vrow = (uint32_t *) malloc (T * sizeof (uint32_t));
      t->vlist = (uint32_t *) malloc (T * sizeof (uint32_t));
      if (!t->recs || !t->n_recs || !t->chrom_slot || !t->col_slot || !t->vrow || !t->vlist)
        die ("\n pecaller_hip: out of memory for %s", "a tile's records");
    }
  t->reads = (uint16_t *) malloc (T * indiv * NA * sizeof (uint16_t));
  t->ref_base = (uint8_t *) malloc (T);
  t->chrom = (uint8_t *) malloc (T);
  t->denovo = (int32_t *) malloc (T * sizeof (int32_t));
  t->ref_char = (char *) malloc (T);
  t->contig = (int *) malloc (T * sizeof (int));
  t->pos = (unsigned int *) malloc (T * sizeof (unsigned int));
  t->call = (int8_t *) malloc (T * indiv);
  t->post_cap = r->post_cap;
  t->post_site = (uint32_t *) malloc (t->post_cap * sizeof (uint32_t));
  t->post_rows = (double *) malloc (t->post_cap * indiv * sizeof (double));
  t->type = (int8_t *) malloc (T);
  t->ac = (int32_t *) malloc (T * NA * sizeof (int32_t));
  if (!t->reads || !t->ref_base || !t->chrom || !t->denovo || !t->ref_char || !t->contig || !t->pos || !t->call || !t->post_site || !t->post_rows || !t->type || !t->ac)
    die ("\n pecaller_hip: out of memory for %s", "a tile");
  /* (device_guide: a range's records are those at guided positions, a few percent of the buffer on an exome; page-locking the whole
     buffer costs more at start-up than the library's staged copy of what is in it) */
  if (r->device_merge)
    tile_pin (r, t, t->recs, (uint64_t) indiv * T * 16);
  if (!r->device_merge)         /* (there the columns' arrays do not travel) */
    {
      tile_pin (r, t, t->reads, (uint64_t) T * indiv * NA * sizeof (uint16_t));
      tile_pin (r, t, t->ref_base, (uint64_t) T);
      tile_pin (r, t, t->chrom, (uint64_t) T);
    }
  if (r->device_rows)
    {
      /* every column a row of the longest form: the longest contig name, ten digits */
      tile_text_alloc (r, t, (uint64_t) T * pcr_row_len ((uint32_t) r->max_name, PCR_MAX_POS, (uint32_t) indiv));
      tile_holes_alloc (t, t->post_cap);
    }
  tile_pin (r, t, t->call, (uint64_t) T * indiv);
  tile_pin (r, t, t->type, (uint64_t) T);
  tile_pin (r, t, t->ac, (uint64_t) T * NA * sizeof (int32_t));
  tile_pin (r, t, t->denovo, (uint64_t) T * sizeof (int32_t));
}

static void
tile_free (run_t * r, tile_t * t)
{
  for (int k = 0; k < t->n_pinned; k++)
    (void) pecall_dev_unpin_host (r->pc, t->pinned[k]);
  if (t->dtext_pinned)
    (void) pecall_dev_unpin_host (r->pc, t->dtext);
  void *rows[] = { t->dtext, t->hole_site, t->hole_len, t->hole_at, t->hole_off, t->hole_pre, (void *) t->hole_src };
  for (size_t k = 0; k < sizeof rows / sizeof rows[0]; k++)
    free (rows[k]);
  void *all[] = { t->iv_first, t->iv_count, t->iv_chrom, t->iv_which, t->recs, t->n_recs, t->chrom_slot, t->col_slot, t->vrow, t->vlist, t->reads, t->ref_base, t->chrom, t->denovo, t->ref_char, t->contig,
    t->pos, t->call, t->post_site, t->post_rows, t->type, t->ac };
  for (size_t k = 0; k < sizeof all / sizeof all[0]; k++)
    free (all[k]);
}

/* the next line of the BED guide file (pecaller.c:1041-1066): contig, first and last position, 1-based -> 0 at its end.  The first
   line is read the reference's way too (pecaller.c:927-940): only a file without any line ends the run quietly there */
static int
next_guide_interval (run_t * r, int first)
{
  r->gline++;
  const ref_t *g = &r->ref;
  char line[4096];
  line[0] = '\0';
  if (!feof (r->guide_file))
    fgets (line, 4095, r->guide_file);
  if (first ? line[0] == '\0' : strlen (line) < 5)
    return 0;
  char *tok = strtok (line, "\t \n");
  r->gwhich = -1;
  for (int i = 0; i < g->no_contigs && tok; i++)
    if (strcmp (tok, g->contig_names[i]) == 0)
      {
        r->gwhich = i;
        break;
      }
  if (r->gwhich < 0 && r->device_guide)
    {
      /* (the range builder reads a line ahead of the walk: the run ends where the walk gets to this line, fill_tile) */
      snprintf (r->gbad_name, sizeof r->gbad_name, "%s", tok ? tok : "");
      r->gbad = 1;
      return 1;
    }
  if (r->gwhich < 0)
    {
      printf ("\n For line chrom %s \n", tok ? tok : "");
      exit (1);
    }
  r->lowest = g->frag_pos[r->gwhich - 1] + (unsigned int) atoi (strtok (NULL, "\t \n")) - 1;
  r->gend = g->frag_pos[r->gwhich - 1] + (unsigned int) atoi (strtok (NULL, "\t \n")) - 1;
  return 1;
}

/* ---- the steps of a run, in the order run_once takes them */
static void
parse_args (run_t * r)
{
  const int argc = r->argc;
  char **argv = r->argv;
  if (argc < 10 || argc > 13)
    {
      printf
        ("\n Usage %s pileup_extension sdx_file no_files outfile Prob_to_call theta haploid[y,n] no_threads use_pedfile[y,n] [pedfilename] [denovo_mutation_rate] [guide_file_bed_format]\n",
         argv[0]);
      exit (1);
    }
  r->no_threads = atoi (argv[8]);
  if (r->no_threads < 2 || r->no_threads > 200)
    {
      printf ("\n Number of threads is limited to 2 to 200.   You entered %d \n\n", r->no_threads);
      exit (1);
    }
  r->threshold = atof (argv[5]);
  r->theta = atof (argv[6]);
  if (r->theta < 1e-10 || r->theta > 0.5)
    {
      printf ("\n Encountered impossible value for theta = %g \n", r->theta);
      exit (1);
    }
  r->use_ped = (strchr (argv[9], 'Y') || strchr (argv[9], 'y')) ? 1 : 0;
  if (r->use_ped)
    {
      if (argc < 12)
        die ("\n pecaller_hip: use_pedfile = %s needs the ped file name and the de-novo mutation rate", argv[9]);
      r->denovo_rate = atof (argv[11]);
      if (r->denovo_rate < 1e-30 || r->denovo_rate > r->theta)
        {
          printf ("\n Encounted impossible denovo mutation rate of %g with a theta of %g", r->denovo_rate, r->theta);
          exit (1);
        }
    }
  if (argc != (r->use_ped ? 12 : 10) && argc != (r->use_ped ? 13 : 11))
    die ("\n pecaller_hip: unexpected number of arguments (last: %s)", argv[argc - 1]);
  if (argc == (r->use_ped ? 13 : 11) && !(r->guide_file = fopen (argv[argc - 1], "r")))
    die ("\n Can not open file %s for writing which should contain the guide_file", argv[argc - 1]);
  r->haploid = (strchr (argv[7], 'Y') || strchr (argv[7], 'y')) ? 1 : 0;
}

static void
open_outputs (run_t * r)
{
  char ss[4096];
  sprintf (ss, "%s.base.gz", r->argv[4]);
  const int pgz_rc = pgz_open (&r->outfile, ss, r->no_threads > 64 ? 64 : r->no_threads);
  /* the rows are ~280 bytes of text per column and 64 samples: at zlib's default level their deflate is the largest single item of the
     run's CPU time (12 of ~30 core-seconds per 8 M columns); level 2 takes half of that for a file 1.4 times the size */
  if (!getenv ("PEMAP_GZ_LEVEL"))
    r->outfile.level = 2;
  if (pgz_rc)
    die ("\n Can not open file %s", ss);
  sprintf (ss, "%s.snp", r->argv[4]);
  if (!(r->snpfile = fopen (ss, "w")))
    die ("\n Can not open file %s for writing", ss);
  sprintf (ss, "%s.dist", r->argv[4]);
  if (!(r->distfile = fopen (ss, "w")))
    die ("\n Can not open file %s for writing", ss);
  sprintf (ss, "%s.piles.gz", r->argv[4]);
  if (!(r->pilefile = gzopen (ss, "w")))
    die ("\n Can not open file %s for writing", ss);
  gzbuffer (r->pilefile, 131072);
}

/* .sdx: contig ends in .seq coordinates (length + 15 each), names, the chrY flag (pecaller.c:447-483); then the reference letters:
   the whole .seq in memory (the reference pages 50 MB windows through gzseek, 1753-1789) */
static void
load_reference (run_t * r)
{
  ref_t *g = &r->ref;
  char ss[4096], sdxname[4096];
  strcpy (sdxname, r->argv[2]);
  FILE *sfile = fopen (sdxname, "r");
  if (!sfile)
    die ("\n Can not open file %s", sdxname);
  if (strstr (sdxname, ".sdx"))
    for (int i = (int) strlen (sdxname) - 1; i > 0; i--)
      if (sdxname[i] == '.')
        {
          sdxname[i] = '\0';
          break;
        }
  if (!fgets (ss, 256, sfile))
    die ("\n Empty file %s", r->argv[2]);
  g->no_contigs = atoi (ss);
  g->start_chrom = (g->no_contigs - 1) / 2 > 0 ? (g->no_contigs - 1) / 2 : 0;
  unsigned int *frag_pos = (unsigned int *) calloc (g->no_contigs + 2, sizeof (unsigned int)) + 1;
  g->frag_pos = frag_pos;
  g->contig_names = (char **) calloc (g->no_contigs + 1, sizeof (char *));
  g->chrom_type = (uint8_t *) calloc (g->no_contigs + 1, 1);
  frag_pos[-1] = 0;
  for (int i = 0; i < g->no_contigs; i++)
    {
      if (!fgets (ss, 1024, sfile))
        die ("\n Short file %s", r->argv[2]);
      char *tok = strtok (ss, "\t \n");
      frag_pos[i] = (unsigned int) atoi (tok) + 15 + frag_pos[i - 1];
      tok = strtok (NULL, "\t \n");
      g->contig_names[i] = strdup (tok);
      char low[1024];
      strcpy (low, tok);
      char *pre = strtok (low, ":_- \n");
      for (char *q = pre; q && *q; q++)
        *q = (char) tolower (*q);
      g->chrom_type[i] = !pre ? 0 : !strcmp (pre, "chrx") ? 1 : !strcmp (pre, "chry") ? 2 : !strcmp (pre, "chrmt") ? 3 : 0;
    }
  fclose (sfile);
  sprintf (ss, "%s.seq", sdxname);
  gzFile reffile = gzopen (ss, "r");
  if (!reffile)
    die ("\n Can not open file %s for reading", ss);
  gzbuffer (reffile, 1 << 22);
  g->gsize = frag_pos[g->no_contigs - 1];
  g->genome = (char *) calloc (g->gsize + 1, 1);
  for (size_t got = 0; got < g->gsize;)
    {
      int n = gzread (reffile, g->genome + got, (unsigned) ((g->gsize - got) > (1u << 30) ? (1u << 30) : (g->gsize - got)));
      if (n <= 0)
        break;
      got += (size_t) n;
    }
  gzclose (reffile);
}

/* the samples: directory order (pecaller.c:486-520) */
static void
open_samples (run_t * r)
{
  char ss[4096];
  int no_files = atoi (r->argv[3]);
  r->sm = (sample_t *) calloc (no_files + 1, sizeof (sample_t));
  DIR *dir = opendir (".");
  if (!dir)
    {
      fprintf (stderr, "%s %d: opendir() failed (%s)\n", __FILE__, __LINE__, strerror (errno));
      exit (-1);
    }
  int found = 0;
  for (struct dirent * de = readdir (dir); de != NULL && found <= no_files; de = readdir (dir))
    if (strstr (de->d_name, r->argv[1]) != NULL)
      {
        if (found == no_files)
          {
            found++;
            break;
          }
        sample_t *s = &r->sm[found];
        strcpy (s->file, de->d_name);      /* (the reader keeps the name for its messages) */
        if (zr_open (&s->f, s->file))
          die ("\n Can not open file %s which should contain pileup information", de->d_name);
        strncpy (ss, de->d_name, sizeof ss - 1);
        char *tok = strtok (ss, "\n.\t ");
        strncpy (s->name, tok ? tok : "", sizeof s->name - 1);
        found++;
      }
  closedir (dir);
  if (found > no_files)
    die ("%s", "\n Found more files than you specified \n");
  r->indiv = found;
  printf ("\n Found a total of %d individuals\n\n", r->indiv);
  if (r->indiv < 1 || r->indiv > MAX_SAMPLES)
    die ("\n pecaller_hip: %s samples; the device caller takes 1 to 512 (64 and fewer are its fast case)", r->argv[3]);
}

/* the ped file: family, individual, father, mother, sex per line (pecaller.c:561-604); parents that are not among the samples are
   ignored; a parent's kids are numbered in the order of the lines */
static void
read_pedigree (run_t * r)
{
  char **argv = r->argv;
  const sample_t *sm = r->sm;
  const int indiv = r->indiv;
  if (!r->use_ped)
    return;
  static int dad[MAX_SAMPLES], mom[MAX_SAMPLES], sex[MAX_SAMPLES], nk[MAX_SAMPLES], kid[MAX_SAMPLES][2 * MAX_SAMPLES], off[MAX_SAMPLES + 1],
    list[2 * MAX_SAMPLES];
  for (int i = 0; i < MAX_SAMPLES; i++)
    {
      dad[i] = mom[i] = -1;
      sex[i] = nk[i] = 0;
    }
  FILE *pedfile = fopen (argv[10], "r");
  if (!pedfile)
    die ("\n Could Not open %s", argv[10]);
  char line[8192];
  while (fgets (line, sizeof line, pedfile) && strlen (line) > 5)
    {
      strtok (line, "\n\t ");
      char *ind = strtok (NULL, "\n\t "), *tf = strtok (NULL, "\n\t "), *tm = strtok (NULL, "\n\t "), *ts = strtok (NULL, "\n\t ");
      if (!ind || !tf || !tm || !ts)
        die ("\n pecaller_hip: short line in %s", argv[10]);
      for (int i = 0; i < indiv; i++)
        if (strcmp (ind, sm[i].name) == 0)
          {
            if (strcmp (tf, "0") != 0)
              for (int j = 0; j < indiv; j++)
                if (strcmp (tf, sm[j].name) == 0)
                  {
                    dad[i] = j;
                    kid[j][nk[j]++] = i;
                    break;
                  }
            if (strcmp (tm, "0") != 0)
              for (int j = 0; j < indiv; j++)
                if (strcmp (tm, sm[j].name) == 0)
                  {
                    mom[i] = j;
                    kid[j][nk[j]++] = i;
                    break;
                  }
            sex[i] = atoi (ts);
          }
    }
  fclose (pedfile);
  off[0] = 0;
  for (int i = 0; i < indiv; i++)
    {
      off[i + 1] = off[i] + nk[i];
      if (off[i + 1] > 2 * MAX_SAMPLES)
        die ("\n pecaller_hip: too many parent-child links in %s", argv[10]);
      for (int k = 0; k < nk[i]; k++)
        list[off[i] + k] = kid[i][k];
    }
  if (pecall_dev_set_pedigree (r->pc, indiv, dad, mom, sex, off, list, r->denovo_rate))
    die ("\n pecaller_hip: %s", pecall_dev_last_error (r->pc));
}

static int
live_streams (const run_t * r)
{
  int n = 0;
  for (int i = 0; i < r->indiv; i++)
    n += r->sm[i].cur != 0;
  return n;
}

/* every stream's first record pending; the header lines of the three row files */
static void
prime_streams (run_t * r)
{
  for (int i = 0; i < r->indiv; i++)
    (void) advance (&r->sm[i]);
  r->running = live_streams (r);
  fprintf (r->snpfile, "Fragment\tPosition\tReference\tAlleles\tAllele_Counts\tType");
  r->ob.n += (size_t) sprintf (sb_room (&r->ob, 64), "Fragment\tPosition\tReference");
  gzprintf (r->pilefile, "Fragment\tPosition\tReference");
  for (int i = 0; i < r->indiv; i++)
    {
      fprintf (r->snpfile, "\t%s\t", r->sm[i].name);
      r->ob.n += (size_t) sprintf (sb_room (&r->ob, strlen (r->sm[i].name) + 8), "\t%s\t", r->sm[i].name);
      gzprintf (r->pilefile, "\t%s\t\t\t\t\t", r->sm[i].name);
    }
}

/* the sizes the environment may set, the three tiles, the merge's threads and planes, the two stages */
static void
start_pipeline (run_t * r)
{
  const char *e = getenv ("PECALLER_TILE_LOG2");
  r->tile = (size_t) 1 << 20;
  if (e && atoi (e) >= 10 && atoi (e) <= 22)
    r->tile = (size_t) 1 << atoi (e);
  else
    {
      /* the host arrays hold ~54 bytes per (column, sample) -- the merge's planes, three tiles of reads and calls, the lists of the
         posteriors that are not 1: 2^20 columns are 3.6 GB with 64 samples; with more samples the tile shrinks so that columns x samples stays at that product */
      while (r->tile > ((size_t) 1 << 16) && r->tile * (size_t) r->indiv > ((size_t) 1 << 26))
        r->tile >>= 1;
    }
  r->mg_chunk = r->tile < 65536 ? r->tile : 65536;
  r->guide_range_min = 4096;
  if ((e = getenv ("PECALLER_GUIDE_RANGE_MIN")) && atol (e) >= 1)
    r->guide_range_min = (unsigned long long) atol (e);
  /* (tests: a list that is too short for the first tiles, so that the second call with the size asked for is taken) */
  r->post_cap = r->tile / 8 > 1024 ? r->tile / 8 : 1024;
  if ((e = getenv ("PECALLER_POST_CAP")) && atol (e) >= 1)
    r->post_cap = (uint64_t) atol (e);
  r->device_merge = !r->guide_file && !r->serial_merge && (e = getenv ("PECALLER_DEVICE_MERGE")) && atoi (e) == 1;
  r->device_guide = r->guide_file && !r->serial_merge && (e = getenv ("PECALLER_DEVICE_GUIDE")) && atoi (e) == 1;
  if (r->device_guide && !pecall_dev_call_records_guided)
    die ("\n pecaller_hip: PECALLER_DEVICE_GUIDE=1 needs %s, which this library lacks", "pecall_dev_call_records_guided");
  r->device_rows = (e = getenv ("PECALLER_DEVICE_ROWS")) && atoi (e) == 1;
  if (r->device_rows && !pecall_dev_sites_base_text)
    die ("\n pecaller_hip: PECALLER_DEVICE_ROWS=1 needs %s, which this library lacks", "pecall_dev_sites_base_text");
  r->device_gz = (e = getenv ("PECALLER_DEVICE_GZ")) && atoi (e) == 1;
  if (r->device_gz && !r->device_rows)
    die ("\n pecaller_hip: PECALLER_DEVICE_GZ=1 needs %s", "PECALLER_DEVICE_ROWS=1: it deflates the rows the device made");
  if (r->device_gz && !pecall_dev_sites_base_gz)
    die ("\n pecaller_hip: PECALLER_DEVICE_GZ=1 needs %s, which this library lacks", "pecall_dev_sites_base_gz");
  if (r->device_rows)
    {
      const ref_t *g = &r->ref;
      size_t bytes = 0;
      for (int i = 0; i < g->no_contigs; i++)
        bytes += strlen (g->contig_names[i]);
      r->names = (char *) malloc (bytes + 1);
      r->name_off = (uint32_t *) calloc ((size_t) g->no_contigs + 1, sizeof (uint32_t));
      if (!r->names || !r->name_off)
        die ("\n pecaller_hip: out of memory for %s", "the contig names");
      for (int i = 0; i < g->no_contigs; i++)
        {
          const size_t l = strlen (g->contig_names[i]);
          memcpy (r->names + r->name_off[i], g->contig_names[i], l);
          r->name_off[i + 1] = r->name_off[i] + (uint32_t) l;
          if (l > r->max_name)
            r->max_name = l;
        }
    }
  pthread_mutex_init (&r->pool.mu, NULL);
  pthread_cond_init (&r->pool.cv, NULL);
  for (int k = 0; k < N_TILES; k++)
    tile_alloc (r, &r->pool.free_tile[r->pool.n_free++]);
  /* the threads of the merge and of the row formatting: the reference's worker threads minus its dispatcher, as many as the host has CPUs and the run has streams, at most 128 */
  const long ncpu = sysconf (_SC_NPROCESSORS_ONLN);
  r->MT = r->no_threads - 1;
  if (ncpu > 0 && r->MT > (int) ncpu)
    r->MT = (int) ncpu;
  r->MT = r->MT > MAX_MT ? MAX_MT : r->MT;
  r->MT = r->MT > r->indiv ? r->indiv : r->MT < 1 ? 1 : r->MT;
  r->chunk_base = (long *) calloc (r->tile / r->mg_chunk, sizeof (long));
  /* (with a guide file too: its long intervals go through the same merge) */
  if (!r->device_merge)
    {
      r->planes = (uint16_t *) malloc ((size_t) r->indiv * r->tile * NA * sizeof (uint16_t));
      r->marks = (uint8_t *) malloc ((size_t) r->MT * r->tile);
      if (!r->planes || !r->marks)
        die ("\n pecaller_hip: out of memory for %s", "the merge planes");
    }
  stage_init (&r->dev_stage, r, 0);
  stage_init (&r->row_stage, r, 1);
  if (pthread_create (&r->row_stage.th, NULL, stage_main, &r->row_stage) || pthread_create (&r->dev_stage.th, NULL, stage_main, &r->dev_stage))
    die ("\n pecaller_hip: can not start %s", "the device and the text threads");
}

/* ---- the four ways a tile is filled (run, tile -> 1 when the tile is to be handed over whatever it holds) */
static unsigned int
lowest_pending (const run_t * r)        /* find_lowest, pecaller.c:1820-1833 */
{
  unsigned int lowest = 0;
  for (int i = 0; i < r->indiv; i++)
    if (r->sm[i].cur > 0 && (lowest == 0 || r->sm[i].cur < lowest))
      lowest = r->sm[i].cur;
  return lowest;
}

/* One column at position `lowest`: the streams that have a record there, zeros for the others; a stream's records are taken in the
   order they come.  which >= 0: a position of a guide interval on that contig (pecaller.c:941-1039) -- the streams behind it are
   advanced first, a sample without a record has seen the position too, and chrY / chrMT are flagged */
static void
column_at (run_t * r, tile_t * t, unsigned int lowest, int which)
{
  const int guide = which >= 0;
  const long col = t->n++;
  column_header (&r->ref, t, col, lowest, which);
  t->chrom[col] = chrom_class (&r->ref, t->contig[col], guide);
  r->tot_bases++;
  uint16_t *dst = t->reads + (size_t) col * r->indiv * NA;
  for (int i = 0; i < r->indiv; i++)
    {
      sample_t *s = &r->sm[i];
      while (guide && s->cur < lowest && s->cur > 0)
        r->running -= advance (s);
      if (s->cur == lowest)
        {
          unsigned int cov = 0;
          for (int a = 0; a < NA; a++)
            {
              dst[i * NA + a] = s->data[a];
              cov += s->data[a];
            }
          s->mean += (double) cov;
          if (cov > s->max_coverage)
            s->max_coverage = cov;
          s->counts[cov < MAX_DIST - 1 ? cov : MAX_DIST - 1]++;
          s->base_count++;
          r->running -= advance (s);
        }
      else
        {
          memset (dst + i * NA, 0, NA * sizeof (uint16_t));
          s->base_count += (unsigned int) guide;
        }
    }
}

/* one column, the reference's way (pecaller.c:865-923): the lowest pending position of all streams */
static int
fill_serial_column (run_t * r, tile_t * t)
{
  column_at (r, t, lowest_pending (r), -1);
  return 0;
}

static void
set_range (run_t * r, tile_t * t, unsigned int p0, unsigned long long p1, int gwhich)
{
  for (int k = 0; k < r->MT; k++)
    r->mc[k] = (merge_ctx) { r, t, k, p0, p1, gwhich >= 0, gwhich, t->n, -1 };
}

/* the run is abandoned: what is in flight is finished and closed, run_once returns RC_UNORDERED */
static int
abandon (run_t * r, tile_t * t)
{
  r->running = 0;
  t->n = 0;
  return 0;
}

/* device merge: the chromosome classes of the range's positions, a stretch between two contig boundaries at a time -- find_chrom's
   answer changes at a contig's last position and the one behind it only */
static void
chrom_classes (const ref_t * g, tile_t * t, unsigned int p0, size_t tile)
{
  unsigned long long q = p0;
  const unsigned long long end = (unsigned long long) p0 + tile;
  while (q < end)
    {
      const int which = find_chrom (g->frag_pos, 0, g->no_contigs - 1, g->start_chrom, (unsigned int) (q > 0xffffffffull ? 0xffffffffull : q));
      unsigned long long stop = end;
      for (int w = which - 2; w <= which + 1; w++)
        if (w >= -1 && w < g->no_contigs)
          for (unsigned long long b = g->frag_pos[w]; b <= (unsigned long long) g->frag_pos[w] + 1; b++)
            if (b > q && b < stop)
              stop = b;
      memset (t->chrom_slot + (q - p0), g->chrom_type[which], (size_t) (stop - q));
      q = stop;
    }
}

/* the next range of positions, from the lowest pending position of all streams: a tile of its own */
static int
fill_range (run_t * r, tile_t * t)
{
  const unsigned int p0 = lowest_pending (r);
  set_range (r, t, p0, (unsigned long long) p0 + r->tile, -1);
  if (!r->unordered)            /* (set already: the library's word on an earlier range, device merge) */
    run_threads (r->device_merge ? merge_streams_dev : merge_streams, r);
  if (r->unordered)
    return abandon (r, t);
  if (r->device_merge)
    {
      chrom_classes (&r->ref, t, p0, r->tile);
      t->p0 = p0;
      t->from_records = 1;
      t->n = 0;                 /* (known when the device has made the columns: the device thread counts them) */
    }
  else
    walked_columns (r, t);
  r->running = live_streams (r);
  return 1;
}

/* a long stretch of the guide interval: every stream is walked over it on its own, as without a guide file (the per-column scan of
   all streams in fill_guide_position costs 1.4 us a column) */
static int
fill_guide_stretch (run_t * r, tile_t * t)
{
  unsigned long long n = (unsigned long long) r->gend + 1 - r->lowest;
  if (n > r->tile - (size_t) t->n)
    n = r->tile - (size_t) t->n;
  set_range (r, t, r->lowest, (unsigned long long) r->lowest + n, r->gwhich);
  run_threads (merge_streams, r);
  if (r->unordered)
    return abandon (r, t);
  /* The reference's loop runs while a stream is open (pecaller.c:952): the column at which the last stream ends is the last one.
     The walk above went over the whole stretch: cut it there, and take the positions behind the cut out of every stream's
     count of positions seen again. */
  if (live_streams (r) == 0)
    {
      long last = 0;
      for (int k = 0; k < r->MT; k++)
        if (r->mc[k].end_slot > last)
          last = r->mc[k].end_slot;
      const unsigned long long keep = (unsigned long long) last + 1;
      if (keep < n)
        {
          memset (r->marks + keep, 0, (size_t) (n - keep));
          for (int i = 0; i < r->indiv; i++)
            r->sm[i].base_count -= (unsigned int) (n - keep);
          n = keep;
        }
      r->running = 0;
    }
  walked_columns (r, t);
  r->lowest += (unsigned int) n;
  if (r->running > 0 && r->lowest > r->gend && !next_guide_interval (r, 0))
    r->running = 0;
  return 0;
}

/* one position of the guide interval (pecaller.c:941-1039) */
static int
fill_guide_position (run_t * r, tile_t * t)
{
  column_at (r, t, r->lowest, r->gwhich);
  r->lowest++;
  if (r->lowest > r->gend && !next_guide_interval (r, 0))
    r->running = 0;
  return 0;
}

/* PECALLER_DEVICE_GUIDE=1: can the range builder take the BED line at hand, from r->lowest on?  Not a line whose end lies in front of
   its start (the reference still calls the start position), nor one that leaves the genome or begins at position 0 of the .seq (an
   exhausted stream's pending position is 0 too): such a line goes through the per-position path as without the switch. */
static int
guide_line_fits (const run_t * r)
{
  return r->lowest >= 1 && r->lowest <= r->gend && (size_t) r->gend < r->ref.gsize && r->lowest >= r->ref.frag_pos[r->gwhich - 1];
}

/* PECALLER_DEVICE_GUIDE=1: a range of guide intervals, a tile of its own.  The range is a maximal run of consecutive BED lines that
   ascend, are disjoint and fit from the first guided position on into r->tile positions; a longer line is cut there and goes on in
   the next range; a line that goes backwards or overlaps begins a new one; a line guide_line_fits refuses ends the range and is left
   to the per-position path.  The streams are walked from the first to the last guided position (walk_streams, to_records = 2), the
   columns are made and called on the device (pecall_dev_call_records_guided, the device thread).
   The reference's loop runs while a stream is open (pecaller.c:952): the column at which the last stream ends is the run's last.  If
   that happened in this range the intervals are cut behind that column; no record lies behind it. */
static int
fill_guide_range (run_t * r, tile_t * t)
{
  if (t->n > 0)
    return 1;                   /* (columns of the per-position path: that tile goes first) */
  const unsigned int p0 = r->lowest;
  unsigned long long end = p0;  /* the range so far: [p0, end) */
  uint32_t n_iv = 0;
  for (;;)
    {
      const unsigned long long first = (unsigned long long) r->lowest - p0;
      if (first >= r->tile)
        break;
      unsigned long long cnt = (unsigned long long) r->gend + 1 - r->lowest;
      if (first + cnt > r->tile)
        cnt = r->tile - first;
      t->iv_first[n_iv] = (uint32_t) first;
      t->iv_count[n_iv] = (uint32_t) cnt;
      t->iv_chrom[n_iv] = chrom_class (&r->ref, r->gwhich, 1);
      t->iv_which[n_iv++] = r->gwhich;
      end = (unsigned long long) p0 + first + cnt;
      if (r->gline_taken != r->gline)
        {
          r->gline_taken = r->gline;
          r->dg_ivs++;
        }
      if ((unsigned long long) r->lowest + cnt <= r->gend)
        {
          r->lowest += (unsigned int) cnt;      /* (cut at the span: the line goes on in the next range) */
          break;
        }
      if (!next_guide_interval (r, 0))
        {
          r->guide_done = 1;
          break;
        }
      r->gline_judged = r->gline;
      r->gline_host = r->gbad || !guide_line_fits (r);
      if (r->gline_host || (unsigned long long) r->lowest < end)
        break;
    }
  t->n_iv = n_iv;
  t->p0 = p0;
  t->span = (uint32_t) (end - p0);
  t->from_records = 1;
  t->n = 0;                     /* (known when the device has made the columns: the device thread counts them) */
  set_range (r, t, p0, end, t->iv_which[0]);
  run_threads (merge_streams_guided, r);
  if (r->unordered)
    {
      t->n_iv = 0;
      return abandon (r, t);
    }
  r->running = live_streams (r);
  if (r->running == 0)
    {
      long last = 0;
      for (int k = 0; k < r->MT; k++)
        if (r->mc[k].end_slot > last)
          last = r->mc[k].end_slot;
      while (t->n_iv > 1 && t->iv_first[t->n_iv - 1] > (uint32_t) last)
        t->n_iv--;
      t->iv_count[t->n_iv - 1] = (uint32_t) last + 1 - t->iv_first[t->n_iv - 1];
      t->span = (uint32_t) last + 1;
    }
  unsigned int ncols = 0;
  for (uint32_t k = 0; k < t->n_iv; k++)
    ncols += t->iv_count[k];
  /* every sample has seen every column, its stream open or not (pecaller.c:1005, 1028) */
  for (int i = 0; i < r->indiv; i++)
    r->sm[i].base_count += ncols;
  r->tot_bases += ncols;
  if (r->guide_done)
    r->running = 0;
  return 1;
}

static int
fill_tile (run_t * r, tile_t * t)
{
  if (!r->guide_file)
    return (r->serial_merge ? fill_serial_column : fill_range) (r, t);
  if (r->device_guide)
    {
      if (r->gline_judged != r->gline)
        {
          r->gline_judged = r->gline;
          r->gline_host = r->gbad || !guide_line_fits (r);
        }
      if (r->gbad)
        {
          if (t->n > 0)
            return 1;           /* (what is in the tile is written first, as the reference's workers would have) */
          stage_wait_idle (&r->dev_stage);
          stage_wait_idle (&r->row_stage);
          printf ("\n For line chrom %s \n", r->gbad_name);
          exit (1);
        }
      if (!r->gline_host)
        return fill_guide_range (r, t);
    }
  /* (with the serial merge every guide position goes through the per-column scan, which is the reference's) */
  /* (a line whose end lies in front of its start is one position, the start, as in the reference: never a stretch) */
  if (!r->serial_merge && r->gend >= r->lowest && (unsigned long long) r->gend + 1 - r->lowest >= r->guide_range_min && (size_t) t->n < r->tile)
    return fill_guide_stretch (r, t);
  return fill_guide_position (r, t);
}

/* tiles are filled and handed to the device stage until the streams (or the guide file) end; then both stages finish what they hold */
static void
walk (run_t * r)
{
  struct timespec tc0, tc1;
  tile_t t = pool_get (&r->pool);
  clock_gettime (CLOCK_MONOTONIC, &tc0);
  if (r->guide_file && !next_guide_interval (r, 1))
    r->running = 0;
  while (r->running > 0 || t.n > 0)
    {
      const int full = r->running > 0 ? fill_tile (r, &t) : 0;
      if (full || (size_t) t.n == r->tile || (r->running <= 0 && t.n > 0))
        {
          clock_gettime (CLOCK_MONOTONIC, &tc1);
          r->sec_merge += seconds_between (&tc0, &tc1);
          stage_give (&r->dev_stage, t);        /* (and on with a free set of arrays) */
          t = pool_get (&r->pool);
          clock_gettime (CLOCK_MONOTONIC, &tc0);
          r->sec_wait += seconds_between (&tc1, &tc0);
        }
    }
  pool_put (&r->pool, t);
  stage_stop (&r->dev_stage);   /* (the device thread has passed its last tile on before it is idle) */
  stage_stop (&r->row_stage);
  r->tot_bases += (unsigned int) r->dev_cols;
}

/* <outfile>.dist, pecaller.c:1077-1140: text from the samples' statistics and the number of columns */
static void
write_dist (run_t * r)
{
  sample_t *sm = r->sm;
  const int no_files = r->indiv;
  const unsigned int tot_bases = r->tot_bases;
  FILE *distfile = r->distfile;
  unsigned int *tot_1x = (unsigned int *) calloc (no_files, sizeof (unsigned int)), *tot_8x = (unsigned int *) calloc (no_files, sizeof (unsigned int));
  int *median = (int *) calloc (no_files, sizeof (int));
  for (int i = 0; i < no_files; i++)
    {
      if (sm[i].base_count > 0)
        sm[i].mean /= (double) sm[i].base_count;
      for (int j = 8; j < MAX_DIST; j++)
        tot_8x[i] += sm[i].counts[j];
      tot_1x[i] = tot_8x[i];
      for (int j = 1; j < 8; j++)
        tot_1x[i] += sm[i].counts[j];
      sm[i].counts[0] = tot_bases - tot_1x[i];
      long median_count = sm[i].counts[0];
      const long stop = tot_bases / 2;
      for (int j = 1; j < MAX_DIST; j++)
        {
          if (median_count > stop)
            break;
          median_count += sm[i].counts[++median[i]];
        }
    }
  fprintf (distfile, "Category");
  for (int i = 0; i < no_files; i++)
    fprintf (distfile, "\t%s", sm[i].name);
  fprintf (distfile, "\nTotal Number of bases in target");
  for (int i = 0; i < no_files; i++)
    fprintf (distfile, "\t%u", tot_bases);
  fprintf (distfile, "\nTotal Number of bases with at least 1x coverage");
  for (int i = 0; i < no_files; i++)
    fprintf (distfile, "\t%u", tot_1x[i]);
  fprintf (distfile, "\nTotal Number of bases with at least 8x coverage");
  for (int i = 0; i < no_files; i++)
    fprintf (distfile, "\t%u", tot_8x[i]);
  fprintf (distfile, "\nMean depth of coverage");
  for (int i = 0; i < no_files; i++)
    fprintf (distfile, "\t%g", sm[i].mean);
  fprintf (distfile, "\nMedian depth of coverage");
  for (int i = 0; i < no_files; i++)
    fprintf (distfile, "\t%d", median[i]);
  fprintf (distfile, "\nMaximum depth of coverage");
  for (int i = 0; i < no_files; i++)
    fprintf (distfile, "\t%d", (int) sm[i].max_coverage);
  fprintf (distfile, "\n\nDepth");
  for (int j = 0; j < MAX_DIST - 1; j++)
    {
      fprintf (distfile, "\n%d", j);
      for (int i = 0; i < no_files; i++)
        fprintf (distfile, "\t%u", sm[i].counts[j]);
    }
  fprintf (distfile, "\n%d+", MAX_DIST - 1);
  for (int i = 0; i < no_files; i++)
    fprintf (distfile, "\t%u", sm[i].counts[MAX_DIST - 1]);
  fprintf (distfile, "\n");
  fclose (distfile);
  free (tot_1x);
  free (tot_8x);
  free (median);
}

static void
close_outputs (run_t * r)
{
  fclose (r->snpfile);
  if (r->ob.n && pgz_write (&r->outfile, r->ob.p, r->ob.n))     /* (the header line, when there was no column at all) */
    die ("\n pecaller_hip: write to %s.base.gz failed", r->argv[4]);
  if (pgz_close (&r->outfile))
    die ("\n pecaller_hip: closing %s.base.gz failed", r->argv[4]);
  gzclose (r->pilefile);
  struct timespec now;
  clock_gettime (CLOCK_MONOTONIC, &now);
  const double sec = seconds_between (&r->tstart, &now);
  printf ("\n pecaller_hip: %ld columns x %d samples merged, called and written in %.3f s (%.3f M columns/s; stream merge %.3f s + %.3f s waiting for the other thread: device calls %.3f s, rows and gz %.3f s) \n",
          r->tot_cols, r->indiv, sec, (double) r->tot_cols / (sec > 0 ? sec : 1) / 1e6, r->sec_merge, r->sec_wait, r->dev_stage.sec, r->row_stage.sec);
  if (r->device_merge && !r->unordered)
    printf (" pecaller_hip: device merge: %ld columns in %ld ranges\n", r->dev_cols, r->dev_ranges);
  if (r->device_guide && !r->unordered)
    printf (" pecaller_hip: device guide merge: %ld columns of %ld intervals in %ld ranges\n", r->dg_cols, r->dg_ivs, r->dg_ranges);
  if (r->device_rows && !r->unordered)
    printf (" pecaller_hip: device rows: %ld rows from the device, %ld holes formatted by the host\n", r->rows_dev, r->rows_hole);
  if (r->device_gz && !r->unordered)
    printf (" pecaller_hip: device gz: %llu bytes of text deflated on the device into %llu bytes of gz\n", r->gz_text, r->gz_bytes);
}

/* everything the run holds is given back (the stages' threads ended in walk); page-locked ranges before their memory and the device */
static void
teardown (run_t * r)
{
  ref_t *g = &r->ref;
  for (int i = 0; i < r->indiv; i++)
    zr_close (&r->sm[i].f);
  for (int k = 0; k < r->pool.n_free; k++)
    tile_free (r, &r->pool.free_tile[k]);
  free (r->planes);
  free (r->marks);
  free (r->chunk_base);
  for (int k = 0; k < MAX_MT; k++)
    free (r->jobs[k].ob.p), free (r->jobs[k].sb.p), free (r->jobs[k].pb.p);
  free (r->ob.p);
  free (r->gzb.p);
  free (r->names);
  free (r->name_off);
  free (r->sm);
  for (int i = 0; i < g->no_contigs; i++)
    free (g->contig_names[i]);
  free (g->contig_names);
  free ((void *) (g->frag_pos - 1));
  free (g->chrom_type);
  free (g->genome);
  pecall_dev_destroy (r->pc);
  if (r->guide_file)
    fclose (r->guide_file);
  free (r);
}

/* One pass over the inputs, by the parallel walk of the streams or (serial_merge) the reference's way.  RC_UNORDERED: the parallel walk
   met a record out of order (what has been written by then is written over by the repeat, which starts from nothing: main) */
static int
run_once (int argc, char *argv[], int serial_merge)
{
  run_t *r = (run_t *) calloc (1, sizeof (run_t));
  if (!r)
    die ("\n pecaller_hip: out of memory for %s", "the run");
  r->argc = argc;
  r->argv = argv;
  r->serial_merge = serial_merge;
  parse_args (r);
  open_outputs (r);
  load_reference (r);
  open_samples (r);
  if (pecall_dev_create (&r->pc, getenv ("PEMAP_DEVICE") ? atoi (getenv ("PEMAP_DEVICE")) : 0))
    die ("\n pecaller_hip: %s", pecall_dev_last_error (NULL));
  read_pedigree (r);
  prime_streams (r);
  clock_gettime (CLOCK_MONOTONIC, &r->tstart);
  start_pipeline (r);
  walk (r);
  write_dist (r);
  close_outputs (r);
  const int rc = r->unordered ? RC_UNORDERED : 0;
  teardown (r);
  return rc;
}

int
main (int argc, char *argv[])
{
  /* PECALLER_SERIAL_MERGE=1: the serial merge from the start (pileup files known to be out of order) */
  const char *e = getenv ("PECALLER_SERIAL_MERGE");
  int rc = run_once (argc, argv, e && atoi (e));
  if (rc == RC_UNORDERED)
    {
      printf ("\n pecaller_hip: a pileup stream is not in ascending order: starting over with the serial merge (the reference's dispatcher) \n");
      fflush (stdout);
      rc = run_once (argc, argv, 1);
    }
  return rc;
}
