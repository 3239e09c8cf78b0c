// pemap_capi.hip -- the C-ABI of include/pemap_hip.h on top of the gfx950 kernels.
//
// Built as libpemap_hip.so:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared ...
// There is no CPU fallback in this library: every entry either runs on the GPU or returns an error.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <unistd.h>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>
#include "../../include/pemap_hip.h"
#include "pemap_kernels.hip.h"
#include "pemap_aux.hip.h"
#include "pemap_fastq.hip.h"
#include "pemap_gz.hip.h"
#include <rocprim/rocprim.hpp>

static char g_create_err[512] = "";

// ---- batches in flight (pemap_dev_submit_batch / pemap_dev_wait_batch).  The staged-read arrays of the object are cut in
// PM_RING slots of PmRing::cap rows; a submitted batch owns one slot from its host-to-device copy to the device-to-host copy of
// its m1 / m2 / mapping_type.  Lengths and results pass through pinned staging buffers of the slot; the read rows are copied
// straight from the caller's buffers where the caller pinned them (pemap_dev_pin_host).
#define PM_RING 3
struct PmRingSlot
{
  bool active = false;
  unsigned long long seq = 0;   // ticket of the batch that owns the slot
  int n = 0, first = 0;
  uint32_t *m1 = nullptr, *m2 = nullptr;        // the caller's result buffers
  int *mt = nullptr;
  int *h_len = nullptr;         // pinned: len1 | len2
  uint32_t *h_res = nullptr;    // pinned: m1 | m2 | mapping_type
  char *h_rows = nullptr;       // pinned staging for read rows submitted from pageable memory: reads1 | reads2 (allocated on first need)
  size_t h_rows_bytes = 0;
  hipEvent_t ev_done = nullptr; // recorded behind the device-to-host copy of the results
  std::vector < hipEvent_t > ev_copy;   // one per slice: the slice's rows are on the device
};

// ---- chunks in flight.  The pipeline keeps PM_SETS chunks in flight (the seed stage of chunk k+1 beside the SW / walk of chunk k),
// so everything a chunk works on exists PM_SETS times: chunk g of a run, counted over the runs queued behind each other, uses set
// g % PM_SETS.  All sets have the same sizes (the capacities are PmChunkWork's) and are allocated and released together.
#define PM_SETS 2
// A third set is this constant plus what the constant does not say: the waits of enqueue_seed on ev_lists_free / ev_walk_done are
// written for "the chunk PM_SETS back" but were only ever run with two sets, the seed stage would run three chunks ahead of the ALU
// stream (run_slice), and at the seam a third batch has to be in flight for a third chunk to exist.
static_assert (PM_SETS == 2, "the wait rules of enqueue_seed and the look-ahead of run_slice are only validated for two sets");
struct PmChunkSet
{
  PmHits hits = {};
  uint32_t *wins = nullptr, *dirbuf = nullptr;
  uint32_t *walks = nullptr;    // places in `wins` of the alignments pm_walk_kernel follows
  uint32_t *tasks_s = nullptr, *tasks_m = nullptr;      // SW problems of the single-hit / multi-hit ends, PM_TASK_QUARTERS quarters each (task_list)
  unsigned long long *path = nullptr;   // recorded traceback steps per winning alignment
  uint16_t *nsteps = nullptr;
  PmLists lists = {};
  hipEvent_t ev_lists_ready = nullptr, ev_lists_free = nullptr, ev_walk_done = nullptr;
  uint64_t rest_id = 0;         // run serial and chunk number of the last remainder enqueued on the set (launch_rest)
};

// The timing events of a chunk (PmRun::evs holds PM_NEV per chunk), each recorded behind the kernel(s) it is named for, and the
// times pemap_dev_run_stats reports (in the order of include/pemap_hip.h), each the sum over pm_intervals' rows for its slot.
enum PmEvent
{
  PM_EV_LOOKUP_BEGIN, PM_EV_LOOKUP_END, PM_EV_VOTE_BEGIN, PM_EV_VOTE_END, PM_EV_SEED_END,       // the seed stage, on either stream
  PM_EV_SW_SINGLE_END, PM_EV_SW_MULTI_END, PM_EV_SELECT_END, PM_EV_SW_REDO_END, PM_EV_WALK_END, PM_NEV       // the ALU stream
};
enum PmTime { PM_T_SEED, PM_T_SW_SINGLE, PM_T_SW_MULTI, PM_T_SELECT, PM_T_SW_REDO, PM_T_WALK, PM_T_LOOKUP, PM_T_VOTE, PM_NT };
static_assert (PM_NT == 8, "pemap_dev_run_stats copies last_ms into the caller's times_ms8");
// the slots of pemap_dev_pipeline_stats (include/pemap_hip.h): runs queued; of them, runs that continued a pending pipeline; absorbs because
// the chunk table was full / the longest read changed / the pending runs' arrays are too small; ring set-ups; the last run's chunks; its first
enum PmPipeStat
{
  PM_PS_RUNS, PM_PS_CONTINUED, PM_PS_ABSORB_TABLE_FULL, PM_PS_ABSORB_LENGTH, PM_PS_ABSORB_ARRAYS, PM_PS_RING_SETUPS, PM_PS_LAST_CHUNKS,
  PM_PS_LAST_FIRST_CHUNK, PM_NPS
};
static_assert (PM_NPS == 8, "pemap_dev_pipeline_stats copies pstat into the caller's out8");
static const struct { PmTime slot; PmEvent from, to; bool seed_too; } pm_intervals[] = {
  // the seed stage in two rows: its look-ups (one measurement for two slots), then vote, remainder and emit (the reference layout's run on the ALU stream)
  { PM_T_LOOKUP, PM_EV_LOOKUP_BEGIN, PM_EV_LOOKUP_END, true }, { PM_T_SEED, PM_EV_VOTE_BEGIN, PM_EV_SEED_END },
  { PM_T_VOTE, PM_EV_VOTE_BEGIN, PM_EV_VOTE_END }, { PM_T_SW_SINGLE, PM_EV_SEED_END, PM_EV_SW_SINGLE_END },
  { PM_T_SW_MULTI, PM_EV_SW_SINGLE_END, PM_EV_SW_MULTI_END }, { PM_T_SELECT, PM_EV_SW_MULTI_END, PM_EV_SELECT_END },
  { PM_T_SW_REDO, PM_EV_SELECT_END, PM_EV_SW_REDO_END }, { PM_T_WALK, PM_EV_SW_REDO_END, PM_EV_WALK_END },
};

// per-chunk device counters: the kernels' PmCounters plus what the look-up kernel counts
struct PmChunkCtr
{
  PmCounters c;
  unsigned long long positions;
  unsigned n_big;
  unsigned next_end;            // work counter of the persistent look-up waves
  unsigned n_big2;              // read-ends the second tier of the fused seed kernel leaves to pm_seed_kernel
  unsigned next_end2;           // the second tier's work counter
  unsigned long long t_lookup_begin, t_lookup_end;      // the fused first tier's own stamps (wall_clock64; 0: the launch took none)
};

#define PM_MAX_CHUNKS 256

// Host ranges page-locked through pemap_dev_pin_host.  HIP's registrations are process-wide and keyed by the pointer, so the
// table is too (one object must not undo what another still copies from); a range stays until its last unpin.  The library
// never registers memory on its own: a registration outlives the buffer it was made for, and any later copy of the process
// that touches part of such a stale range is refused by the runtime (a copy must lie inside ONE registration or outside all:
// tools/micro/hostreg.hip).  Rows submitted from memory that is not pinned go through the slot's own pinned staging buffer.
struct PmPinned
{
  char *base;
  size_t bytes;
  int users;                    // pemap_dev_pin_host calls not yet undone
};
static std::mutex g_pin_mu;
static std::vector < PmPinned > g_pinned;

// Tuning knobs.  The environment is read ONCE, by pemap_dev_create, into the object: nothing below
// calls getenv again, so two objects of one process may run with different settings and a setting cannot change under a
// run.  None is needed in normal use.
struct PmKnobs
{
  int big_blocks_per_cu, sw_waves_per_cu;
  int replicas;                 // -1 unset, 0 never, 1 as the default
  int gapless;                  // 0 off, 1 first case only, 2 the first two, 3 all three
  double dir_budget_gb;
  int lookup_waves /* -1 unset */;
  int lookup_prio, vote_prio, sw_prio;
  int vote_waves;
  int walk_blocks_per_cu, pile_blocks_per_cu;
  int pipeline;                 // 1 the seed stage on a stream of its own, two chunks ahead; 2 everything on the ALU stream
  int chunk_pairs;
  int gapless_blocks_per_cu;
  int band, band_waves_per_cu;  // the banded DP (pm_band_kernel) for the problems it is exact for; its waves per CU
  int band_gate;                // one-gap reads reach the band by the two-diagonal bound (PM_BAND_MAXX_, pemap_sw.hip.h): 1 always, 0 never
                                // (by x <= 6 alone), -1 (unset) in chunks that hold more read-ends than one pass of the full DP's grid
  int first_tier;               // 0 (tests): every end of a chunk goes to the second tier's list, the first tier is not launched
  int tier2_waves;              // persistent waves per CU of the fused seed kernel's second tier (the first tier's big-end list)
  int absorb_staged;            // pemap_dev_absorb: 1 = through the staging buffers even when both objects sit on one device
  size_t absorb_chunk;          // bytes of a staging piece (PEMAP_ABSORB_CHUNK is in KiB): a multiple of 256, at least 256
};

static int env_int (const char *name, int dflt)
{
  const char *e = getenv (name);
  return (e && *e) ? atoi (e) : dflt;
}

static void read_knobs (PmKnobs & k)
{
  k.big_blocks_per_cu = env_int ("PEMAP_BIG_BLOCKS_PER_CU", 8);
  k.sw_waves_per_cu = env_int ("PEMAP_SW_WAVES_PER_CU", 16);
  // a grid of zero or fewer blocks is not a setting
  if (k.big_blocks_per_cu < 1) k.big_blocks_per_cu = 1;
  if (k.sw_waves_per_cu < 1) k.sw_waves_per_cu = 1;
  k.replicas = getenv ("PEMAP_REPLICAS") ? (env_int ("PEMAP_REPLICAS", 1) ? 1 : 0) : -1;
  k.gapless = env_int ("PEMAP_GAPLESS", 3);
  { const char *e = getenv ("PEMAP_DIR_BUDGET_GB"); k.dir_budget_gb = e ? atof (e) : 40.0; if (k.dir_budget_gb < 0.25) k.dir_budget_gb = 0.25; }
  k.lookup_waves = env_int ("PEMAP_LOOKUP_WAVES", -1);
  k.lookup_prio = env_int ("PEMAP_LOOKUP_PRIO", 0);
  k.tier2_waves = env_int ("PEMAP_TIER2_WAVES", 3);
  if (k.tier2_waves < 1) k.tier2_waves = 1;
  k.first_tier = env_int ("PEMAP_FIRST_TIER", 1);
  k.vote_prio = env_int ("PEMAP_VOTE_PRIO", 0);
  k.sw_prio = env_int ("PEMAP_SW_PRIO", 0);
  k.vote_waves = env_int ("PEMAP_VOTE_WAVES", 1024);
  if (k.vote_waves < 1) k.vote_waves = 1;
  k.walk_blocks_per_cu = env_int ("PEMAP_WALK_BLOCKS_PER_CU", 4);
  k.pile_blocks_per_cu = env_int ("PEMAP_PILE_BLOCKS_PER_CU", 4);
  if (k.walk_blocks_per_cu < 1) k.walk_blocks_per_cu = 1;
  if (k.pile_blocks_per_cu < 1) k.pile_blocks_per_cu = 1;
  k.pipeline = env_int ("PEMAP_PIPELINE", 1);
  k.chunk_pairs = env_int ("PEMAP_CHUNK_PAIRS", 262144);
  k.band = env_int ("PEMAP_BAND", 1);
  k.band_gate = getenv ("PEMAP_BAND_GATE") ? (env_int ("PEMAP_BAND_GATE", 1) ? 1 : 0) : -1;
  k.gapless_blocks_per_cu = env_int ("PEMAP_GAPLESS_BLOCKS_PER_CU", -1);     // one-wave workgroups of pm_gapless_kernel launched per CU at most; -1: by read length
  if (k.gapless_blocks_per_cu == 0) k.gapless_blocks_per_cu = 1;
  k.band_waves_per_cu = env_int ("PEMAP_BAND_WAVES_PER_CU", 16);
  if (k.band_waves_per_cu < 1) k.band_waves_per_cu = 1;
  k.absorb_staged = env_int ("PEMAP_ABSORB_STAGED", 0) ? 1 : 0;
  const int kib = env_int ("PEMAP_ABSORB_CHUNK", 262144);
  k.absorb_chunk = kib > 0 ? ((size_t) kib * 1024) & ~(size_t) 255 : 0;
  if (k.absorb_chunk < 256) k.absorb_chunk = 256;
}

// ---- fastq text parsed on the device (pemap_dev_stage_fastq / pemap_dev_submit_fastq; kernels: pemap_fastq.hip.h).  Per mate the text, the
// scans' arrays and the records' places; they grow on demand and are the object's.  Every call waits for its own kernels before it
// returns, so one set serves the batches in flight.
struct PmFastqMate
{
  uint8_t *d_text = nullptr;
  size_t text_cap = 0;
  unsigned *d_tile_cnt = nullptr;       // per PFQ_TILE bytes
  size_t tile_cap = 0;
  unsigned *d_line_start = nullptr;     // n_lines + 1
  size_t line_cap = 0;
  PfqTileSum *d_sums = nullptr;         // per PFQ_LINE_TILE lines
  uint2 *d_tile_in = nullptr;
  size_t ltile_cap = 0;
  unsigned *d_rec_off = nullptr, *d_rec_next = nullptr; // max_records
  int *d_rec_len = nullptr;
  size_t rec_cap = 0;
};
struct PmFastq
{
  PmFastqMate mate[2];
  PfqCtl *d_ctl = nullptr;      // [2]
  struct Host { PfqCtl ctl[2]; unsigned next[2]; } *h = nullptr;        // pinned
};

// ---- the object and its groups.  What a pemap_dev owns is split by owner; each group says who makes it and who reads it, and has one
// free function (pointers released and nulled by the primitives below, capacities 0, events destroyed).  pemap_dev_destroy is those
// functions.  An ensure function frees what it re-makes through them and sets the capacity behind the last allocation: one that fails
// leaves null pointers under a capacity of 0.
template < class ... T > static void pm_free (T * &... p)
{
  ((hipFree (p), p = nullptr), ...);
}

template < class ... T > static void pm_host_free (T * &... p)
{
  ((p ? (void) hipHostFree (p) : (void) 0, p = nullptr), ...);
}

static void pm_event_free (hipEvent_t & e)
{
  (e ? (void) hipEventDestroy (e) : (void) 0, e = nullptr);
}

static void fq_free (PmFastq & F)
{
  for (PmFastqMate & M : F.mate)
    {
      pm_free (M.d_text, M.d_tile_cnt, M.d_line_start, M.d_sums, M.d_tile_in, M.d_rec_off, M.d_rec_next, M.d_rec_len);
      M = PmFastqMate ();
    }
  pm_free (F.d_ctl);
  pm_host_free (F.h);
}

// The index.  Made by pemap_dev_index_alloc (the arrays and sizes; their contents by the caller's copies or build_from_genome) and
// by build_replicas at index_commit (d_rep, d_multi and their figures); read by index_of for every kernel, pemap_dev_buffer, index_share.
struct PmIndexArrays
{
  uint32_t *d_pos_index = nullptr, *d_mers = nullptr;
  uint32_t *d_rep = nullptr, *d_multi = nullptr;        // look-up replicas (pemap_aux.hip.h)
  uint32_t multi_base = 0;
  int n_rep = 0;
  uint64_t multi_units = 0;
  uint8_t *d_genome = nullptr, *d_genome_alloc = nullptr;       // the letters, and the allocation they sit in (padded in front)
  uint32_t *d_contig_starts = nullptr;
  uint64_t n_mers = 0, gsize = 0;
  int n_contigs = 0, idepth = 16;
  bool ready = false;
};

// keep_rep: the replicas' allocation stays for the next index (build_replicas says why); only pemap_dev_destroy releases it
static void index_free (PmIndexArrays & x, bool keep_rep)
{
  pm_free (x.d_pos_index, x.d_mers, x.d_multi, x.d_genome_alloc, x.d_contig_starts);
  if (!keep_rep)
    pm_free (x.d_rep);
  x.d_genome = nullptr;
  x.n_mers = x.gsize = x.multi_units = 0;
  x.n_contigs = x.n_rep = 0;
  x.ready = false;
}

// The pileup.  The planes are made by pemap_dev_index_alloc (the genome sizes them), the cursor by pemap_dev_create, the log by
// ensure_work; the walk and pile kernels write them (pile_of), drain_ins and fold_summary keep the host's side, and the fetch entries,
// pemap_dev_buffer (4) and pemap_dev_absorb read.
struct PmPileup
{
  uint32_t *d_counts = nullptr; // the counter planes (PmPile): 6 planes of plane_words words
  size_t plane_words = 0;
  // plane 0 holds differences while the object maps (PmPile): guarded by mu.  run_slice unfolds, pile_fold folds back for every
  // entry that reads or hands out the counters; d_tiles is the conversions' word per tile of PD_TILE words.
  bool diff = false;
  uint32_t *d_tiles = nullptr;
  PmInsCursor *d_cur = nullptr;
  uint8_t *d_ins_log = nullptr;
  unsigned ins_cap = 0;
  std::vector < uint8_t > h_ins;        // host copy of all insertion-log bytes so far
  long summary[13] = {};
};

// planes_only: what a new index re-makes; the cursor, the log and the host's totals go on
static void pile_free (PmPileup & p, bool planes_only)
{
  pm_free (p.d_counts, p.d_tiles);
  p.plane_words = 0;
  p.diff = false;
  if (planes_only)
    return;
  pm_free (p.d_cur, p.d_ins_log);
  p.ins_cap = 0;
}

// The staged read set: one resident set of reads (stage_reads, stage_fastq, synth_reads) or the ring's PM_RING slots of rows (ring_setup).
// Made by ensure_reads and described by reads_staged / ring_setup / ring_take; read by run_slice (batch_of), by collect and
// ring_queue_run (the outputs) and by fold_summary (h_len).
struct PmReadSet
{
  uint8_t *d_rows[2] = {};      // per mate: cap rows of stride bytes
  int *d_len[2] = {};
  std::vector < int >h_len[2];
  int cap = 0, stride = 0;
  int n = 0, paired = 0, max_len = 0, min_len = 0;      // what is staged: rows, pairing, the longest and the shortest read
  uint32_t *d_m1 = nullptr, *d_m2 = nullptr;    // a run's results: cap_out rows
  int *d_mtype = nullptr;
  int cap_out = 0;
};

// (the two parts ensure_reads re-makes on their own: the mates' arrays, the outputs)
static void reads_free (PmReadSet & r, bool rows, bool outputs)
{
  if (rows)
    {
      pm_free (r.d_rows[0], r.d_rows[1], r.d_len[0], r.d_len[1]);
      r.cap = r.n = 0;
    }
  if (outputs)
    {
      pm_free (r.d_m1, r.d_m2, r.d_mtype);
      r.cap_out = 0;
    }
}

// The chunk work: what the chunks in flight compute in.  pemap_dev_create makes the grids and the sets' events, ensure_work the arrays
// sized by a chunk's read-ends, its direction slabs and its path words, ensure_pipeline the lists; the launch functions read them.
// A part is released by its work_free_* and allocated again for every set.
struct PmChunkWork
{
  PmChunkSet set[PM_SETS];
  int cap_ends = 0;             // read-ends the hit, winner and task arrays hold
  size_t dirbuf_dwords = 0;
  size_t dir_slabs = 0;         // slabs a dirbuf holds for the staged read length; the last one is the dump slab of task-less lane groups
  int path_words = 0, path_cap_ends = 0;
  int lists_cap = 0;
  bool lists_arrays = false;    // the (key, segment) lists exist (not needed, and not allocated, while the fused seed kernel serves)
  uint32_t *d_redo = nullptr;   // cap_ends; used by one stream at a time, like the scratch
  uint32_t *d_seed_scratch = nullptr;   // big_grid spill areas of pm_seed_kernel
  int sw_grid = 0, big_grid = 0;
};

static void work_free_paths (PmChunkWork & w)
{
  for (PmChunkSet & s : w.set)
    pm_free (s.path, s.nsteps);
  w.path_words = w.path_cap_ends = 0;
}

static void work_free_dirs (PmChunkWork & w)
{
  for (PmChunkSet & s : w.set)
    pm_free (s.dirbuf);
  w.dirbuf_dwords = w.dir_slabs = 0;
}

static void work_free_lists (PmChunkWork & w)
{
  for (PmChunkSet & s : w.set)
    pm_free (s.lists.hdr, s.lists.key, s.lists.seg, s.lists.big_list);
  w.lists_cap = 0;
  w.lists_arrays = false;
}

static void work_free_ends (PmChunkWork & w)
{
  for (PmChunkSet & s : w.set)
    {
      PmHits & h = s.hits;
      pm_free (h.n_hits, h.spot, h.gpos, h.nn, h.orient, h.score, h.sti, h.stk, h.slot);
      pm_free (s.wins, s.walks, s.tasks_s, s.tasks_m);
    }
  pm_free (w.d_redo);
  w.cap_ends = 0;
  work_free_paths (w);
}

static void work_free (PmChunkWork & w)
{
  work_free_ends (w);
  work_free_dirs (w);
  work_free_lists (w);
  pm_free (w.d_seed_scratch);
  for (PmChunkSet & s : w.set)
    for (hipEvent_t * e : { &s.ev_lists_ready, &s.ev_lists_free, &s.ev_walk_done })
      pm_event_free (*e);
}

// A run's bookkeeping.  run_slice writes what is queued, absorb_run the totals of what ran; the seed stream, the chunks' counters and
// their timing events are made by ensure_pipeline.  Read by the next run_slice (does it continue the pipeline?), collect and the stats entries.
struct PmRun
{
  int first = 0, n = 0, chunks = 0, L = 0;
  uint64_t ends = 0;
  bool pending = false;         // kernels of the last run still in flight / not yet accounted
  // each chunk's big-end remainder is enqueued exactly once: checked in launch_rest (the round-3 fault)
  uint64_t serial = 0;
  bool rest_twice = false;
  // two-stream pipeline: the look-up kernel of chunk k+1 (memory stream) runs beside vote/SW/walk of chunk k
  hipStream_t stream2 = nullptr;
  PmChunkCtr *d_chunk_ctr = nullptr;    // PM_MAX_CHUNKS
  // where absorb_run copies them, and the insertion cursor behind them: pinned memory of the object's own.  (A copy into heap memory must
  // lie outside every host registration of the process, PmPinned above -- and a heap block may lie where a caller's buffer, registered
  // and since freed, lay: the copy of a run's counters into a std::vector was refused that way, `invalid argument`, in one run of
  // pemapper_hip in some, whatever the library's other sources)
  struct Absorbed { PmChunkCtr ctr[PM_MAX_CHUNKS]; PmInsCursor cur; } *h_absorbed = nullptr;
  std::vector < hipEvent_t > evs;       // PM_NEV per chunk
  int wall_khz = 0;             // ticks of wall_clock64 per millisecond (hipDeviceAttributeWallClockRate): the first tier's own stamps
  uint64_t last_big = 0, last_big2 = 0; // read-ends the fused seed kernel's first tier passed over; of them, left to pm_seed_kernel
  PmCounters last_ctr = {};     // summed over the chunks of the last run
  PmInsCursor last_cur = {};
  float last_ms[PM_NT] = {};
  // the fused seed kernel's first tier: workgroups of the form for S segments that the runtime keeps resident on a CU with the
  // form's LDS (0 = not asked yet), and what the last launch used: the knob, the runtime's answer, workgroups per CU, LDS bytes
  int seed_resident[32] = { };
  int seed_launch[4] = { };
  // which way run_slice and ring_setup went, since the object was made (pemap_dev_pipeline_stats: host integers, guarded by mu)
  uint64_t pstat[PM_NPS] = { };
};

// (the stream goes with the object's other streams, in pemap_dev_destroy)
static void run_free (PmRun & r)
{
  pm_free (r.d_chunk_ctr);
  pm_host_free (r.h_absorbed);
  for (hipEvent_t & e : r.evs)
    pm_event_free (e);
  r.evs.clear ();
}

// The ring of batches in flight.  ring_setup makes the slots' pinned blocks (sized like the read set's rows, which the slots cut up) and
// ring_leave gives the rows back to a resident set; ring_take hands a submit its slot, ring_queue_run fills it in, ring_finish delivers.
struct PmRing
{
  PmRingSlot slot[PM_RING];
  int cap = 0;                  // rows per slot, 0 = the ring is not set up (the staged arrays hold a resident read set)
  unsigned long long seq = 0;
  hipStream_t stream_h2d = nullptr;
};

static bool ring_active (const PmRing & g)     // (mu held)
{
  for (const PmRingSlot & r : g.slot)
    if (r.active)
      return true;
  return false;
}

// blocks_only: what ring_setup re-makes; the slots' events serve the next geometry too
static void ring_free (PmRing & g, bool blocks_only)
{
  for (PmRingSlot & r : g.slot)
    {
      pm_host_free (r.h_len, r.h_res, r.h_rows);
      r.h_rows_bytes = 0;
      if (blocks_only)
        continue;
      pm_event_free (r.ev_done);
      for (hipEvent_t & e : r.ev_copy)
        pm_event_free (e);
      r.ev_copy.clear ();
    }
  g.cap = 0;
}

// The deflated records' way out (pemap_dev_fetch_records_gz): the kernel times of the last call, and the two page-locked blocks the
// members pass through where the caller's buffer is not pinned (made at the first such call, released by pemap_dev_destroy).
#define PM_GZ_BLOCK ((size_t) 8 << 20)
struct PmGzOut
{
  float ms[4] = {};
  char *h_block[2] = {};
};

struct pemap_dev
{
  int device = 0, n_cus = 0;
  PmKnobs kn = {};
  hipStream_t stream = nullptr; // the ALU stream (pemap_dev_create); the seed stream is run.stream2, the copy stream rg.stream_h2d
  char err[512] = "";
  int rep_want = -1;            // settings.  Replicas: -1 = when the memory is there (default), 0 = never, 8 = required
  int paired = 1, min_dist = 0, max_dist = 500, bisulfite = 0;
  double min_align = 0.9;       // MIN_ALIGN default, pemapper.c:151
  PmIndexArrays ix;
  PmPileup pile;
  PmReadSet rd;
  PmChunkWork wk;
  PmRun run;
  std::mutex mu;                // guards the enqueue state: submit / wait may be called from several host threads
  // Submitters are serialised for the whole of a submit (taken BEFORE mu).  ring_finish drops mu while the host blocks on the old
  // batch's event; with mu alone a second submitter saw the same rg.seq there, chose the same slot, and whichever came second went
  // on with a stale slot and `first` -- overwriting an active slot's staging and handing out a ticket of another slot (round-2 review).
  // Waiters take mu only, so a wait is never held up by a submit that blocks on a full ring.
  std::mutex submit_mu;
  PmRing rg;
  PmFastq fq;
  PmGzOut gz;
};

static inline PmPile pile_of (const pemap_dev * d)
{
  PmPile p;
  p.w = d->pile.d_counts;
  p.plane_words = d->pile.plane_words;
  p.genome = d->ix.d_genome;
  return p;
}

static inline PmIndex index_of (const pemap_dev * d)
{
  return PmIndex { d->ix.d_pos_index, d->ix.d_mers, d->ix.d_genome, d->ix.d_contig_starts, d->ix.n_mers, d->ix.gsize, d->ix.n_contigs, d->ix.idepth,
                   d->ix.d_rep, d->ix.d_multi, d->ix.multi_base, d->ix.n_rep };
}

static inline PmParams params_of (const pemap_dev * d)
{
  return PmParams { d->min_dist, d->max_dist, d->min_align, d->bisulfite };
}

static int fail (pemap_dev * d, const char *fmt, ...)
{
  va_list ap;
  va_start (ap, fmt);
  vsnprintf (d ? d->err : g_create_err, 512, fmt, ap);
  va_end (ap);
  return 1;
}

#define HIPCHK(d, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail (d, "%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString (e_)); } while (0)

template < class T > static int dev_alloc (pemap_dev * d, T ** p, size_t n)
{
  *p = nullptr;
  if (n == 0)
    n = 1;
  HIPCHK (d, hipMalloc ((void **) p, n * sizeof (T)));
  return 0;
}

// a device temporary of one function: freed when it goes out of scope, on the early returns of TRY / HIPCHK too
template < class T > struct DevTmp
{
  T *p = nullptr;
  DevTmp () = default;
  DevTmp (const DevTmp &) = delete;
  DevTmp & operator= (const DevTmp &) = delete;
  ~DevTmp () { hipFree (p); }
  operator T * () const { return p; }
};

#define TRY(x) do { int r_ = (x); if (r_) return r_; } while (0)

extern "C" const char *pemap_dev_last_error (const pemap_dev * dev)
{
  return dev ? dev->err : g_create_err;
}

extern "C" void pemap_dev_destroy (pemap_dev * d)
{
  if (!d)
    return;
  hipSetDevice (d->device);
  for (hipStream_t st : { d->stream, d->run.stream2 })
    if (st)
      hipStreamSynchronize (st);
  index_free (d->ix, false);
  pile_free (d->pile, false);
  reads_free (d->rd, true, true);
  work_free (d->wk);
  run_free (d->run);
  ring_free (d->rg, false);
  fq_free (d->fq);
  pm_host_free (d->gz.h_block[0], d->gz.h_block[1]);
  for (hipStream_t st : { d->rg.stream_h2d, d->run.stream2, d->stream })
    if (st)
      hipStreamDestroy (st);
  delete d;
}

// (every failure ends in pemap_dev_destroy, through the pointer's deleter: the stream, the events and the cursor made so far go with it)
extern "C" int pemap_dev_create (pemap_dev ** out, int device_id)
{
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount (&n) != hipSuccess || n <= 0)
    return fail (nullptr, "no HIP device visible: this library has no CPU path");
  if (device_id < 0 || device_id >= n)
    return fail (nullptr, "device %d out of range (0..%d)", device_id, n - 1);
  std::unique_ptr < pemap_dev, void (*) (pemap_dev *) > d (new pemap_dev (), pemap_dev_destroy);
  d->device = device_id;
  if (hipSetDevice (device_id) != hipSuccess)
    return fail (nullptr, "hipSetDevice(%d) failed", device_id);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties (&prop, device_id) != hipSuccess)
    return fail (nullptr, "hipGetDeviceProperties failed");
  if (strncmp (prop.gcnArchName, "gfx950", 6) != 0)
    return fail (nullptr, "device %d is %s: this library is built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
  int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  read_knobs (d->kn);
  if (d->kn.pipeline != 1 && d->kn.pipeline != 2)
    return fail (nullptr, "PEMAP_PIPELINE=%d: the settings are 1 (the default) and 2", d->kn.pipeline);
  // pm_seed_kernel is launched with big_grid blocks; every block owns one spill area of d_seed_scratch, which is sized for
  // big_grid blocks and passed to the kernel as its capacity.  (Round 1: the area was sized by another grid, an A/B run
  // raised big_grid above it through an environment knob, and the blocks beyond it wrote past the allocation: the memory
  // access fault of DESIGN.md section 8.)
  d->wk.sw_grid = cus * d->kn.sw_waves_per_cu;
  d->wk.big_grid = cus * d->kn.big_blocks_per_cu;
  d->n_cus = cus;
  if (hipStreamCreateWithFlags (&d->stream, hipStreamNonBlocking) != hipSuccess)
    return fail (nullptr, "hipStreamCreate failed");
  for (PmChunkSet & s : d->wk.set)
    for (hipEvent_t * e : { &s.ev_lists_ready, &s.ev_lists_free, &s.ev_walk_done })
      if (hipEventCreateWithFlags (e, hipEventDisableTiming) != hipSuccess)
        return fail (nullptr, "hipEventCreate failed");
  if (hipMalloc ((void **) &d->pile.d_cur, sizeof (PmInsCursor)) != hipSuccess)
    return fail (nullptr, "hipMalloc failed");
  hipMemset (d->pile.d_cur, 0, sizeof (PmInsCursor));
  *out = d.release ();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------
static const uint64_t POS_INDEX_N = (1ull << 32) + 1ull;

// Zeros in device memory, there when this returns.  hipMemset of device memory returns before the fill has run, and on the null
// stream it is not ordered against the object's non-blocking streams: the 26 GB pileup of a genome of 2.1 G letters was still being
// cleared, 4 GiB at a time, when a small batch's conversion of plane 0 -- queued a few milliseconds after reset_pileup -- read the
// counts of the positions from 2^31 on (byte 2^32 of the plane), and those stale counts came back as a run-on through the plane.
static int zero_on_stream (pemap_dev * d, void *p, size_t bytes)
{
  HIPCHK (d, hipMemsetAsync (p, 0, bytes, d->stream));
  HIPCHK (d, hipStreamSynchronize (d->stream));
  return 0;
}

extern "C" int pemap_dev_index_alloc (pemap_dev * d, uint64_t n_mers, uint64_t genome_size, int n_contigs, int idepth)
{
  HIPCHK (d, hipSetDevice (d->device));
  if (genome_size == 0 || genome_size >= (1ull << 32) - 400 || n_contigs < 1)
    return fail (d, "index_alloc: genome_size %llu / n_contigs %d not supported (positions are u32)",
                 (unsigned long long) genome_size, n_contigs);
  if (idepth != 16)
    return fail (d, "index_alloc: idepth %d: the .idx table is addressed by 16-mers (index_genome_whole.c:149)", idepth);
  index_free (d->ix, true);
  pile_free (d->pile, true);
  d->ix.n_mers = n_mers;
  d->ix.gsize = genome_size;
  d->ix.n_contigs = n_contigs;
  d->ix.idepth = idepth;
  TRY (dev_alloc (d, &d->ix.d_pos_index, POS_INDEX_N));
  TRY (dev_alloc (d, &d->ix.d_mers, n_mers + 128));
  // (256 bytes in front, 512 behind: pm_band_kernel's window loads start a few bytes before a window and the kernels' 8-byte loads
  // end a few bytes behind one; d_genome points at the first letter)
  TRY (dev_alloc (d, &d->ix.d_genome_alloc, genome_size + 768));
  HIPCHK (d, hipMemset (d->ix.d_genome_alloc, 0, 256));
  d->ix.d_genome = d->ix.d_genome_alloc + 256;
  TRY (dev_alloc (d, &d->ix.d_contig_starts, (size_t) n_contigs + 2));
  // (a plane is a whole number of 256-byte blocks: planes start line-aligned)
  const size_t plane_words = (((size_t) genome_size + 2) / 2 + 63) & ~(size_t) 63;
  TRY (dev_alloc (d, &d->pile.d_counts, 6 * plane_words));
  TRY (dev_alloc (d, &d->pile.d_tiles, (plane_words + PD_TILE - 1) / PD_TILE));
  d->pile.plane_words = plane_words;
  HIPCHK (d, hipMemset (d->ix.d_genome + genome_size, 0, 512));
  TRY (zero_on_stream (d, d->pile.d_counts, 6 * d->pile.plane_words * sizeof (uint32_t)));
  return 0;
}

// The 8 look-up replicas and the records of the multi-position buckets (pemap_aux.hip.h), from pos_index / mers.
static int build_replicas (pemap_dev * d)
{
  pm_free (d->ix.d_multi);
  d->ix.n_rep = 0;
  int want = d->rep_want;
  if (want < 0 && d->kn.replicas >= 0)
    want = d->kn.replicas ? 8 : 0;
  if (want == 0)
    {
      pm_free (d->ix.d_rep);
      return 0;
    }
  const size_t rep_bytes = 8ull * (1ull << 32) * sizeof (uint32_t);
  if (!d->ix.d_rep)
    {
      // The replicas' 128 GiB are allocated once per object and kept across indexes.  What must stay free beside them for
      // the work arrays of a run (direction slabs, hit records, lists) and the records is probed by allocating it.  The
      // driver hands freed memory back lazily (an allocation of this size right after a hipFree of the same size fails,
      // and hipMemGetInfo lags too), hence the retries.
      const size_t reserve = (size_t) 48 << 30;
      bool ok = false;
      {
        // the common case, a fresh process: the free-memory figure is accurate, no probe needed (a 48 GiB allocation costs ~1 s)
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo (&fr, &tot) == hipSuccess && fr >= rep_bytes + reserve)
          {
            if (hipMalloc ((void **) &d->ix.d_rep, rep_bytes) == hipSuccess)
              ok = true;
            else
              {
                (void) hipGetLastError ();
                d->ix.d_rep = nullptr;
              }
          }
      }
      for (int attempt = 0; attempt < 10 && !ok; attempt++)
        {
          void *probe = nullptr;
          if (attempt)
            {
              (void) hipDeviceSynchronize ();
              usleep (300000);
            }
          if (hipMalloc ((void **) &d->ix.d_rep, rep_bytes) == hipSuccess)
            {
              if (hipMalloc (&probe, reserve) == hipSuccess)
                ok = true;
              else
                pm_free (d->ix.d_rep);
              hipFree (probe);
            }
          if (!ok)
            {
              (void) hipGetLastError ();
              d->ix.d_rep = nullptr;
            }
        }
      if (!ok)
        {
          if (want == 8)
            return fail (d, "look-up replicas: the device cannot hold %.1f GB beside the index and %.1f GB of work arrays", rep_bytes / 1e9, reserve / 1e9);
          // the reference's layout serves the look-ups (pm_lookup_wave_kernel): same results, about 1.6x the time per step
          fprintf (stderr, "libpemap_hip: device %d has no room for the %.0f GB of look-up replicas beside the index and %.0f GB of work arrays; "
                   "the look-ups read the reference's table instead (slower, same results; PEMAP_REPLICAS=0 silences this)\n", d->device,
                   rep_bytes / 1e9, reserve / 1e9);
          return 0;
        }
    }
  uint32_t *units = d->ix.d_rep + (1ull << 32);    // replica 1's place holds the record offsets until replica 0 is encoded
  const uint64_t n = 1ull << 32;
  const unsigned grid = (unsigned) d->n_cus * 64u;
  hipLaunchKernelGGL (ix_rep_units_kernel, dim3 (grid), dim3 (256), 0, d->stream, d->ix.d_pos_index, units);
  const uint64_t sc_tiles = (n + SC_TILE - 1) / SC_TILE;
  DevTmp < unsigned long long > d_total;
  DevTmp < uint32_t > d_tsum;
  TRY (dev_alloc (d, &d_tsum.p, sc_tiles));
  TRY (dev_alloc (d, &d_total.p, 1));
  hipLaunchKernelGGL (ix_sumscan_reduce_kernel, dim3 ((unsigned) sc_tiles), dim3 (SC_BLOCK), 0, d->stream, units, n, d_tsum);
  hipLaunchKernelGGL (ix_sumscan_tiles_kernel, dim3 (1), dim3 (1024), 0, d->stream, d_tsum, sc_tiles, d_total);
  unsigned long long total = 0;
  HIPCHK (d, hipMemcpyAsync (&total, d_total, sizeof (total), hipMemcpyDeviceToHost, d->stream));
  HIPCHK (d, hipStreamSynchronize (d->stream));
  // entries below multi_base are positions (compressed coordinates < genome size); codes up to 0xFFFFFFFD address the records
  d->ix.multi_base = (uint32_t) d->ix.gsize;
  const bool fits = total < (unsigned long long) (0xFFFFFFFEu - d->ix.multi_base);
  if (fits)
    {
      hipLaunchKernelGGL (ix_sumscan_apply_kernel, dim3 ((unsigned) sc_tiles), dim3 (SC_BLOCK), 0, d->stream, units, n, d_tsum);
      TRY (dev_alloc (d, &d->ix.d_multi, (size_t) total * 4 + 64));
      hipLaunchKernelGGL (ix_rep_encode_kernel, dim3 (grid), dim3 (256), 0, d->stream, d->ix.d_pos_index, d->ix.d_mers, units, d->ix.multi_base, d->ix.d_rep,
                          d->ix.d_multi);
      for (int p = 1; p < 8; p++)
        hipLaunchKernelGGL (ix_rep_permute_kernel, dim3 ((unsigned) d->n_cus * 32u), dim3 (256), 0, d->stream, d->ix.d_rep,
                            d->ix.d_rep + ((size_t) p << 32), p);
    }
  HIPCHK (d, hipStreamSynchronize (d->stream));
  HIPCHK (d, hipGetLastError ());
  if (!fits)
    {
      if (want == 8)
        return fail (d, "look-up replicas: %llu record units do not fit the codes above genome size %llu", total, (unsigned long long) d->ix.gsize);
      // as when the memory is not there: the reference's layout serves the look-ups
      fprintf (stderr, "libpemap_hip: device %d: the look-up replicas need %llu record units and a genome of %llu letters leaves codes for %llu; "
               "the look-ups read the reference's table instead (slower, same results; PEMAP_REPLICAS=0 silences this)\n", d->device, total,
               (unsigned long long) d->ix.gsize, (unsigned long long) (0xFFFFFFFEu - d->ix.multi_base - 1u));
      return 0;
    }
  d->ix.multi_units = total;
  d->ix.n_rep = 8;
  return 0;
}

extern "C" int pemap_dev_set_lookup_replicas (pemap_dev * d, int n)
{
  if (n != -1 && n != 0 && n != 8)
    return fail (d, "set_lookup_replicas: %d (-1 = when the memory is there, 0 = never, 8 = required)", n);
  d->rep_want = n;
  if (d->ix.ready)
    {
      HIPCHK (d, hipSetDevice (d->device));
      HIPCHK (d, hipDeviceSynchronize ());
      return build_replicas (d);
    }
  return 0;
}

extern "C" int pemap_dev_lookup_replicas (pemap_dev * d, int *n_replicas, uint64_t * record_bytes)
{
  *n_replicas = d->ix.n_rep;
  if (record_bytes)
    *record_bytes = d->ix.n_rep ? d->ix.multi_units * 16ull : 0ull;
  return 0;
}

extern "C" int pemap_dev_index_commit (pemap_dev * d)
{
  if (!d->ix.d_pos_index)
    return fail (d, "index_commit: no index arrays allocated");
  HIPCHK (d, hipSetDevice (d->device));
  HIPCHK (d, hipDeviceSynchronize ());
  TRY (build_replicas (d));
  d->ix.ready = true;
  return 0;
}

extern "C" int pemap_dev_load_index (pemap_dev * d, const uint32_t * pos_index, const uint32_t * mers, uint64_t n_mers,
                                     const char *genome, uint64_t genome_size, const uint32_t * contig_starts, int n_contigs,
                                     int idepth)
{
  TRY (pemap_dev_index_alloc (d, n_mers, genome_size, n_contigs, idepth));
  HIPCHK (d, hipMemcpy (d->ix.d_pos_index, pos_index, POS_INDEX_N * sizeof (uint32_t), hipMemcpyHostToDevice));
  HIPCHK (d, hipMemcpy (d->ix.d_mers, mers, n_mers * sizeof (uint32_t), hipMemcpyHostToDevice));
  HIPCHK (d, hipMemcpy (d->ix.d_genome, genome, genome_size, hipMemcpyHostToDevice));
  HIPCHK (d, hipMemcpy (d->ix.d_contig_starts, contig_starts, ((size_t) n_contigs + 1) * sizeof (uint32_t), hipMemcpyHostToDevice));
  return pemap_dev_index_commit (d);
}

// the index of a genome that lies on the host or on the device (`from`)
static int build_from_genome (pemap_dev * d, const void *genome, hipMemcpyKind from, uint64_t gsize, const uint32_t * contig_len, int n_contigs, int bisulfite)
{
  TRY (pemap_dev_index_alloc (d, 0, gsize, n_contigs, 16));
  HIPCHK (d, hipMemcpy (d->ix.d_genome, genome, gsize, from));
  std::vector < uint64_t > real_starts (n_contigs + 1);
  std::vector < uint32_t > cstarts (n_contigs + 1);
  real_starts[0] = 0;
  cstarts[0] = 0;
  for (int c = 0; c < n_contigs; c++)
    {
      if (contig_len[c] < 16)
        return fail (d, "build_index: contig %d has %u letters; fewer than 16 is not indexable", c, contig_len[c]);
      real_starts[c + 1] = real_starts[c] + contig_len[c];
      cstarts[c + 1] = cstarts[c] + (contig_len[c] - 15);       // index_genome_whole.c:213, 316, 349
    }
  if (real_starts[n_contigs] != gsize)
    return fail (d, "build_index: contig lengths sum to %llu, genome has %llu letters", (unsigned long long) real_starts[n_contigs],
                 (unsigned long long) gsize);
  HIPCHK (d, hipMemcpy (d->ix.d_contig_starts, cstarts.data (), (n_contigs + 1) * sizeof (uint32_t), hipMemcpyHostToDevice));
  {
    // the temporaries (some 3 x n_mers words) are released, last one first, before the replicas are built
    DevTmp < uint64_t > d_real, d_total, d_to;
    DevTmp < uint32_t > d_tc, d_vals, d_keys2, d_keys, d_tmax;
    DevTmp < void > d_tmp;
    TRY (dev_alloc (d, &d_real.p, (size_t) n_contigs + 1));
    HIPCHK (d, hipMemcpy (d_real, real_starts.data (), (n_contigs + 1) * sizeof (uint64_t), hipMemcpyHostToDevice));
    const uint64_t n_tiles = (gsize + IX_PER_BLOCK - 1) / IX_PER_BLOCK;
    TRY (dev_alloc (d, &d_tc.p, n_tiles));
    TRY (dev_alloc (d, &d_to.p, n_tiles));
    TRY (dev_alloc (d, &d_total.p, 1));
    hipLaunchKernelGGL (ix_count_kernel, dim3 ((unsigned) n_tiles), dim3 (IX_BLOCK), 0, d->stream, d->ix.d_genome, d_real, n_contigs, gsize,
                        bisulfite, d_tc);
    hipLaunchKernelGGL (ix_scan_tiles_kernel, dim3 (1), dim3 (1024), 0, d->stream, d_tc, d_to, n_tiles, d_total);
    uint64_t n_mers = 0;
    HIPCHK (d, hipMemcpyAsync (&n_mers, d_total, sizeof (uint64_t), hipMemcpyDeviceToHost, d->stream));
    HIPCHK (d, hipStreamSynchronize (d->stream));
    if (n_mers == 0)
      return fail (d, "build_index: the genome has no 16-mer free of N");
    TRY (dev_alloc (d, &d_keys.p, n_mers));
    TRY (dev_alloc (d, &d_vals.p, n_mers));
    TRY (dev_alloc (d, &d_keys2.p, n_mers));
    pm_free (d->ix.d_mers);
    TRY (dev_alloc (d, &d->ix.d_mers, n_mers + 128));
    d->ix.n_mers = n_mers;
    hipLaunchKernelGGL (ix_emit_kernel, dim3 ((unsigned) n_tiles), dim3 (IX_BLOCK), 0, d->stream, d->ix.d_genome, d_real, n_contigs, gsize,
                        bisulfite, d_to, d_keys, d_vals);
    // stable LSD radix sort by k-mer: equal k-mers keep genome order, which is the .mdx order
    size_t tmp_bytes = 0;
    HIPCHK (d, rocprim::radix_sort_pairs (nullptr, tmp_bytes, d_keys.p, d_keys2.p, d_vals.p, d->ix.d_mers, (size_t) n_mers, 0, 32, d->stream));
    HIPCHK (d, hipMalloc (&d_tmp.p, tmp_bytes ? tmp_bytes : 1));
    HIPCHK (d, rocprim::radix_sort_pairs (d_tmp.p, tmp_bytes, d_keys.p, d_keys2.p, d_vals.p, d->ix.d_mers, (size_t) n_mers, 0, 32, d->stream));
    // prefix table: bucket ends scattered, then a running maximum over 2^32 + 1 entries
    HIPCHK (d, hipMemsetAsync (d->ix.d_pos_index, 0, POS_INDEX_N * sizeof (uint32_t), d->stream));
    hipLaunchKernelGGL (ix_run_ends_kernel, dim3 ((unsigned) ((n_mers + 255) / 256)), dim3 (256), 0, d->stream, d_keys2, n_mers,
                        d->ix.d_pos_index);
    const uint64_t sc_tiles = (POS_INDEX_N + SC_TILE - 1) / SC_TILE;
    TRY (dev_alloc (d, &d_tmax.p, sc_tiles));
    hipLaunchKernelGGL (ix_maxscan_reduce_kernel, dim3 ((unsigned) sc_tiles), dim3 (SC_BLOCK), 0, d->stream, d->ix.d_pos_index, POS_INDEX_N, d_tmax);
    hipLaunchKernelGGL (ix_maxscan_tiles_kernel, dim3 (1), dim3 (1024), 0, d->stream, d_tmax, sc_tiles);
    hipLaunchKernelGGL (ix_maxscan_apply_kernel, dim3 ((unsigned) sc_tiles), dim3 (SC_BLOCK), 0, d->stream, d->ix.d_pos_index, POS_INDEX_N, d_tmax);
    HIPCHK (d, hipStreamSynchronize (d->stream));
    HIPCHK (d, hipGetLastError ());
  }
  return pemap_dev_index_commit (d);
}

extern "C" int pemap_dev_build_index (pemap_dev * d, const char *genome, uint64_t genome_size, const uint32_t * contig_len,
                                      int n_contigs, int bisulfite)
{
  return build_from_genome (d, genome, hipMemcpyHostToDevice, genome_size, contig_len, n_contigs, bisulfite);
}

extern "C" int pemap_dev_build_index_resident (pemap_dev * d, const void *d_genome, uint64_t genome_size,
                                               const uint32_t * contig_len, int n_contigs, int bisulfite)
{
  return build_from_genome (d, d_genome, hipMemcpyDeviceToDevice, genome_size, contig_len, n_contigs, bisulfite);
}

// ---- plane 0 between counts and differences (PmPile, pemap_pile_diff.h).  Both conversions run on the ALU stream, behind whatever
// is queued there; both want mu held.  On an hg38-sized plane either moves 6.2 GB in and out.
struct PmConvTimer
{
  hipEvent_t ev[2] = {};
  bool on = false;
  PmConvTimer (hipStream_t st)
  {
    on = hipEventCreate (&ev[0]) == hipSuccess && hipEventCreate (&ev[1]) == hipSuccess && hipEventRecord (ev[0], st) == hipSuccess;
  }
  void stop (hipStream_t st)
  {
    on = on && hipEventRecord (ev[1], st) == hipSuccess;
  }
  // (after the stream was waited for)
  void report (const char *what)
  {
    float ms = 0.f;
    if (on && hipEventElapsedTime (&ms, ev[0], ev[1]) == hipSuccess)
      fprintf (stderr, "libpemap_hip: plane 0 %s in %.3f ms\n", what, ms);
  }
  ~PmConvTimer ()
  {
    pm_event_free (ev[0]);
    pm_event_free (ev[1]);
  }
};

// counts -> differences, enqueued only: the pile kernels behind it on the stream find differences
static int pile_unfold_locked (pemap_dev * d)
{
  if (d->pile.diff)
    return 0;
  const uint64_t n_words = d->pile.plane_words, n_tiles = (n_words + PD_TILE - 1) / PD_TILE;
  uint64_t sgrid = (n_tiles + PD_BLOCK - 1) / PD_BLOCK;
  if (sgrid > (uint64_t) d->n_cus * 8)
    sgrid = (uint64_t) d->n_cus * 8;
  const bool log = env_int ("PEMAP_PILE_CONV_LOG", 0) != 0;
  std::unique_ptr < PmConvTimer > tm (log ? new PmConvTimer (d->stream) : nullptr);
  hipLaunchKernelGGL (pd_unfold_save_kernel, dim3 ((unsigned) sgrid), dim3 (PD_BLOCK), 0, d->stream, d->pile.d_counts, n_tiles, d->pile.d_tiles);
  hipLaunchKernelGGL (pd_unfold_apply_kernel, dim3 ((unsigned) n_tiles), dim3 (PD_BLOCK), 0, d->stream, d->pile.d_counts, n_words, d->pile.d_tiles);
  HIPCHK (d, hipGetLastError ());
  if (tm)
    {
      // (the logged figure is worth a wait: the knob is for measuring)
      tm->stop (d->stream);
      HIPCHK (d, hipStreamSynchronize (d->stream));
      tm->report ("unfolded");
    }
  d->pile.diff = true;
  return 0;
}

// differences -> counts, and waited for: afterwards the planes hold what the reference's array would
static int pile_fold_locked (pemap_dev * d)
{
  if (!d->pile.diff)
    return 0;
  HIPCHK (d, hipSetDevice (d->device));
  const uint64_t n_words = d->pile.plane_words, n_tiles = (n_words + PD_TILE - 1) / PD_TILE;
  DevTmp < unsigned long long > d_total;
  TRY (dev_alloc (d, &d_total.p, 1));
  // PEMAP_PILE_CONV_LOG=1: either conversion's time on the device goes to stderr
  const bool log = env_int ("PEMAP_PILE_CONV_LOG", 0) != 0;
  std::unique_ptr < PmConvTimer > tm (log ? new PmConvTimer (d->stream) : nullptr);
  hipLaunchKernelGGL (pd_fold_sums_kernel, dim3 ((unsigned) n_tiles), dim3 (PD_BLOCK), 0, d->stream, d->pile.d_counts, n_words, d->pile.d_tiles);
  hipLaunchKernelGGL (ix_sumscan_tiles_kernel, dim3 (1), dim3 (1024), 0, d->stream, d->pile.d_tiles, n_tiles, d_total);
  hipLaunchKernelGGL (pd_fold_apply_kernel, dim3 ((unsigned) n_tiles), dim3 (PD_BLOCK), 0, d->stream, d->pile.d_counts, n_words, d->pile.d_tiles);
  if (tm)
    tm->stop (d->stream);
  HIPCHK (d, hipGetLastError ());
  HIPCHK (d, hipStreamSynchronize (d->stream));
  if (tm)
    tm->report ("folded");
  d->pile.diff = false;
  return 0;
}

static int pile_fold (pemap_dev * d)
{
  std::lock_guard < std::mutex > lk (d->mu);
  return pile_fold_locked (d);
}

// drain the device insertion log into the host copy and reset the cursor (stream must be idle)
static int drain_ins (pemap_dev * d)
{
  HIPCHK (d, hipStreamSynchronize (d->stream));
  PmInsCursor cur;
  HIPCHK (d, hipMemcpy (&cur, d->pile.d_cur, sizeof (cur), hipMemcpyDeviceToHost));
  unsigned nb = cur.ins_bytes;
  if (nb > d->pile.ins_cap)
    nb = d->pile.ins_cap;
  if (nb)
    {
      size_t at = d->pile.h_ins.size ();
      d->pile.h_ins.resize (at + nb);
      HIPCHK (d, hipMemcpy (d->pile.h_ins.data () + at, d->pile.d_ins_log, nb, hipMemcpyDeviceToHost));
    }
  HIPCHK (d, hipMemset (d->pile.d_cur, 0, sizeof (PmInsCursor)));
  d->run.last_cur.ins_bytes = 0;
  return 0;
}

extern "C" int pemap_dev_buffer (pemap_dev * d, int which, void **d_ptr, uint64_t * n_bytes)
{
  if (!d->ix.d_pos_index)
    return fail (d, "buffer: no index");
  if (which == 4)
    TRY (pile_fold (d));        // the view holds counts when it is handed out (include/pemap_hip.h)
  switch (which)
    {
    case 0: *d_ptr = d->ix.d_pos_index; *n_bytes = POS_INDEX_N * 4; break;
    case 1: *d_ptr = d->ix.d_mers; *n_bytes = d->ix.n_mers * 4; break;
    case 2: *d_ptr = d->ix.d_genome; *n_bytes = d->ix.gsize; break;
    case 3: *d_ptr = d->ix.d_contig_starts; *n_bytes = ((uint64_t) d->ix.n_contigs + 1) * 4; break;
    case 4: *d_ptr = d->pile.d_counts; *n_bytes = 6 * d->pile.plane_words * 4; break;
    case 5: *d_ptr = d->ix.d_rep; *n_bytes = d->ix.n_rep ? 8ull * (1ull << 32) * 4ull : 0ull; break;
    case 6: *d_ptr = d->ix.d_multi; *n_bytes = d->ix.n_rep ? d->ix.multi_units * 16ull : 0ull; break;
    default: return fail (d, "buffer: which = %d", which);
    }
  return 0;
}

extern "C" int pemap_dev_index_info (pemap_dev * d, uint64_t * n_mers, uint64_t * genome_size, int *n_contigs, int *idepth)
{
  if (!d->ix.ready)
    return fail (d, "index_info: no index");
  *n_mers = d->ix.n_mers;
  *genome_size = d->ix.gsize;
  *n_contigs = d->ix.n_contigs;
  *idepth = d->ix.idepth;
  return 0;
}

extern "C" int pemap_dev_read_buffer (pemap_dev * d, int which, uint64_t byte_offset, void *host_dst, uint64_t n_bytes)
{
  void *p;
  uint64_t nb;
  TRY (pemap_dev_buffer (d, which, &p, &nb));
  if (byte_offset + n_bytes > nb)
    return fail (d, "read_buffer: range beyond buffer %d (%llu bytes)", which, (unsigned long long) nb);
  HIPCHK (d, hipSetDevice (d->device));
  HIPCHK (d, hipStreamSynchronize (d->stream));
  HIPCHK (d, hipMemcpy (host_dst, (const char *) p + byte_offset, n_bytes, hipMemcpyDeviceToHost));
  return 0;
}

// ---- staging: the read set's arrays and what they hold.  Either part is released through reads_free before it is made again and gets
// its capacity behind its last allocation: where one fails the part is empty (null, capacity 0, nothing staged) and the next call makes it.
static int ensure_reads (pemap_dev * d, int n, int stride, int paired)
{
  PmReadSet & R = d->rd;
  if (n > R.cap || stride != R.stride || (paired && !R.d_rows[1]))
    {
      const int cap = n > R.cap ? n : R.cap;
      reads_free (R, true, false);
      for (int m = 0; m < 2; m++)
        {
          TRY (dev_alloc (d, &R.d_rows[m], (size_t) cap * stride + 64));
          TRY (dev_alloc (d, &R.d_len[m], (size_t) cap));
        }
      R.cap = cap;
      R.stride = stride;
    }
  if (n > R.cap_out)
    {
      reads_free (R, false, true);
      TRY (dev_alloc (d, &R.d_m1, (size_t) n));
      TRY (dev_alloc (d, &R.d_m2, (size_t) n));
      TRY (dev_alloc (d, &R.d_mtype, (size_t) n));
      R.cap_out = n;
    }
  return 0;
}

// the arrays hold n rows (pairs, if paired) whose lengths lie in mn..mx
static void reads_staged (pemap_dev * d, int n, int paired, int mx, int mn)
{
  d->rd.n = n;
  d->rd.paired = paired ? 1 : 0;
  d->rd.max_len = mx;
  d->rd.min_len = mn;
}

static int check_lengths (pemap_dev * d, const int *len, int n, int *mx, int *mn)
{
  for (int i = 0; i < n; i++)
    {
      if (len[i] < PEMAP_MIN_READ || len[i] > PEMAP_MAX_READ)
        return fail (d, "read %d has length %d: supported range is %d..%d", i, len[i], PEMAP_MIN_READ, PEMAP_MAX_READ);
      if (len[i] > *mx)
        *mx = len[i];
      if (len[i] < *mn)
        *mn = len[i];
    }
  return 0;
}

// result fold of one finished batch, pemapper.c:1238-1265
static void fold_summary (pemap_dev * d, int first, int n, const uint32_t * m1, const uint32_t * m2, const int *mapping_type)
{
  long *S = d->pile.summary;
  for (int j = 0; j < n; j++)
    {
      uint32_t a = m1[j], b = (d->paired && m2) ? m2[j] : 0;
      int la = d->rd.h_len[0][first + j], lb = d->paired ? d->rd.h_len[1][first + j] : 0;
      S[4 + mapping_type[j]]++;
      if (a)
        {
          S[0]++;
          S[1] += la;
          if (b)
            {
              S[0]++;
              S[1] += lb;
              long test = (long) (uint32_t) (a - b);    // unsigned difference widened to long, pemapper.c:1250
              if (test < (long) d->max_dist * 4)
                {
                  S[2] += test;
                  S[3]++;
                }
            }
        }
      else if (b)
        {
          S[0]++;
          S[1] += lb;
        }
    }
}

// SW geometry for the longest staged read L: lanes per alignment and W columns per lane, the smallest instantiation with
// lanes * W >= L.  8 lanes x 13 columns up to 104 bases.  Beyond that 16 lanes (x 10 / 13 / 16 / 19 columns): beside the gapless
// rule the DP sees few problems per launch and the finer form wins (2 x 150 bp: 44.8 ms per step against 46.2 with 8 x 19;
// 2 x 250 bp: 111.8 against 120.5 with 8 x 32); with the rule off (PEMAP_GAPLESS=0: every problem through the DP) reads of
// 105..152 bases take 8 x 19, which was 18 % faster there.  (8 x 26 / 32 / 38 and 12 x 13 were measured equal or slower and are gone.)
// PEMAP_GAPLESS=0: every problem goes through the DP (the rule of pm_gapless_kernel off); 1: its first case only (diagonals
// with at most one mismatch); 2: the first two (best diagonal with two mismatches, as before case (3) existed: the A/B switch
// inside one build); default 3: all three (best diagonal with three mismatches on a full-width window)
static int pm_gapless_max_x (const pemap_dev * d)
{
  return d->kn.gapless;
}

static bool pm_gapless_on (const pemap_dev * d)
{
  return d->kn.gapless != 0;
}

static void pick_geom (const pemap_dev * d, int L, int *lanes, int *w)
{
  if (L <= 8 * 13) { *lanes = 8; *w = 13; }
  else if (!pm_gapless_on (d) && L <= 8 * 19) { *lanes = 8; *w = 19; }
  else if (L <= 16 * 10) { *lanes = 16; *w = 10; }
  else if (L <= 16 * 13) { *lanes = 16; *w = 13; }
  else if (L <= 16 * 16) { *lanes = 16; *w = 16; }
  else { *lanes = 16; *w = 19; }
}

// what a batch whose longest read has read_len bases runs with on this object (host code only: nothing is launched)
extern "C" int pemap_dev_sw_geom (pemap_dev * d, int read_len, int *lanes, int *columns)
{
  if (!lanes || !columns)
    return fail (d, "sw_geom: lanes and columns must not be NULL");
  if (read_len < PEMAP_MIN_READ || read_len > PEMAP_MAX_READ)
    return fail (d, "sw_geom: read length %d: supported range is %d..%d", read_len, PEMAP_MIN_READ, PEMAP_MAX_READ);
  pick_geom (d, read_len, lanes, columns);
  return 0;
}

// f (PmInt < W > {}, PmInt < LPA > {}) for the SW geometry of reads up to L bases: one instantiation per form pick_geom can choose
template < int N > using PmInt = std::integral_constant < int, N >;
template < class F > static void with_sw_geom (const pemap_dev * d, int L, F f)
{
  int lanes, w;
  pick_geom (d, L, &lanes, &w);
  if (lanes == 8 && w == 13) f (PmInt < 13 > {}, PmInt < 8 > {});
  else if (lanes == 8) f (PmInt < 19 > {}, PmInt < 8 > {});
  else if (w == 10) f (PmInt < 10 > {}, PmInt < 16 > {});
  else if (w == 13) f (PmInt < 13 > {}, PmInt < 16 > {});
  else if (w == 16) f (PmInt < 16 > {}, PmInt < 16 > {});
  else f (PmInt < 19 > {}, PmInt < 16 > {});
}

// rows of one lane's region in a direction slab: window rows + the skew steps, rounded up to the 16-step flush unit
static int tstride_for (const pemap_dev * d, int L)
{
  int lanes, w;
  pick_geom (d, L, &lanes, &w);
  return (L + 21 + lanes + 15) & ~15;
}

static size_t slab_dwords_for (const pemap_dev * d, int L)
{
  int lanes, W;
  pick_geom (d, L, &lanes, &W);
  return (size_t) lanes * (size_t) tstride_for (d, L) * (size_t) ((W * 4 + 31) / 32);
}

// device bytes the direction slabs of one chunk may take (one slab per read-end); PEMAP_DIR_BUDGET_GB overrides
static size_t dir_budget_bytes (const pemap_dev * d)
{
  return (size_t) (d->kn.dir_budget_gb * 1073741824.0);
}

// ---- a chunk's SW problems of one kind, those of the read-ends with exactly one hit or those of the ends with several, as the DP
// cascade (launch_cascade) sees them.  A set's task array is PM_TASK_QUARTERS quarters of task_quarter_words words: every problem
// (written by the seed stage), then what the gapless rule leaves to the full DP, to the banded DP, and to its own second launch.
#define PM_TASK_QUARTERS 4
struct PmTaskList
{
  uint32_t *all, *dp, *band, *c3;       // band: null with PEMAP_BAND=0; c3: null below PEMAP_GAPLESS=3 unless the band's gate needs it
  unsigned *n_all, *n_dp, *n_band, *n_c3, *dp_next, *band_next; // the lists' lengths; the work counters of the full and the banded DP
  unsigned *n_gate;             // problems the second launch admits to the band by the two-diagonal bound; null with PEMAP_BAND_GATE=0
                                // (launch_cascade passes it on for the chunks in which the bound is tested)
};

static size_t task_quarter_words (int n_ends, bool multi)
{
  return (size_t) n_ends * (multi ? PM_MAX_HITS : 1);
}

static PmTaskList task_list (const pemap_dev * d, const PmChunkSet & S, PmCounters * ctr, bool multi)
{
  uint32_t *const t = multi ? S.tasks_m : S.tasks_s;
  const size_t q = task_quarter_words (d->wk.cap_ends, multi);
  const bool rule = pm_gapless_on (d);
  PmTaskList l;
  l.all = t;
  l.n_all = multi ? &ctr->n_tasks_m : &ctr->n_tasks_s;
  l.dp = rule ? t + q : l.all;  // (PEMAP_GAPLESS=0: no rule, the full DP takes the seed stage's list as it is)
  l.n_dp = !rule ? l.n_all : multi ? &ctr->n_tasks_mdp : &ctr->n_tasks_dp;
  l.band = rule && d->kn.band ? t + 2 * q : nullptr;
  // (the two-diagonal bound is tested in the rule's second launch: its problems travel in case (3)'s list)
  l.n_gate = l.band && d->kn.band_gate ? &ctr->n_gate[multi] : nullptr;
  l.c3 = rule && (pm_gapless_max_x (d) >= 3 || l.n_gate) ? t + 3 * q : nullptr;
  l.n_band = &ctr->n_band[multi];
  l.n_c3 = &ctr->n_c3[multi];
  l.dp_next = &ctr->sw_next[multi];
  l.band_next = &ctr->band_next[multi];
  return l;
}

static int ensure_work (pemap_dev * d, int n_ends)
{
  if (n_ends > d->wk.cap_ends)
    {
      work_free_ends (d->wk);
      for (PmChunkSet & s : d->wk.set)
        {
          PmHits & h = s.hits;
          const size_t nh = (size_t) n_ends * PM_MAX_HITS;
          TRY (dev_alloc (d, &h.n_hits, (size_t) n_ends));
          TRY (dev_alloc (d, &h.slot, (size_t) n_ends));
          TRY (dev_alloc (d, &h.spot, nh));
          TRY (dev_alloc (d, &h.gpos, nh));
          TRY (dev_alloc (d, &h.nn, nh));
          TRY (dev_alloc (d, &h.orient, nh));
          TRY (dev_alloc (d, &h.score, nh));
          TRY (dev_alloc (d, &h.sti, nh));
          TRY (dev_alloc (d, &h.stk, nh));
          TRY (dev_alloc (d, &s.wins, (size_t) n_ends));
          TRY (dev_alloc (d, &s.walks, (size_t) n_ends));
          TRY (dev_alloc (d, &s.tasks_s, task_quarter_words (n_ends, false) * PM_TASK_QUARTERS));
          TRY (dev_alloc (d, &s.tasks_m, task_quarter_words (n_ends, true) * PM_TASK_QUARTERS));
        }
      TRY (dev_alloc (d, &d->wk.d_redo, (size_t) n_ends));
      d->wk.cap_ends = n_ends;
    }
  if (!d->wk.d_seed_scratch)
    TRY (dev_alloc (d, &d->wk.d_seed_scratch, (size_t) d->wk.big_grid * 6 * PM_MAX_SEG * PM_SEG_LIST_MAX));
  const size_t need = ((size_t) n_ends + 1) * slab_dwords_for (d, d->rd.max_len); // + 1: dump slab for task-less lane groups
  if (need > d->wk.dirbuf_dwords)
    {
      work_free_dirs (d->wk);
      for (PmChunkSet & s : d->wk.set)
        TRY (dev_alloc (d, &s.dirbuf, need));
      d->wk.dirbuf_dwords = need;
    }
  d->wk.dir_slabs = d->wk.dirbuf_dwords / slab_dwords_for (d, d->rd.max_len);
  // recorded traceback steps: PM_PATH_WORDS words of 32 two-bit steps per read-end
  const int pwords = PM_PATH_WORDS (d->rd.max_len);
  if (n_ends > d->wk.path_cap_ends || pwords != d->wk.path_words)
    {
      work_free_paths (d->wk);
      for (PmChunkSet & s : d->wk.set)
        {
          TRY (dev_alloc (d, &s.path, (size_t) n_ends * pwords));
          TRY (dev_alloc (d, &s.nsteps, (size_t) n_ends));
        }
      d->wk.path_words = pwords;
      d->wk.path_cap_ends = n_ends;
    }
  // insertion log: 64 bytes per read-end of a chunk is ample for real data, and at least 512 MB so that runs queued back to
  // back (the log is drained when a run is absorbed) do not fill it; overflow is reported as an error
  size_t want = (size_t) n_ends * 64 + (1u << 20);
  if (want < ((size_t) 512 << 20))
    want = (size_t) 512 << 20;
  if (want > 0xF0000000ull)
    want = 0xF0000000ull;
  if (want > d->pile.ins_cap)
    {
      TRY (drain_ins (d));
      pm_free (d->pile.d_ins_log);
      d->pile.ins_cap = 0;     // (set again behind the allocation: a log that is not there holds nothing)
      TRY (dev_alloc (d, &d->pile.d_ins_log, want));
      d->pile.ins_cap = (unsigned) want;
    }
  return 0;
}

static int seg_template (int L)
{
  const int segs = L / 16 + ((L % 16) ? 1 : 0);      // len/16 (+1 unless divisible), pemapper.c:1573-1587
  return segs <= 7 ? 7 : segs <= 10 ? 10 : segs <= 13 ? 13 : segs <= 16 ? 16 : 19;
}

// f (std::integral_constant < int, SM >) for the segment template SM of reads up to L bases
template < class F > static void with_seg_template (int L, F f)
{
  switch (seg_template (L))
    {
    case 7: f (std::integral_constant < int, 7 > {}); break;
    case 10: f (std::integral_constant < int, 10 > {}); break;
    case 13: f (std::integral_constant < int, 13 > {}); break;
    case 16: f (std::integral_constant < int, 16 > {}); break;
    default: f (std::integral_constant < int, 19 > {}); break;
    }
}

// chunk size run_slice cuts a run of n pairs of reads up to L bases into
static int chunk_pairs_for (const pemap_dev * d, int n, int L)
{
  const int per = d->paired ? 2 : 1;
  // one direction slab per read-end must fit the budget; the pipeline wants several chunks per run
  size_t slab_bytes = slab_dwords_for (d, L) * 4;
  long max_ends = (long) (dir_budget_bytes (d) / slab_bytes);
  if (max_ends > 20000000)
    max_ends = 20000000;        // task ids are end * 200 + hit in 32 bits
  int chunk = (int) (max_ends / per);
  const int want = d->kn.chunk_pairs;
  if (want > 0 && chunk > want)
    chunk = want;
  if (chunk < 1)
    chunk = 1;
  if (chunk > n)
    chunk = n;
  if ((n + chunk - 1) / chunk > PM_MAX_CHUNKS)
    chunk = (n + PM_MAX_CHUNKS - 1) / PM_MAX_CHUNKS;
  return chunk;
}

__global__ void pm_nop_kernel ()
{
}

// PEMAP_FIRST_TIER=0: the list the first tier would leave had it passed over every end of the chunk
__global__ void pm_all_big_kernel (uint32_t * list, unsigned *n_list, int n_ends)
{
  const int i = (int) (blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n_ends)
    list[i] = (uint32_t) i;
  if (i == 0)
    *n_list = (unsigned) n_ends;
}

struct RunCtx
{
  PmIndex ix;
  PmBatch b;
  PmParams prm;
  int tstride, L;
  size_t dump_off;              // dwords from the start of a set's dirbuf to its dump slab
};

#ifndef PM_LOOKUP_WAVES_DEFAULT
#define PM_LOOKUP_WAVES_DEFAULT 12
#endif

// is the seed stage of this run the fused kernel (pm_seed4_kernel: look-ups and vote of a read-end in one wave)?
static bool pm_fused (const pemap_dev * d)
{
  return d->ix.n_rep == 8;
}

// The seed stage's schedule, decided once per run by run_slice ("The seed stage's schedule"):
//   layout     PEMAP_PIPELINE  seed stream, per chunk                                 ALU stream, per chunk, before the DP
//   fused      1               tier 0, tier 1, remainder, emit unless emit_on_alu     emit, if emit_on_alu
//   reference  1               look-ups                                               vote, remainder, emit
//   either     2               the same kernels in the same order, all on the ALU stream, no look-ahead
struct PmSchedule
{
  hipStream_t seed;             // the seed stage's stream: stream2, or the ALU stream with PEMAP_PIPELINE=2
  bool ahead;                   // the seed stage runs PM_SETS chunks ahead of the ALU stream
  bool emit_on_alu;             // the fused layout's emit kernel goes to the ALU stream in front of the chunk's DP
};

// does the look-up launch of a chunk stamp its own interval (PmChunkCtr::t_lookup_begin / t_lookup_end)?  The fused kernel's first
// tier does; the reference layout, PEMAP_FIRST_TIER=0 and a build with the phase probes keep the empty kernel and the two events
static bool pm_stamped (const pemap_dev * d)
{
#ifdef PEMAP_TIMING_PROBES
  return false;
#else
  return pm_fused (d) && d->kn.first_tier && d->run.wall_khz > 0;  // (a device without a wall clock rate keeps the events)
#endif
}

// ---- the look-ups of one chunk: the fused seed kernel's two tiers, or the reference layout's look-ups into the set's lists
static void launch_lookup (pemap_dev * d, const RunCtx & c, PmChunkSet & S, PmChunkCtr * cc, hipEvent_t * ev, hipStream_t st)
{
  PmLists L = S.lists;
  L.n_big = &cc->n_big;
  L.positions = &cc->positions;
  L.next_end = &cc->next_end;
  // (an event recorded straight after a stream wait is stamped when the wait is queued, not when it is satisfied: the empty
  // kernel makes the stamp the moment the look-up kernel can start, so that LOOKUP_BEGIN..LOOKUP_END is the kernel's own duration.
  // The fused first tier stamps its interval itself, pm_stamped: no empty kernel and neither event in front of it)
  const bool stamped = pm_stamped (d);
  if (stamped)
    {
      L.t_begin = &cc->t_lookup_begin;
      L.t_end = &cc->t_lookup_end;
    }
  else
    {
      hipLaunchKernelGGL (pm_nop_kernel, dim3 (1), dim3 (1), 0, st);
      hipEventRecord (ev[PM_EV_LOOKUP_BEGIN], st);
    }
  // PEMAP_LOOKUP_WAVES=n: n persistent one-wave workgroups per CU (pm_seed4_kernel: 12,784 bytes of LDS and 128 VGPRs a wave).  The
  // kernel itself keeps gaining with n (5.06 / 4.53 / 4.05 / 3.84 ms per launch with 7 / 8 / 9 / 10, profiles/r04_ab_sweeps.txt) while the
  // other stream's DP kernels lose the SIMDs' registers to it.  Ten was the most 14,976 bytes admitted; twelve is what
  // profiles/r13_ab_sweeps.txt found with the smaller struct (10: 110.0 M reads/s; 11 and 12: 115.4 and 115.3 .. 116.0, not told apart)
  const int lw_asked = d->kn.lookup_waves > 0 ? d->kn.lookup_waves : PM_LOOKUP_WAVES_DEFAULT;
  int lw = lw_asked;
  if (pm_fused (d))
    {
      // (no more workgroups than are resident at once: a workgroup owns its first ends by its number, and one that starts when
      // another ends -- at the launch's end -- would be the launch's tail.  How many are is the runtime's answer for the form and
      // its dynamic LDS, asked once per form)
      size_t lds = 0;
      int per_simd = 2, fit = 0;
      with_seg_template (c.L, [&] (auto sm)
      {
        lds = sizeof (PmSeed4Shared < sm.value, 0 >);
        if (sm.value <= 10)
          per_simd = PM_S4_WAVES_PER_EU;
        int &res = d->run.seed_resident[sm.value];
        if (res <= 0 && hipOccupancyMaxActiveBlocksPerMultiprocessor (&res, pm_seed4_kernel < sm.value, 0 >, 64, lds) != hipSuccess)
          res = 0;
        fit = res;
      });
      if (fit < 1)
        fit = 1;
      const int resident = fit;
      if (lw > fit)
        lw = fit;
      if (lw > 4 * per_simd)
        lw = 4 * per_simd;
      d->run.seed_launch[0] = lw_asked;
      d->run.seed_launch[1] = resident;
      d->run.seed_launch[2] = lw;
      d->run.seed_launch[3] = (int) lds;
    }
  int lgrid = lw * d->n_cus;
  if (lgrid > c.b.n_ends)
    lgrid = c.b.n_ends;
  const int lprio = d->kn.lookup_prio;
  const PmHits & H = S.hits;
  if (!pm_fused (d))
    {
      with_seg_template (c.L, [&] (auto sm)
      {
        hipLaunchKernelGGL (HIP_KERNEL_NAME (pm_lookup_wave_kernel < sm.value, 4 >), dim3 (lgrid), dim3 (64), 0, st, c.ix, c.b, c.prm, L, lprio);
      });
      hipEventRecord (ev[PM_EV_LOOKUP_END], st);
      return;
    }
  // the fused seed kernel's first tier, then its second tier over the ends the first passed over: the same kernel with four times
  // the list (twice, for reads over 160 bases), a few waves per CU -- most launches find a few thousand ends; what THAT leaves goes
  // to pm_seed_kernel (launch_rest)
  PmLists L2 = L;
  L2.t_begin = L2.t_end = nullptr;
  L2.big_list = L.big_list + d->wk.lists_cap;
  L2.n_big = &cc->n_big2;
  L2.next_end = &cc->next_end2;
  const int grid2 = d->kn.tier2_waves * d->n_cus;
  with_seg_template (c.L, [&] (auto sm)
  {
    if (d->kn.first_tier)
      hipLaunchKernelGGL (HIP_KERNEL_NAME (pm_seed4_kernel < sm.value, 0 >), dim3 (lgrid), dim3 (64), sizeof (PmSeed4Shared < sm.value, 0 >), st, c.ix, c.b,
                          c.prm, H, L, (const uint32_t *) nullptr, (const unsigned *) nullptr, lprio);
    else if (c.b.n_ends > 0)    // (a chunk's ends fit the list: run_slice sizes it by the chunk)
      hipLaunchKernelGGL (pm_all_big_kernel, dim3 ((unsigned) (c.b.n_ends + 255) / 256), dim3 (256), 0, st, L.big_list, L.n_big, c.b.n_ends);
    if (!stamped)
      hipEventRecord (ev[PM_EV_LOOKUP_END], st);
    hipLaunchKernelGGL (HIP_KERNEL_NAME (pm_seed4_kernel < sm.value, 1 >), dim3 (grid2), dim3 (64), sizeof (PmSeed4Shared < sm.value, 1 >), st, c.ix, c.b,
                        c.prm, H, L2, (const uint32_t *) L.big_list, (const unsigned *) L.n_big, lprio);
  });
  // the vote is part of the kernel: its interval is empty
  hipEventRecord (ev[PM_EV_VOTE_BEGIN], st);
  hipEventRecord (ev[PM_EV_VOTE_END], st);
}

// ---- the reference layout's vote kernel on the set's lists; VOTE_BEGIN..VOTE_END is its own interval
static void launch_vote (pemap_dev * d, const RunCtx & c, PmChunkSet & S, PmChunkCtr * cc, hipEvent_t * ev, hipStream_t st)
{
  PmLists L = S.lists;
  L.n_big = &cc->n_big;
  L.positions = &cc->positions;
  const PmHits & H = S.hits;
  // PEMAP_VOTE_WAVES=n: at most n one-wave workgroups per CU, each striding over the ends.  Default 1024 = one wave per end: the
  // dispatcher then places vote waves wherever the look-up and SW waves of the other stream leave room (measured 71.6 ms per
  // step against 74.9 with 12 persistent waves per CU)
  const int vprio = d->kn.vote_prio;
  int vgrid = d->kn.vote_waves * d->n_cus;
  if (vgrid > c.b.n_ends)
    vgrid = c.b.n_ends;
  hipLaunchKernelGGL (pm_nop_kernel, dim3 (1), dim3 (1), 0, st);
  hipEventRecord (ev[PM_EV_VOTE_BEGIN], st);
  with_seg_template (c.L, [&] (auto sm)
  {
    hipLaunchKernelGGL (HIP_KERNEL_NAME (pm_vote_wave_kernel < sm.value >), dim3 (vgrid), dim3 (64), 0, st, c.ix, c.b, c.prm, H, L, vprio);
  });
  hipEventRecord (ev[PM_EV_VOTE_END], st);
}

// ---- the big-end remainder: pm_seed_kernel over the read-ends the look-up / vote kernels (the fused kernel's second tier) passed
//      over; then the set's lists are consumed
static void launch_rest (pemap_dev * d, const RunCtx & c, PmChunkSet & S, PmChunkCtr * cc, hipStream_t st)
{
  // The remainder writes the raw hit lists of its ends and uses the one spill scratch: a second launch for the same chunk would share
  // that scratch with the first (the fault PEMAP_REST_STREAM3=1 produced in round 3, when it still appended to the task lists).
  // Refused here, reported by run_slice.  (It touches neither n_tasks_s nor n_slots: pm_emit_kernel, which numbers the slabs by
  // the single-hit task numbers, is their only writer before pm_select_kernel.)
  const uint64_t id = (d->run.serial << 24) | (uint64_t) (cc - d->run.d_chunk_ctr);
  if (S.rest_id == id)
    {
      d->run.rest_twice = true;
      return;
    }
  S.rest_id = id;
  const uint32_t *list = S.lists.big_list;
  const unsigned *n_list = &cc->n_big;
  if (pm_fused (d))
    {
      list += d->wk.lists_cap;
      n_list = &cc->n_big2;
    }
  with_seg_template (c.L, [&] (auto sm)
  {
    hipLaunchKernelGGL (HIP_KERNEL_NAME (pm_seed_kernel < sm.value >), dim3 (d->wk.big_grid), dim3 (PM_SEED_THREADS), 0, st, c.ix, c.b, c.prm, S.hits, S.tasks_s,
                        S.tasks_m, &cc->c, d->wk.d_seed_scratch, d->wk.big_grid, list, n_list);
  });
  hipEventRecord (S.ev_lists_free, st);
}

// ---- the emit kernel (windows, slab numbers, SW task lists); the seed stage ends here
static void launch_emit (pemap_dev * d, const RunCtx & c, PmChunkSet & S, PmChunkCtr * cc, hipEvent_t * ev, hipStream_t st)
{
  const int per_wave = 64 * PM_EMIT_ROUNDS;
  hipLaunchKernelGGL (pm_emit_kernel, dim3 ((c.b.n_ends + per_wave - 1) / per_wave), dim3 (64), 0, st, c.ix, c.b, S.hits, S.tasks_s, S.tasks_m, &cc->c);
  hipEventRecord (ev[PM_EV_SEED_END], st);
}

// ---- the seed stream's work for chunk g (the chunk's rows in c.b)
static int enqueue_seed (pemap_dev * d, const PmSchedule & s, const RunCtx & c, int g, const hipEvent_t * copy_ev)
{
  PmChunkSet & S = d->wk.set[g % PM_SETS];
  PmChunkCtr *cc = d->run.d_chunk_ctr + g;
  hipEvent_t *ev = &d->run.evs[(size_t) g * PM_NEV];
  if (copy_ev)
    HIPCHK (d, hipStreamWaitEvent (s.seed, *copy_ev, 0));
  // the set's lists must have been consumed by the remainder of chunk g - PM_SETS
  if (g >= PM_SETS)
    HIPCHK (d, hipStreamWaitEvent (s.seed, S.ev_lists_free, 0));
  if (pm_fused (d))
    {
      // the fused kernel writes the hit arrays that the SW / walk of chunk g - PM_SETS used
      if (g >= PM_SETS && s.ahead)
        HIPCHK (d, hipStreamWaitEvent (s.seed, S.ev_walk_done, 0));
      launch_lookup (d, c, S, cc, ev, s.seed);
      // the remainder: 256-thread workgroups with 31 KB of LDS, which find no room beside the next chunk's persistent seed waves --
      // here, between two seed launches, they do (and mostly find nothing to do)
      launch_rest (d, c, S, cc, s.seed);
      if (!s.emit_on_alu)
        launch_emit (d, c, S, cc, ev, s.seed);
    }
  else
    launch_lookup (d, c, S, cc, ev, s.seed);
  HIPCHK (d, hipEventRecord (S.ev_lists_ready, s.seed));
  return 0;
}

// ---- one launch of the gapless rule over `tasks`; short_rows: the form whose rows hold reads of up to PM_GL_SHORT_MM bases
template < bool C3 > static void launch_gapless (pemap_dev * d, bool short_rows, int ggrid, const RunCtx & c, const PmChunkSet & S, const uint32_t * tasks,
                                                 const unsigned *n_tasks, const PmTaskList & l, int max_x, uint32_t * tasks_c3, unsigned *n_tasks_c3)
{
  if (short_rows)
    hipLaunchKernelGGL (HIP_KERNEL_NAME (pm_gapless_kernel < C3, true >), dim3 (ggrid), dim3 (PM_GL_BLOCK), 0, d->stream, c.ix, c.b, c.prm, S.hits, tasks, n_tasks,
                        l.dp, l.n_dp, max_x, l.band, l.n_band, tasks_c3, n_tasks_c3, l.n_gate);
  else
    hipLaunchKernelGGL (HIP_KERNEL_NAME (pm_gapless_kernel < C3, false >), dim3 (ggrid), dim3 (PM_GL_BLOCK), 0, d->stream, c.ix, c.b, c.prm, S.hits, tasks, n_tasks,
                        l.dp, l.n_dp, max_x, l.band, l.n_band, tasks_c3, n_tasks_c3, l.n_gate);
}

// ---- the DP cascade over one task list, on the ALU stream: the gapless rule, its second launch for case (3), the banded DP, the full
//      DP.  DIRS: the single-hit ends' list, scored with direction nibbles (the multi-hit ends' problems get scores only; a winner the
//      rule decided is not scored again).  (`auto`: instantiated where launch_chunk names it, which keeps the kernels' order in the code object)
template < int W, int LPA, bool DIRS > static auto launch_cascade (pemap_dev * d, const RunCtx & c, const PmChunkSet & S, PmCounters * ctr, const PmTaskList & l)
{
  const int n_ends = c.b.n_ends, max_x = pm_gapless_max_x (d);
  // The two-diagonal bound takes work off the full DP where that launch is more than one pass of its grid (sw_grid persistent waves,
  // 64 / LPA problems each at a time): a list cannot be longer than the chunk has read-ends, so a chunk of no more ends than that
  // keeps the routing by x <= 6 alone -- its full DP is one pass whatever the band takes, and the problems are spared the second
  // launch.  PEMAP_BAND_GATE=1 / 0 decide for every chunk.  (The outputs are the same either way.)
  PmTaskList lg = l;
  if (d->kn.band_gate < 0 && (long) n_ends <= (long) d->wk.sw_grid * (64 / LPA))
    lg.n_gate = nullptr;
  // the multi-hit list's rule and band launches fill the device; the single-hit list holds at most one problem per read-end
  int ggrid = d->n_cus * 16, bgrid = d->n_cus * d->kn.band_waves_per_cu;
  if (DIRS)
    {
      // The rule's kernel and the NEXT chunk's seed kernel are launched at the same moment (both wait for this chunk's seed kernel), and
      // whichever gets its waves onto the SIMDs first keeps them: the seed kernel's persistent waves (pm_seed4_kernel < 10, 0 >, twelve per
      // CU) take 128 registers and 12,800 bytes of LDS each, this kernel's 109 to 115 registers (four fill a SIMD's 512) and 1 KB of LDS
      // with short rows.  Beside ten seed waves (the default up to round 12; twelve leave a wave per SIMD) a CU has room for six of these waves by registers (1 + 1 + 2 + 2) and for eight
      // to ten by LDS (allocated in units of 1,280 or of 512 bytes); where these come first, sixteen of them hold a CU's registers
      // until they end.  (Until round 10 the kernel had one form, compiled for six waves per SIMD -- 80 registers and 96 to 112 bytes
      // of scratch per lane -- whose 1.7 KB of LDS admitted four or five beside ten seed waves.)
      // For reads of up to 160 bases 24 workgroups per CU are the measured optimum (the seed
      // kernel's launch is short of its 7 waves per CU for 0.4 ms at most); for longer reads the seed kernel's launches are twice
      // as long, its waves came up late on many CUs, and the step was 69 ms with 12 or more against 54 with 6 (2 x 245 bases:
      // profiles/r03_ab_sweeps.txt; round 2's 256-thread workgroups had hidden this: they rarely found room at all).  Since the
      // kernel takes 109 to 115 registers instead of 80, four per CU are the optimum there (2 x 245: 54.95 M reads/s against 54.72
      // with 6, 54.35 with 8, 54.10 with 12; profiles/r10_ab_sweeps.txt)
      const int gbp = d->kn.gapless_blocks_per_cu > 0 ? d->kn.gapless_blocks_per_cu : (seg_template (c.L) <= 10 ? 24 : 4);
      ggrid = (n_ends + PM_GL_PER_BLOCK - 1) / PM_GL_PER_BLOCK;
      if (ggrid > d->n_cus * gbp)
        ggrid = d->n_cus * gbp;
      if (bgrid > (n_ends + 15) / 16)
        bgrid = (n_ends + 15) / 16;
    }
  // (reads of up to PM_GL_SHORT_MM = 160 bases, the seed stage's class boundary: the kernel's short rows, 1 KB of LDS per workgroup)
  const bool short_rows = seg_template (c.L) <= 10;
  if (pm_gapless_on (d))
    launch_gapless < false > (d, short_rows, ggrid, c, S, l.all, l.n_all, lg, max_x, l.c3, l.n_c3);
  // case (3) in a launch of its own over the problems it may decide (one in eight; what it refuses joins the DP's lists), and with
  // them the problems without a good diagonal, which it sends to the band if two diagonals and one gap prove the band's premise
  if (l.c3)
    launch_gapless < true > (d, short_rows, ggrid, c, S, l.c3, l.n_c3, lg, max_x, (uint32_t *) nullptr, (unsigned *) nullptr);
  // the problems the rule left open whose best diagonal has few mismatches: the DP restricted to a band of 32 diagonals,
  // four lanes per problem (pemap_band.hip.h); what is left for pm_sw_kernel are mostly the reads with a real indel
  if (l.band)
    hipLaunchKernelGGL (HIP_KERNEL_NAME (pm_band_kernel < DIRS >), dim3 (bgrid), dim3 (64), 0, d->stream, c.ix, c.b, c.prm, S.hits, l.band, l.n_band, ctr,
                        S.dirbuf, slab_dwords_for (d, c.L), l.band_next);
  hipLaunchKernelGGL (HIP_KERNEL_NAME (pm_sw_kernel < W, LPA, DIRS >), dim3 (d->wk.sw_grid), dim3 (64), 0, d->stream, c.ix, c.b, c.prm, S.hits, l.dp, l.n_dp, ctr,
                      S.dirbuf, S.dirbuf + c.dump_off, c.tstride, c.L, d->kn.sw_prio, l.dp_next);
}

// ---- the ALU stream's work for one chunk: the rest of the seed stage, SW, selection, traceback.
template < int W, int LPA > static void launch_chunk (pemap_dev * d, const PmSchedule & s, const RunCtx & c, uint32_t * m1, uint32_t * m2, int *mt,
                                             PmChunkSet & S, PmChunkCtr * cc, hipEvent_t * ev)
{
  const PmHits & H = S.hits;
  uint32_t *wins = S.wins, *dirbuf = S.dirbuf;
  PmCounters *ctr = &cc->c;
  if (!pm_fused (d))
    {
      launch_vote (d, c, S, cc, ev, d->stream);
      launch_rest (d, c, S, cc, d->stream);
      launch_emit (d, c, S, cc, ev, d->stream);
    }
  else if (s.emit_on_alu)
    launch_emit (d, c, S, cc, ev, d->stream);
  launch_cascade < W, LPA, true > (d, c, S, ctr, task_list (d, S, ctr, false));
  hipEventRecord (ev[PM_EV_SW_SINGLE_END], d->stream);
  launch_cascade < W, LPA, false > (d, c, S, ctr, task_list (d, S, ctr, true));
  hipEventRecord (ev[PM_EV_SW_MULTI_END], d->stream);
  hipLaunchKernelGGL (pm_select_kernel, dim3 ((c.b.n + 63) / 64), dim3 (64), 0, d->stream, c.b, c.prm, H, d->wk.d_redo, wins, S.walks,
                      ctr, m1, m2, mt);
  hipEventRecord (ev[PM_EV_SELECT_END], d->stream);
  hipLaunchKernelGGL (HIP_KERNEL_NAME (pm_sw_kernel < W, LPA, true >), dim3 (d->wk.sw_grid), dim3 (64), 0, d->stream, c.ix, c.b, c.prm, H,
                      d->wk.d_redo, &ctr->n_redo, ctr, dirbuf, dirbuf + c.dump_off, c.tstride, c.L, d->kn.sw_prio, &ctr->sw_next[2]);
  hipEventRecord (ev[PM_EV_SW_REDO_END], d->stream);
  // PEMAP_WALK_BLOCKS_PER_CU (default 4, swept 1..16): resident 256-lane blocks of the walk per CU; few enough walkers that
  // their direction lines stay in L2 between steps
  const int wbp = d->kn.walk_blocks_per_cu;
  int wgrid = (c.b.n_ends + 63) / 64;
  if (wgrid > d->n_cus * wbp * 4)
    wgrid = d->n_cus * wbp * 4;         // (waves: the knob counts blocks of four)
  // (the walk on the look-up stream, beside the next chunk's vote and SW, was tried: 107 ms per step against 103; it stays here)
  hipLaunchKernelGGL (HIP_KERNEL_NAME (pm_walk_kernel < W, LPA >), dim3 (wgrid), dim3 (64), 0, d->stream, c.b, H, wins, S.walks, ctr, d->pile.d_cur,
                      dirbuf, c.tstride, pile_of (d), d->pile.d_ins_log, d->pile.ins_cap, S.path, d->wk.path_words, S.nsteps);
  // the winners applied to the pileup: the plain diagonals two to a wave, then the walked ones, one wave each, by their recorded steps
  // PEMAP_PILE_BLOCKS_PER_CU (default 4, swept 2 / 3 / 4 / 6 / 8 in round 9): the waves wait for their atomics' old words, and more of
  // them than this only take wave slots from the seed kernel on the other stream
  const int pbp = d->kn.pile_blocks_per_cu;
  int pgrid = c.b.n_ends;
  if (pgrid > d->n_cus * pbp * 4)
    pgrid = d->n_cus * pbp * 4;         // (waves: the knob counts blocks of four)
  hipLaunchKernelGGL (pm_pile_kernel, dim3 (pgrid), dim3 (64), 0, d->stream, c.b, H, wins, ctr, pile_of (d));
  hipLaunchKernelGGL (pm_pile_walked_kernel, dim3 (pgrid), dim3 (64), 0, d->stream, c.b, H, wins, S.walks, ctr, pile_of (d), S.path, d->wk.path_words, S.nsteps);
  hipEventRecord (ev[PM_EV_WALK_END], d->stream);
  hipEventRecord (S.ev_walk_done, d->stream);
}

// wait for the run in flight and fold its chunks' counters and kernel times into the run's totals
static int absorb_run (pemap_dev * d)
{
  HIPCHK (d, hipStreamSynchronize (d->run.stream2));
  HIPCHK (d, hipStreamSynchronize (d->stream));
  const int nch = d->run.chunks;
#ifdef PEMAP_TIMING_PROBES
  {
    // the fused seed kernel's phase probes (pemap_seed4.hip.h): cycles summed over waves, printed per run
    unsigned long long pr2[2][32], z[2][32] = { { 0ull } };
    if (hipMemcpyFromSymbol (pr2, HIP_SYMBOL (pm_s4_probe), sizeof pr2) == hipSuccess)
      {
        for (int tier = 0; tier < 2; tier++)
          {
            const unsigned long long *pr = pr2[tier];
            unsigned long long tot = 0;
            for (int i = 0; i < 16; i++)
              tot += pr[i];
            if (!tot)
              continue;
            // (marks 0 to 2 -- the lines' copies to LDS and the first strand's decode -- went with the line requests: a lane holds
            // its own entries, both strands are decoded in one run of rounds, which waits for the entries: mark 3)
            static const char *nm[16] = { "-", "-", "-", "wait+decode", "records-end", "stage next", "segmask", "candidates", "relevant", "pairs", "rank+walk", "out", "rec:headers", "rec:scan+3", "-", "rec:tails" };
            fprintf (stderr, "[pm_s4_probe tier %d]", tier);
            for (int i = 0; i < 16; i++)
              fprintf (stderr, " %s %.1f%%", nm[i], 100.0 * (double) pr[i] / (double) tot);
            fprintf (stderr, " | total %.3f G wave-cycles | segments %llu, dropped for a too-many bucket %llu, of them by the k-mer's own bucket %llu\n", (double) tot / 1e9, pr[16], pr[17], pr[18]);
            fprintf (stderr, "[pm_s4_probe tier %d] ends decoded %llu; passed over: the list's room %llu, positions next to candidates %llu\n", tier, pr[20], pr[21], pr[23]);
          }
        (void) hipMemcpyToSymbol (HIP_SYMBOL (pm_s4_probe), z, sizeof z);
      }
  }
#endif
  const PmChunkCtr *const hc = d->run.h_absorbed->ctr;
  HIPCHK (d, hipMemcpy (d->run.h_absorbed->ctr, d->run.d_chunk_ctr, sizeof (PmChunkCtr) * nch, hipMemcpyDeviceToHost));
  HIPCHK (d, hipMemcpy (&d->run.h_absorbed->cur, d->pile.d_cur, sizeof (PmInsCursor), hipMemcpyDeviceToHost));
  d->run.last_cur = d->run.h_absorbed->cur;
  PmCounters & t = d->run.last_ctr;
  for (int k = 0; k < nch; k++)
    {
      const PmCounters & c = hc[k].c;
      t.n_tasks_s += c.n_tasks_s;
      t.n_tasks_m += c.n_tasks_m;
      t.n_tasks_dp += pm_gapless_on (d) ? c.n_tasks_dp : c.n_tasks_s;
      t.n_tasks_mdp += pm_gapless_on (d) ? c.n_tasks_mdp : c.n_tasks_m;
      t.n_band[0] += c.n_band[0];
      t.n_band[1] += c.n_band[1];
      t.n_gate[0] += c.n_gate[0];
      t.n_gate[1] += c.n_gate[1];
      t.cells_band += c.cells_band;
      t.n_slots += c.n_slots;
      t.n_redo += c.n_redo;
      t.n_wins += c.n_wins;
      t.n_walks += c.n_walks;
      t.positions += c.positions + hc[k].positions;
      t.cells_score += c.cells_score;
      t.cells_dirs += c.cells_dirs;
      t.pile_incs += c.pile_incs;
      t.n_ins += c.n_ins;
      d->run.last_big += hc[k].n_big;
      d->run.last_big2 += hc[k].n_big2;
      hipEvent_t *ev = &d->run.evs[(size_t) k * PM_NEV];
      float ms = 0.f;
      // (a first tier that stamped its own interval -- its stamps are zeroed with the chunk's counters -- recorded no look-up events.
      // Workgroup 0 is not bound to start first: the interval may miss the few microseconds by which another workgroup was earlier, and
      // a chunk whose end stamp is not behind its begin -- a launch in which workgroup 0 came up last -- adds nothing to `lookup`)
      const bool stamped = hc[k].t_lookup_end != 0ull;
      if (stamped && hc[k].t_lookup_end > hc[k].t_lookup_begin)
        {
          ms = (float) ((double) (hc[k].t_lookup_end - hc[k].t_lookup_begin) / (double) d->run.wall_khz);
          d->run.last_ms[PM_T_LOOKUP] += ms;
          d->run.last_ms[PM_T_SEED] += ms;
        }
      for (const auto & iv : pm_intervals)
        if (stamped && iv.from == PM_EV_LOOKUP_BEGIN)
          continue;
        else if (hipEventElapsedTime (&ms, ev[iv.from], ev[iv.to]) == hipSuccess)
          {
            d->run.last_ms[iv.slot] += ms;
            d->run.last_ms[PM_T_SEED] += iv.seed_too ? ms : 0.f;
          }
    }
  if (d->run.last_cur.ins_overflow)
    return fail (d, "insertion log overflow (%u bytes): lower PEMAP_CHUNK_PAIRS or map smaller slices", d->pile.ins_cap);
  if (d->run.last_cur.ins_bytes > d->pile.ins_cap / 2)
    return drain_ins (d);
  return 0;
}

static int absorb_pending (pemap_dev * d)
{
  if (d->run.pending)
    {
      TRY (absorb_run (d));
      d->run.pending = false;
    }
  return 0;
}

static int ensure_pipeline (pemap_dev * d, int chunk_ends)
{
  // (a CU mask and stream priorities for the look-up stream were tried in rounds 1 and 2 and gave nothing)
  if (!d->run.stream2)
    HIPCHK (d, hipStreamCreateWithFlags (&d->run.stream2, hipStreamNonBlocking));
  // (asked once; -1: the device reports none, and the look-ups are timed by events as before)
  if (d->run.wall_khz == 0 && (hipDeviceGetAttribute (&d->run.wall_khz, hipDeviceAttributeWallClockRate, d->device) != hipSuccess || d->run.wall_khz <= 0))
    d->run.wall_khz = -1;
  if (d->run.evs.empty ())
    {
      // (the counters and the events are there together or not at all: the next call tries again)
      int rc = dev_alloc (d, &d->run.d_chunk_ctr, (size_t) PM_MAX_CHUNKS);
      if (!rc && hipHostMalloc ((void **) &d->run.h_absorbed, sizeof (*d->run.h_absorbed), hipHostMallocDefault) != hipSuccess)
        rc = fail (d, "hipHostMalloc of the absorbed counters failed");
      d->run.evs.resize ((size_t) PM_MAX_CHUNKS * PM_NEV, nullptr);
      for (size_t i = 0; !rc && i < d->run.evs.size (); i++)
        if (hipEventCreate (&d->run.evs[i]) != hipSuccess)
          rc = fail (d, "hipEventCreate failed");
      if (rc)
        {
          run_free (d->run);
          return rc;
        }
    }
  if (chunk_ends > d->wk.lists_cap || (chunk_ends > 0 && !pm_fused (d) && !d->wk.lists_arrays))
    {
      if (chunk_ends < d->wk.lists_cap)
        chunk_ends = d->wk.lists_cap;
      // (the look-up kernels of a pending run may still be writing the old arrays)
      TRY (absorb_pending (d));
      work_free_lists (d->wk);
      // (the fused seed kernel keeps the lists in LDS: only the big-end list is needed then)
      const size_t list_ends = pm_fused (d) ? 0 : (size_t) chunk_ends;
      for (PmChunkSet & s : d->wk.set)
        {
          TRY (dev_alloc (d, &s.lists.hdr, list_ends));
          TRY (dev_alloc (d, &s.lists.key, list_ends * 2 * PM_SEED_CAP));
          TRY (dev_alloc (d, &s.lists.seg, list_ends * 2 * PM_SEED_CAP));
          // (first half: the ends the fused seed kernel passes over; second half: what its second tier leaves of them)
          TRY (dev_alloc (d, &s.lists.big_list, 2 * (size_t) chunk_ends));
        }
      d->wk.lists_arrays = !pm_fused (d);
      d->wk.lists_cap = chunk_ends;
    }
  return 0;
}

// copy_evs (may be NULL): one event per chunk, recorded behind the host-to-device copy of that chunk's rows; the first stream
// that touches the rows waits for it
// (mu held: the form of plane 0 changes here)
static int run_slice (pemap_dev * d, int first, int n, int sync, const hipEvent_t * copy_evs = nullptr)
{
  HIPCHK (d, hipSetDevice (d->device));
  if (!d->ix.ready)
    return fail (d, "run: no index loaded");
  if (d->rd.n <= 0)
    return fail (d, "run: no reads staged");
  if (first < 0 || n <= 0 || first + n > d->rd.n)
    return fail (d, "run: slice [%d, %d) outside the %d staged reads", first, first + n, d->rd.n);
  if (d->rd.paired != d->paired)
    return fail (d, "run: reads were staged in %s mode", d->rd.paired ? "paired" : "single");
  const int L = d->rd.max_len;
  const int per = d->paired ? 2 : 1;
  const int chunk = chunk_pairs_for (d, n, L);
  const int nch = (n + chunk - 1) / chunk;
  // Asynchronous runs queue up behind each other: the chunks of this run continue the pipeline of the pending ones (same
  // sets, same event chain), so that look-ups of this run's first chunk overlap the previous run's last.  The pending runs
  // are absorbed first only when the per-chunk bookkeeping would overflow or the geometry changes.
  int k0 = 0;
  if (d->run.pending)
    {
      // (a smaller chunk than the pending runs' fits their arrays: the tail of a batch continues the pipeline too)
      const bool same = d->kn.pipeline == 1 && d->run.L == L && chunk * per <= d->wk.cap_ends
        && chunk * per <= d->wk.lists_cap && (size_t) (chunk * per) < d->wk.dir_slabs;
      if (same && d->run.chunks + nch <= PM_MAX_CHUNKS)
        k0 = d->run.chunks;
      else
        {
          // (why, for pemap_dev_pipeline_stats: the chunk table is full; the longest read changed; anything else of `same`)
          d->run.pstat[same ? PM_PS_ABSORB_TABLE_FULL : d->kn.pipeline == 1 && d->run.L != L ? PM_PS_ABSORB_LENGTH : PM_PS_ABSORB_ARRAYS]++;
          TRY (absorb_pending (d));
        }
    }
  d->run.pstat[PM_PS_RUNS]++;
  d->run.pstat[PM_PS_CONTINUED] += k0 > 0;
  d->run.pstat[PM_PS_LAST_CHUNKS] = (uint64_t) nch;
  d->run.pstat[PM_PS_LAST_FIRST_CHUNK] = (uint64_t) k0;
  TRY (ensure_work (d, chunk * per));
  TRY (ensure_pipeline (d, chunk * per));
  // PEMAP_PIPELINE=1 (default): the seed stage on stream2, PM_SETS chunks ahead of the ALU stream; 2: everything on the ALU stream.
  // The reference layout's vote runs on the ALU stream (it was slower beside its look-ups).  The fused layout's emit kernel
  // runs on the ALU stream for reads of up to 160 bases (where the seed kernel is the longer side: 29.8 ms per step against
  // 31.4; measured again behind the shorter second tier, profiles/r16_ab_sweeps.txt: 15.4 against 16.0 at 2 x 150, 16.0 against
  // 16.3 at 2 x 160, 11.1 against 11.3 at 2 x 100), behind the seed kernel for longer ones (2 x 245: 56.9 ms against 58.6).
  PmSchedule s;
  s.ahead = d->kn.pipeline == 1;
  s.seed = s.ahead ? d->run.stream2 : d->stream;
  s.emit_on_alu = s.ahead && pm_fused (d) && seg_template (L) <= 10;
  RunCtx c;
  c.ix = index_of (d);
  c.prm = params_of (d);
  c.L = L;
  c.tstride = tstride_for (d, L);
  // (the last slab of the allocation, whatever this run's chunk size: chunks of earlier, larger runs may still be in flight)
  c.dump_off = (d->wk.dir_slabs - 1) * slab_dwords_for (d, L);
  if (k0 == 0)
    {
      memset (&d->run.last_ctr, 0, sizeof (d->run.last_ctr));
      memset (d->run.last_ms, 0, sizeof (d->run.last_ms));
      d->run.last_big = d->run.last_big2 = 0;
      d->run.ends = 0;
    }
  // the first chunk that finds plane 0 holding counts has them turned into differences, ahead of its pile kernel on the ALU stream
  TRY (pile_unfold_locked (d));
  d->run.serial++;
  d->run.first = first;
  d->run.n = n;
  d->run.ends += (uint64_t) n * per;
  d->run.chunks = k0 + nch;
  d->run.L = L;
  // fresh per-chunk counters: zeroed on the stream that touches them first (the seed stream, so that a queued run's first
  // look-ups do not wait for the previous run's ALU work)
  HIPCHK (d, hipMemsetAsync (d->run.d_chunk_ctr + k0, 0, sizeof (PmChunkCtr) * nch, s.seed));
  auto batch_of = [&] (int k, PmBatch & bb, int &f, int &m)
  {
    const int off = k * chunk;
    m = (n - off < chunk) ? n - off : chunk;
    f = first + off;
    bb.reads1 = d->rd.d_rows[0] + (size_t) f * d->rd.stride;
    bb.reads2 = d->paired ? d->rd.d_rows[1] + (size_t) f * d->rd.stride : nullptr;
    bb.len1 = d->rd.d_len[0] + f;
    bb.len2 = d->paired ? d->rd.d_len[1] + f : nullptr;
    bb.n = m;
    bb.stride = d->rd.stride;
    bb.paired = d->paired;
    bb.n_ends = m * per;
  };
  auto enqueue_seed_k = [&] (int k) -> int
  {
    int f, m;
    RunCtx cl = c;
    batch_of (k, cl.b, f, m);
    return enqueue_seed (d, s, cl, k0 + k, copy_evs ? &copy_evs[k] : nullptr);
  };
  // seed stream order: seed(0) .. seed(PM_SETS-1), then per chunk k: seed(k+PM_SETS) behind the ALU stream's enqueue of chunk k
  if (s.ahead)
    for (int k = 0; k < PM_SETS && k < nch; k++)
      TRY (enqueue_seed_k (k));
  for (int k = 0; k < nch; k++)
    {
      int f, m;
      batch_of (k, c.b, f, m);
      const int g = k0 + k;
      PmChunkSet & S = d->wk.set[g % PM_SETS];
      PmChunkCtr *cc = d->run.d_chunk_ctr + g;
      hipEvent_t *ev = &d->run.evs[(size_t) g * PM_NEV];
      if (!s.ahead)
        TRY (enqueue_seed_k (k));
      HIPCHK (d, hipStreamWaitEvent (d->stream, S.ev_lists_ready, 0));
      uint32_t *m1 = d->rd.d_m1 + f, *m2 = d->paired ? d->rd.d_m2 + f : nullptr;
      int *mt = d->rd.d_mtype + f;
      with_sw_geom (d, L, [&] (auto w, auto lanes)
      {
        launch_chunk < w.value, lanes.value > (d, s, c, m1, m2, mt, S, cc, ev);
      });
      HIPCHK (d, hipGetLastError ());
      if (s.ahead && k + PM_SETS < nch)
        TRY (enqueue_seed_k (k + PM_SETS));
    }
  if (d->run.rest_twice)
    return fail (d, "internal: the seed-stage remainder of a chunk was enqueued twice");
  d->run.pending = true;
  if (sync)
    TRY (absorb_pending (d));
  return 0;
}

extern "C" int pemap_dev_run (pemap_dev * d, int sync)
{
  std::lock_guard < std::mutex > lk (d->mu);
  return run_slice (d, 0, d->rd.n, sync);
}

extern "C" int pemap_dev_run_slice (pemap_dev * d, int first, int n, int sync)
{
  std::lock_guard < std::mutex > lk (d->mu);
  return run_slice (d, first, n, sync);
}

extern "C" int pemap_dev_sync (pemap_dev * d)
{
  HIPCHK (d, hipSetDevice (d->device));
  TRY (absorb_pending (d));
  HIPCHK (d, hipStreamSynchronize (d->stream));
  return 0;
}

extern "C" int pemap_dev_collect (pemap_dev * d, uint32_t * m1, uint32_t * m2, int *mapping_type)
{
  TRY (pemap_dev_sync (d));
  const int n = d->run.n, first = d->run.first;
  if (n <= 0)
    return fail (d, "collect: nothing was run");
  HIPCHK (d, hipMemcpy (m1, d->rd.d_m1 + first, (size_t) n * sizeof (uint32_t), hipMemcpyDeviceToHost));
  if (d->paired && m2)
    HIPCHK (d, hipMemcpy (m2, d->rd.d_m2 + first, (size_t) n * sizeof (uint32_t), hipMemcpyDeviceToHost));
  HIPCHK (d, hipMemcpy (mapping_type, d->rd.d_mtype + first, (size_t) n * sizeof (int), hipMemcpyDeviceToHost));
  TRY (drain_ins (d));
  fold_summary (d, first, n, m1, m2, mapping_type);
  return 0;
}

// ---- batches in flight -------------------------------------------------------------------------------------
// The reference hands a filled batch to a worker thread and goes on reading (pthread_create at pemapper.c:684; the batch's
// mutex is released when the worker is done, 1307).  submit / wait are that seam: submit queues the batch's host-to-device
// copies (their own stream) and its kernels (the object's pipeline, continued from the batch before) and returns; wait blocks
// until the batch's m1 / m2 / mapping_type are in the caller's buffers.  With two or three batches in flight the copies of
// batch k + 1 and the results of batch k - 1 move while batch k is computed, and the pipeline never drains between calls.

// is [p, p + bytes) inside a range pinned by the caller?
bool pm_host_pin_lookup (const void *p, size_t bytes)
{
  std::lock_guard < std::mutex > lk (g_pin_mu);
  const char *c = (const char *) p;
  for (size_t i = 0; i < g_pinned.size (); i++)
    if (c >= g_pinned[i].base && c + bytes <= g_pinned[i].base + g_pinned[i].bytes)
      return true;
  return false;
}

// register a host range for DMA on behalf of pemap_dev_pin_host.  Registered ranges that share pages with the new one are
// replaced by the union of all of them (a copy must lie inside one registration); the calling object's copy stream is drained
// before a registration is dropped, copies out of it may be queued.
bool pm_host_pin_range (const void *p, size_t bytes, hipStream_t copy_stream)
{
  std::lock_guard < std::mutex > lk (g_pin_mu);
  const size_t page = 4096;
  char *lo = (char *) ((uintptr_t) p & ~(uintptr_t) (page - 1));
  char *hi = (char *) (((uintptr_t) p + bytes + page - 1) & ~(uintptr_t) (page - 1));
  int users = 1;
  for (size_t i = 0; i < g_pinned.size (); i++)
    if (lo >= g_pinned[i].base && hi <= g_pinned[i].base + g_pinned[i].bytes)
      {
        g_pinned[i].users++;
        return true;
      }
  for (size_t i = 0; i < g_pinned.size ();)
    if (lo < g_pinned[i].base + g_pinned[i].bytes && g_pinned[i].base < hi)
      {
        if (g_pinned[i].base < lo)
          lo = g_pinned[i].base;
        if (g_pinned[i].base + g_pinned[i].bytes > hi)
          hi = g_pinned[i].base + g_pinned[i].bytes;
        users += g_pinned[i].users;
        if (copy_stream)
          (void) hipStreamSynchronize (copy_stream);
        (void) hipHostUnregister (g_pinned[i].base);
        (void) hipGetLastError ();
        g_pinned.erase (g_pinned.begin () + i);
      }
    else
      i++;
  // (hipHostRegisterDefault is "mapped and portable" in HIP: the range serves the copies of every device's objects, not only the
  // registering one's)
  if (hipHostRegister (lo, (size_t) (hi - lo), hipHostRegisterDefault) != hipSuccess)
    {
      (void) hipGetLastError ();
      return false;
    }
  PmPinned e;
  e.base = lo;
  e.bytes = (size_t) (hi - lo);
  e.users = users;
  g_pinned.push_back (e);
  return true;
}

// host copy into a pinned staging buffer, on a few threads when it is large (one core moves ~10 GB/s: 330 MB per million pairs)
void pm_par_memcpy (char *dst, const char *src, size_t bytes)
{
  const size_t piece = (size_t) 4 << 20;
  if (bytes < 2 * piece)
    {
      memcpy (dst, src, bytes);
      return;
    }
  const int nt = 4;
  std::thread th[nt];
  const size_t per = ((bytes / nt) + 63) & ~(size_t) 63;
  for (int t = 0; t < nt; t++)
    {
      const size_t o = per * t, m = o >= bytes ? 0 : (bytes - o < per ? bytes - o : per);
      th[t] = std::thread ([=] { if (m) memcpy (dst + o, src + o, m); });
    }
  for (int t = 0; t < nt; t++)
    th[t].join ();
}

extern "C" int pemap_dev_pin_host (pemap_dev * d, const void *host_ptr, uint64_t n_bytes)
{
  HIPCHK (d, hipSetDevice (d->device));
  if (!host_ptr || !n_bytes)
    return fail (d, "pin_host: empty range");
  if (!pm_host_pin_range (host_ptr, (size_t) n_bytes, d->rg.stream_h2d))
    return fail (d, "pin_host: hipHostRegister of %llu bytes failed", (unsigned long long) n_bytes);
  return 0;
}

// undo one pm_host_pin_range of the range that holds host_ptr: 0 done, 1 not a pinned range, 2 the runtime refused
int pm_host_unpin (const void *host_ptr)
{
  std::lock_guard < std::mutex > lk (g_pin_mu);
  const char *c = (const char *) host_ptr;
  for (size_t i = 0; i < g_pinned.size (); i++)
    if (c >= g_pinned[i].base && c < g_pinned[i].base + g_pinned[i].bytes && g_pinned[i].users > 0)
      {
        if (--g_pinned[i].users == 0)
          {
            const hipError_t e = hipHostUnregister (g_pinned[i].base);
            g_pinned.erase (g_pinned.begin () + i);
            if (e != hipSuccess)
              return 2;
          }
        return 0;
      }
  return 1;
}

extern "C" int pemap_dev_unpin_host (pemap_dev * d, const void *host_ptr)
{
  HIPCHK (d, hipSetDevice (d->device));
  // copies out of the range may still be queued on this object's copy stream
  {
    std::lock_guard < std::mutex > lk (d->mu);
    if (d->rg.stream_h2d)
      HIPCHK (d, hipStreamSynchronize (d->rg.stream_h2d));
  }
  const int rc = pm_host_unpin (host_ptr);
  if (rc == 1)
    return fail (d, "unpin_host: %p is not inside a range pinned through pemap_dev_pin_host", host_ptr);
  if (rc == 2)
    return fail (d, "unpin_host: hipHostUnregister failed");
  return 0;
}

// wait for the batch in `slot` and deliver it (mu held through lk; released while the host blocks on the event)
static int ring_finish (pemap_dev * d, int slot, std::unique_lock < std::mutex > &lk)
{
  PmRingSlot & r = d->rg.slot[slot];
  if (!r.active)
    return 0;
  const unsigned long long seq = r.seq;
  hipEvent_t ev = r.ev_done;
  lk.unlock ();
  hipError_t e = hipEventSynchronize (ev);
  lk.lock ();
  if (e != hipSuccess)
    return fail (d, "wait_batch: %s", hipGetErrorString (e));
  if (!r.active || r.seq != seq)
    return 0;                   // another thread delivered it meanwhile
  const int n = r.n;
  memcpy (r.m1, r.h_res, (size_t) n * 4);
  if (d->paired && r.m2)
    memcpy (r.m2, r.h_res + d->rg.cap, (size_t) n * 4);
  memcpy (r.mt, r.h_res + 2 * (size_t) d->rg.cap, (size_t) n * 4);
  fold_summary (d, r.first, n, r.m1, r.m2, r.mt);
  r.active = false;
  return 0;
}

static int ring_finish_all (pemap_dev * d, std::unique_lock < std::mutex > &lk)
{
  // oldest first, so that the summary folds in submission order
  for (;;)
    {
      int pick = -1;
      for (int i = 0; i < PM_RING; i++)
        if (d->rg.slot[i].active && (pick < 0 || d->rg.slot[i].seq < d->rg.slot[pick].seq))
          pick = i;
      if (pick < 0)
        return 0;
      TRY (ring_finish (d, pick, lk));
    }
}

// the staged arrays go back to holding one resident read set, of n rows at `stride` (stage_reads, stage_fastq, synth_reads): the
// batches in flight are delivered, the pending run is accounted, the arrays are there
static int ring_leave (pemap_dev * d, int n, int stride, int paired)
{
  {
    std::unique_lock < std::mutex > sub (d->submit_mu);
    std::unique_lock < std::mutex > lk (d->mu);
    TRY (ring_finish_all (d, lk));
    d->rg.cap = 0;
  }
  TRY (pemap_dev_sync (d));
  return ensure_reads (d, n, stride, paired);
}

static int ring_setup (pemap_dev * d, int n, int stride, std::unique_lock < std::mutex > &lk)
{
  if (!d->rg.stream_h2d)
    HIPCHK (d, hipStreamCreateWithFlags (&d->rg.stream_h2d, hipStreamNonBlocking));
  if (d->rg.cap >= n && d->rd.stride == stride && d->rd.paired == d->paired && (!d->paired || d->rd.d_rows[1]))
    return 0;
  // a different geometry: everything in flight is delivered and accounted first
  d->run.pstat[PM_PS_RING_SETUPS]++;
  TRY (ring_finish_all (d, lk));
  TRY (absorb_pending (d));
  HIPCHK (d, hipDeviceSynchronize ());
  int cap = n > d->rg.cap ? n : d->rg.cap;
  if (cap < 1024)
    cap = 1024;
  if ((long) cap * PM_RING > 2000000000L)
    return fail (d, "submit_batch: %d reads per batch are too many", n);
  // (from here to its last block the ring is not set up: rg.cap is 0, and a submit after a failure comes through here again)
  ring_free (d->rg, true);
  TRY (ensure_reads (d, cap * PM_RING, stride, d->paired));
  for (PmRingSlot & r : d->rg.slot)
    {
      HIPCHK (d, hipHostMalloc ((void **) &r.h_len, (size_t) cap * 2 * sizeof (int), hipHostMallocDefault));
      HIPCHK (d, hipHostMalloc ((void **) &r.h_res, (size_t) cap * 3 * sizeof (uint32_t), hipHostMallocDefault));
      if (!r.ev_done)
        HIPCHK (d, hipEventCreateWithFlags (&r.ev_done, hipEventDisableTiming));
    }
  d->rg.cap = cap;
  reads_staged (d, cap * PM_RING, d->paired, 0, 1 << 30);
  d->rd.h_len[0].assign ((size_t) cap * PM_RING, 0);
  d->rd.h_len[1].assign (d->paired ? (size_t) cap * PM_RING : 0, 0);
  return 0;
}

// ---- what the two submits share.  A batch of n rows at `stride` gets the slot of this submission (mu and submit_mu held): the ring
// set up for it, the batch that used the slot PM_RING submissions ago delivered; `first` is the slot's first row in the staged arrays.
struct PmSlotTake
{
  PmRingSlot *r;
  int first;
  uint8_t *rows[2];             // per mate: the slot's device rows and lengths, its pinned staging of the lengths
  int *lens[2], *h_len[2];
};

static int ring_take (pemap_dev * d, int n, int stride, std::unique_lock < std::mutex > &lk, PmSlotTake & t)
{
  TRY (ring_setup (d, n, stride, lk));
  const int slot = (int) (d->rg.seq % PM_RING);
  TRY (ring_finish (d, slot, lk));
  t.r = &d->rg.slot[slot];
  t.first = slot * d->rg.cap;
  for (int m = 0; m < 2; m++)
    {
      t.rows[m] = d->rd.d_rows[m] + (size_t) t.first * stride;
      t.lens[m] = d->rd.d_len[m] + t.first;
      t.h_len[m] = t.r->h_len + (size_t) m * d->rg.cap;
    }
  return 0;
}

// The batch's lengths (mn..mx) in: the kernels' geometry follows the longest read seen since the ring was set up (any upper bound gives
// the same results; a bound that never shrinks keeps consecutive batches in one pipeline).  Then the pipeline's streams, which must exist
// before the first copy event is waited on, and one copy event per slice of the batch, the slices cut like the kernels' chunks (chunk
// k's look-ups wait for r.ev_copy[k]).  *slice receives the slice's size in rows.
static int ring_slices (pemap_dev * d, PmRingSlot & r, int n, int mx, int mn, int *slice)
{
  if (mx > d->rd.max_len)
    d->rd.max_len = mx;
  if (mn < d->rd.min_len)
    d->rd.min_len = mn;
  if (!d->run.stream2)
    TRY (ensure_pipeline (d, 0));
  *slice = chunk_pairs_for (d, n, d->rd.max_len);
  const int n_slices = (n + *slice - 1) / *slice;
  while ((int) r.ev_copy.size () < n_slices)
    {
      hipEvent_t e;
      HIPCHK (d, hipEventCreateWithFlags (&e, hipEventDisableTiming));
      r.ev_copy.push_back (e);
    }
  return 0;
}

// the end of a submit: the batch's rows and lengths are on their way into slot r (r.ev_copy recorded behind them, one per slice of
// chunk_pairs_for); its kernels, the copy of its results, and the slot becomes a batch in flight
static int ring_queue_run (pemap_dev * d, PmRingSlot & r, int first, int n, uint32_t * m1, uint32_t * m2, int *mapping_type, uint64_t * ticket)
{
  TRY (run_slice (d, first, n, 0, r.ev_copy.data ()));
  // results: on the ALU stream itself, behind the batch's last kernel (every other stream's work for the batch precedes it).
  // Not on a stream of their own: HIP multiplexes streams onto a few hardware queues, and a copy stream parked on "batch k is
  // done" held up whichever pipeline stream shared its queue -- 3.5 ms per batch (measured: 45.2 ms per step against 41.7).
  hipStream_t rs = d->stream;
  HIPCHK (d, hipMemcpyAsync (r.h_res, d->rd.d_m1 + first, (size_t) n * 4, hipMemcpyDeviceToHost, rs));
  if (d->paired)
    HIPCHK (d, hipMemcpyAsync (r.h_res + d->rg.cap, d->rd.d_m2 + first, (size_t) n * 4, hipMemcpyDeviceToHost, rs));
  HIPCHK (d, hipMemcpyAsync (r.h_res + 2 * (size_t) d->rg.cap, d->rd.d_mtype + first, (size_t) n * 4, hipMemcpyDeviceToHost, rs));
  HIPCHK (d, hipEventRecord (r.ev_done, rs));
  // the slot becomes a batch in flight only now that its event is recorded: an error above leaves it free, and nothing stale is
  // ever "delivered" into the caller's buffers or folded into the summary
  r.active = true;
  r.seq = d->rg.seq;
  r.n = n;
  r.first = first;
  r.m1 = m1;
  r.m2 = m2;
  r.mt = mapping_type;
  *ticket = d->rg.seq++;
  return 0;
}

static bool ring_busy (pemap_dev * d)
{
  std::lock_guard < std::mutex > lk (d->mu);
  return ring_active (d->rg);
}

// The parameters are read again when a batch is delivered (ring_finish: m2 is copied in paired mode; fold_summary: the second end's
// length, the distance cut-off), and ring_setup delivers what is in flight when the pairing changed.  So a change first delivers
// every batch in flight and absorbs the pending run, under the values they were submitted with; a call that changes nothing is free.
extern "C" int pemap_dev_set_params (pemap_dev * d, int paired, int min_dist, int max_dist, double min_align, int bisulfite)
{
  std::unique_lock < std::mutex > sub (d->submit_mu);   // (the order of ring_leave: no submit slips in while mu is dropped in ring_finish)
  std::unique_lock < std::mutex > lk (d->mu);
  paired = paired ? 1 : 0;
  bisulfite = bisulfite ? 1 : 0;
  if (d->paired == paired && d->min_dist == min_dist && d->max_dist == max_dist && d->min_align == min_align && d->bisulfite == bisulfite)
    return 0;
  if (d->run.pending || ring_active (d->rg))
    {
      HIPCHK (d, hipSetDevice (d->device));
      TRY (ring_finish_all (d, lk));
      TRY (absorb_pending (d));
    }
  d->paired = paired;
  d->min_dist = min_dist;
  d->max_dist = max_dist;
  d->min_align = min_align;
  d->bisulfite = bisulfite;
  return 0;
}

// what stage_reads and submit_batch ask of the caller's n rows; the longest and the shortest read
static int check_rows (pemap_dev * d, const char *who, const int *len1, const int *len2, int n, int stride, int *mx, int *mn)
{
  if (stride < PEMAP_MIN_READ)
    return fail (d, "%s: stride %d", who, stride);
  *mx = 0;
  *mn = 1 << 30;
  TRY (check_lengths (d, len1, n, mx, mn));
  if (d->paired)
    TRY (check_lengths (d, len2, n, mx, mn));
  if (*mx > stride)
    return fail (d, "%s: a read is longer than the row stride %d", who, stride);
  return 0;
}

extern "C" int pemap_dev_stage_reads (pemap_dev * d, const char *reads1, const int *len1, const char *reads2, const int *len2,
                                      int n, int stride)
{
  HIPCHK (d, hipSetDevice (d->device));
  if (n <= 0)
    return fail (d, "stage_reads: n = %d", n);
  if (d->paired && (!reads2 || !len2))
    return fail (d, "stage_reads: paired mode needs reads2/len2");
  int mx, mn;
  TRY (check_rows (d, "stage_reads", len1, len2, n, stride, &mx, &mn));
  TRY (ring_leave (d, n, stride, d->paired));
  const char *const rows[2] = { reads1, reads2 };
  const int *const lens[2] = { len1, len2 };
  d->rd.h_len[1].clear ();
  for (int m = 0; m < (d->paired ? 2 : 1); m++)
    {
      HIPCHK (d, hipMemcpy (d->rd.d_rows[m], rows[m], (size_t) n * stride, hipMemcpyHostToDevice));
      HIPCHK (d, hipMemcpy (d->rd.d_len[m], lens[m], (size_t) n * sizeof (int), hipMemcpyHostToDevice));
      d->rd.h_len[m].assign (lens[m], lens[m] + n);
    }
  reads_staged (d, n, d->paired, mx, mn);
  return 0;
}

extern "C" int pemap_dev_submit_batch (pemap_dev * d, const char *reads1, const int *len1, const char *reads2, const int *len2,
                                       int n, int stride, uint32_t * m1, uint32_t * m2, int *mapping_type, uint64_t * ticket)
{
  std::unique_lock < std::mutex > sub (d->submit_mu);   // rg.seq, the slot and `first` below stay this call's own while mu is dropped
  std::unique_lock < std::mutex > lk (d->mu);
  HIPCHK (d, hipSetDevice (d->device));
  if (!d->ix.ready)
    return fail (d, "submit_batch: no index loaded");
  if (n <= 0)
    return fail (d, "submit_batch: n = %d", n);
  if (!reads1 || !len1 || !m1 || !mapping_type || !ticket)
    return fail (d, "submit_batch: a required pointer is NULL");
  if (d->paired && (!reads2 || !len2 || !m2))
    return fail (d, "submit_batch: paired mode needs reads2 / len2 / m2");
  int mx, mn;
  TRY (check_rows (d, "submit_batch", len1, len2, n, stride, &mx, &mn));
  PmSlotTake t;
  TRY (ring_take (d, n, stride, lk, t));
  PmRingSlot & r = *t.r;
  const int first = t.first, mates = d->paired ? 2 : 1;
  const char *const rows[2] = { reads1, reads2 };
  const int *const lens[2] = { len1, len2 };
  for (int m = 0; m < mates; m++)
    {
      memcpy (&d->rd.h_len[m][first], lens[m], (size_t) n * sizeof (int));
      memcpy (t.h_len[m], lens[m], (size_t) n * sizeof (int));
      HIPCHK (d, hipMemcpyAsync (t.lens[m], t.h_len[m], (size_t) n * sizeof (int), hipMemcpyHostToDevice, d->rg.stream_h2d));
    }
  // the rows move by DMA straight out of the caller's buffers when the caller pinned them (pemap_dev_pin_host); otherwise they
  // are copied, slice by slice, into the slot's pinned staging buffer first (the DMA of slice k runs beside the host copy of k + 1)
  bool direct[2] = { true, true };
  for (int m = 0; m < mates; m++)
    direct[m] = pm_host_pin_lookup (rows[m], (size_t) n * stride);
  const size_t need = (size_t) d->rg.cap * stride * 2;
  if ((!direct[0] || !direct[1]) && r.h_rows_bytes < need)
    {
      pm_host_free (r.h_rows);
      r.h_rows_bytes = 0;
      HIPCHK (d, hipHostMalloc ((void **) &r.h_rows, need, hipHostMallocDefault));
      r.h_rows_bytes = need;
    }
  int slice;
  TRY (ring_slices (d, r, n, mx, mn, &slice));
  for (int k = 0, off = 0; off < n; off += slice, k++)
    {
      const int cnt = n - off < slice ? n - off : slice;
      for (int m = 0; m < mates; m++)
        {
          const char *src = rows[m] + (size_t) off * stride;
          if (!direct[m])
            {
              char *stg = r.h_rows + ((size_t) m * d->rg.cap + off) * stride;
              pm_par_memcpy (stg, src, (size_t) cnt * stride);
              src = stg;
            }
          HIPCHK (d, hipMemcpyAsync (t.rows[m] + (size_t) off * stride, src, (size_t) cnt * stride, hipMemcpyHostToDevice, d->rg.stream_h2d));
        }
      HIPCHK (d, hipEventRecord (r.ev_copy[k], d->rg.stream_h2d));
    }
  return ring_queue_run (d, r, first, n, m1, m2, mapping_type, ticket);
}

extern "C" int pemap_dev_wait_batch (pemap_dev * d, uint64_t ticket)
{
  std::unique_lock < std::mutex > lk (d->mu);
  HIPCHK (d, hipSetDevice (d->device));
  if (ticket >= d->rg.seq)
    return fail (d, "wait_batch: ticket %llu was never handed out", (unsigned long long) ticket);
  const int slot = (int) (ticket % PM_RING);
  if (!d->rg.slot[slot].active || d->rg.slot[slot].seq != ticket)
    return 0;                   // delivered already (by a later submit that needed the slot, or by another wait)
  return ring_finish (d, slot, lk);
}

extern "C" int pemap_dev_map_batch (pemap_dev * d, const char *reads1, const int *len1, const char *reads2, const int *len2,
                                    int n, int stride, uint32_t * m1, uint32_t * m2, int *mapping_type)
{
  // submit + wait.  Called from one thread this fills and drains the pipeline once per call; several host threads calling it
  // on the same object (the reference's worker threads, one batch each) overlap like explicit submit / wait pairs do.
  uint64_t t = 0;
  TRY (pemap_dev_submit_batch (d, reads1, len1, reads2, len2, n, stride, m1, m2, mapping_type, &t));
  TRY (pemap_dev_wait_batch (d, t));
  std::unique_lock < std::mutex > lk (d->mu);
  // nothing else in flight: account the run now (counters, kernel times, insertion log), so that run_stats describes this call
  if (!ring_active (d->rg))
    TRY (absorb_pending (d));
  // the one-call entry hands the counters back as counts: a view of buffer 4 taken before the call is read after it.  (With other
  // threads' batches still in flight the fold queues behind them, and their next chunk unfolds again.)
  return pile_fold_locked (d);
}

extern "C" int pemap_dev_summary (pemap_dev * d, long *out13)
{
  memcpy (out13, d->pile.summary, sizeof (d->pile.summary));
  return 0;
}

// host integers only: no synchronisation, nothing absorbed, no device call (pemap_dev_run_stats would absorb the pending run)
extern "C" int pemap_dev_pipeline_stats (pemap_dev * d, uint64_t * out8)
{
  if (!out8)
    return fail (d, "pipeline_stats: out8 must not be NULL");
  std::lock_guard < std::mutex > lk (d->mu);
  memcpy (out8, d->run.pstat, sizeof (d->run.pstat));
  return 0;
}

extern "C" int pemap_dev_run_stats (pemap_dev * d, uint64_t * s, float *t)
{
  TRY (pemap_dev_sync (d));     // a run still in flight is accounted first
  const PmCounters & c = d->run.last_ctr;
  if (s)
    {
      s[0] = d->run.ends;
      s[1] = c.positions;
      s[2] = (uint64_t) c.n_tasks_s + c.n_tasks_m;
      s[3] = (uint64_t) c.n_tasks_dp + c.n_band[0] + c.n_redo;
      s[4] = c.cells_score;
      s[5] = c.cells_dirs;
      s[6] = c.pile_incs;
      s[7] = c.n_ins;
      s[8] = c.n_wins;
      s[9] = c.n_redo;
      s[10] = d->run.last_big;
      s[11] = (uint64_t) d->run.chunks;
      s[12] = ((uint64_t) c.n_tasks_s - c.n_tasks_dp - c.n_band[0]) + ((uint64_t) c.n_tasks_m - c.n_tasks_mdp - c.n_band[1]);
      s[13] = (uint64_t) c.n_band[0] + c.n_band[1];
      s[14] = c.cells_band;
      s[15] = d->run.last_big2;
      s[16] = c.n_walks;
      s[17] = (uint64_t) c.n_gate[0] + c.n_gate[1];
    }
  if (t)
    memcpy (t, d->run.last_ms, sizeof (d->run.last_ms));
  return 0;
}

extern "C" int pemap_dev_seed_launch (pemap_dev * d, int *asked, int *resident, int *launched, int *lds_bytes)
{
  *asked = d->run.seed_launch[0];
  *resident = d->run.seed_launch[1];
  *launched = d->run.seed_launch[2];
  *lds_bytes = d->run.seed_launch[3];
  return 0;
}

extern "C" int pemap_dev_sw_grid (pemap_dev * d)
{
  return d->wk.sw_grid;
}

// The hit records of the last run's first chunk (set 0): meaningful for a run of one chunk only.
extern "C" int pemap_dev_debug_hits (pemap_dev * d, int *n_hits, uint32_t * spot, uint8_t * orient, uint32_t * win_start,
                                     int *win_len, double *score, int *start_k, int *start_i)
{
  HIPCHK (d, hipSetDevice (d->device));
  HIPCHK (d, hipStreamSynchronize (d->stream));
  const int n_ends = d->paired ? 2 * d->run.n : d->run.n;
  const size_t nh = (size_t) n_ends * PM_MAX_HITS;
  const PmHits & H = d->wk.set[0].hits;
  if (n_hits)
    HIPCHK (d, hipMemcpy (n_hits, H.n_hits, (size_t) n_ends * sizeof (int), hipMemcpyDeviceToHost));
  if (spot)
    HIPCHK (d, hipMemcpy (spot, H.spot, nh * 4, hipMemcpyDeviceToHost));
  if (orient)
    HIPCHK (d, hipMemcpy (orient, H.orient, nh, hipMemcpyDeviceToHost));
  if (win_start)
    HIPCHK (d, hipMemcpy (win_start, H.gpos, nh * 4, hipMemcpyDeviceToHost));
  if (score)
    HIPCHK (d, hipMemcpy (score, H.score, nh * 8, hipMemcpyDeviceToHost));
  // the narrow arrays widened to the caller's ints
  auto widened = [&] (int *out, const auto * dev, int mask) -> int
  {
    std::vector < std::decay_t < decltype (*dev) > > t (out ? nh : 0);
    if (out)
      HIPCHK (d, hipMemcpy (t.data (), dev, nh * sizeof (t[0]), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < t.size (); i++)
      out[i] = t[i] & mask;
    return 0;
  };
  TRY (widened (win_len, H.nn, -1));
  TRY (widened (start_i, H.sti, -1));
  return widened (start_k, H.stk, 3);   // (bit 2 = decided by the gapless rule)
}

// ------------------------------------------------------------------------------------------------------------
extern "C" int pemap_dev_reset_pileup (pemap_dev * d)
{
  HIPCHK (d, hipSetDevice (d->device));
  if (!d->pile.d_counts)
    return fail (d, "reset_pileup: no index");
  // (a batch delivered after the reset would be folded into the new totals: the rule of pemap_dev_absorb)
  if (ring_busy (d))
    return fail (d, "reset_pileup: the object has a submitted batch that was not waited for");
  HIPCHK (d, hipStreamSynchronize (d->stream));
  TRY (zero_on_stream (d, d->pile.d_counts, 6 * d->pile.plane_words * sizeof (uint32_t)));
  {
    // a plane of zeros is one in both forms: no conversion, whichever form it had
    std::lock_guard < std::mutex > lk (d->mu);
    d->pile.diff = false;
  }
  TRY (zero_on_stream (d, d->pile.d_cur, sizeof (PmInsCursor)));
  d->pile.h_ins.clear ();
  memset (d->pile.summary, 0, sizeof (d->pile.summary));
  return 0;
}

// ---- several objects in one process: the index handed on, the pileups summed -----------------------------------------------
// dst receives a copy of src's committed index: index_alloc with src's sizes, the four arrays device to device on dst's stream,
// index_commit (dst builds its look-up replicas, or not, by its own setting).  src is only read.
extern "C" int pemap_dev_index_share (pemap_dev * dst, pemap_dev * src)
{
  if (!dst || !src || dst == src)
    return fail (dst, "index_share: the source and the destination are the same object");
  if (!src->ix.ready)
    return fail (dst, "index_share: the source object has no committed index");
  TRY (pemap_dev_index_alloc (dst, src->ix.n_mers, src->ix.gsize, src->ix.n_contigs, src->ix.idepth));
  const size_t piece = (size_t) 1 << 30;
  for (int which = 0; which < 4; which++)
    {
      void *to = nullptr, *from = nullptr;
      uint64_t nb = 0, nb_src = 0;
      TRY (pemap_dev_buffer (dst, which, &to, &nb));
      if (pemap_dev_buffer (src, which, &from, &nb_src) || nb_src != nb)
        return fail (dst, "index_share: buffer %d of the source does not match", which);
      // (hipMemcpyPeerAsync needs no peer access enabled, and is a plain device copy when both objects sit on one GPU)
      for (uint64_t o = 0; o < nb; o += piece)
        HIPCHK (dst, hipMemcpyPeerAsync ((char *) to + o, dst->device, (const char *) from + o, src->device, nb - o < piece ? nb - o : piece, dst->stream));
    }
  HIPCHK (dst, hipStreamSynchronize (dst->stream));
  return pemap_dev_index_commit (dst);
}

// the staged way's temporaries (on dst's device), released on every return
struct PmAbsorbStage
{
  uint32_t *buf[2] = {};
  hipStream_t copy = nullptr;
  hipEvent_t ev_copied[2] = {}, ev_added[2] = {};
  ~PmAbsorbStage ()
  {
    pm_free (buf[0], buf[1]);
    for (hipEvent_t * e : { &ev_copied[0], &ev_copied[1], &ev_added[0], &ev_added[1] })
      pm_event_free (*e);
    if (copy)
      hipStreamDestroy (copy);
  }
};

static void launch_pile_add (pemap_dev * d, uint32_t * to, const uint32_t * from, size_t bytes)
{
  const uint64_t n_vec = bytes / 16;
  uint64_t grid = (n_vec + PA_BLOCK - 1) / PA_BLOCK;
  if (grid > (uint64_t) d->n_cus * 8)
    grid = (uint64_t) d->n_cus * 8;
  hipLaunchKernelGGL (pm_pile_add_kernel, dim3 ((unsigned) grid), dim3 (PA_BLOCK), 0, d->stream, (uint4 *) to, (const uint4 *) from, n_vec);
}

// Afterwards dst is what it would be had it mapped src's batches as well, and src is as after pemap_dev_reset_pileup.
extern "C" int pemap_dev_absorb (pemap_dev * dst, pemap_dev * src)
{
  if (!dst || !src || dst == src)
    return fail (dst, "absorb: the source and the destination are the same object");
  if (!dst->ix.ready || !src->ix.ready)
    return fail (dst, "absorb: %s object has no index", dst->ix.ready ? "the source" : "the destination");
  if (dst->ix.gsize != src->ix.gsize || dst->ix.n_contigs != src->ix.n_contigs || dst->pile.plane_words != src->pile.plane_words)
    return fail (dst, "absorb: the objects hold different genomes (%llu letters in %d contigs against %llu in %d)", (unsigned long long) dst->ix.gsize,
                 dst->ix.n_contigs, (unsigned long long) src->ix.gsize, src->ix.n_contigs);
  if (ring_busy (dst) || ring_busy (src))
    return fail (dst, "absorb: %s object has a submitted batch that was not waited for", ring_busy (dst) ? "the destination" : "the source");
  if (pemap_dev_sync (src) || (hipSetDevice (src->device) != hipSuccess) || drain_ins (src))
    return fail (dst, "absorb: the source object: %.400s", src->err);
  if (pile_fold (src))
    return fail (dst, "absorb: the source object: %.400s", src->err);
  TRY (pemap_dev_sync (dst));   // (leaves dst's device current)
  TRY (pile_fold (dst));
  // ---- counters: every 16-bit counter of the planes becomes (dst + src) mod 2^16, padding included
  const size_t bytes = 6 * dst->pile.plane_words * sizeof (uint32_t);
  // (a plane is a whole number of 256-byte blocks, index_alloc: whole 16-byte vectors, no tail)
  if (dst->pile.plane_words % 64 != 0)
    return fail (dst, "internal: a pileup plane of %zu words is not a whole number of 256-byte blocks", dst->pile.plane_words);
  if (dst->device == src->device && !dst->kn.absorb_staged)
    launch_pile_add (dst, dst->pile.d_counts, src->pile.d_counts, bytes);
  else
    {
      // two staging buffers on dst's device: the copy of piece k + 1 runs under the add of piece k
      PmAbsorbStage S;
      const size_t chunk = dst->kn.absorb_chunk < bytes ? dst->kn.absorb_chunk : bytes;
      HIPCHK (dst, hipStreamCreateWithFlags (&S.copy, hipStreamNonBlocking));
      for (int b = 0; b < 2; b++)
        {
          HIPCHK (dst, hipMalloc ((void **) &S.buf[b], chunk));
          HIPCHK (dst, hipEventCreateWithFlags (&S.ev_copied[b], hipEventDisableTiming));
          HIPCHK (dst, hipEventCreateWithFlags (&S.ev_added[b], hipEventDisableTiming));
        }
      size_t k = 0;
      for (size_t o = 0; o < bytes; o += chunk, k++)
        {
          const int b = (int) (k & 1);
          const size_t m = bytes - o < chunk ? bytes - o : chunk;
          if (k >= 2)
            HIPCHK (dst, hipStreamWaitEvent (S.copy, S.ev_added[b], 0));        // the add of piece k - 2 has read the buffer
          HIPCHK (dst, hipMemcpyPeerAsync (S.buf[b], dst->device, (const char *) src->pile.d_counts + o, src->device, m, S.copy));
          HIPCHK (dst, hipEventRecord (S.ev_copied[b], S.copy));
          HIPCHK (dst, hipStreamWaitEvent (dst->stream, S.ev_copied[b], 0));
          launch_pile_add (dst, dst->pile.d_counts + o / sizeof (uint32_t), S.buf[b], m);
          HIPCHK (dst, hipEventRecord (S.ev_added[b], dst->stream));
        }
      HIPCHK (dst, hipStreamSynchronize (S.copy));
      HIPCHK (dst, hipStreamSynchronize (dst->stream));
    }
  HIPCHK (dst, hipStreamSynchronize (dst->stream));
  HIPCHK (dst, hipGetLastError ());
  // ---- insertion log (drained above) and summary
  dst->pile.h_ins.insert (dst->pile.h_ins.end (), src->pile.h_ins.begin (), src->pile.h_ins.end ());
  for (int i = 0; i < 13; i++)
    dst->pile.summary[i] += src->pile.summary[i];
  if (pemap_dev_reset_pileup (src))
    return fail (dst, "absorb: the source object: %.400s", src->err);
  return 0;
}

extern "C" int pemap_dev_fetch_pileup (pemap_dev * d, uint16_t * counts, pemap_ins_cb cb, void *user)
{
  HIPCHK (d, hipSetDevice (d->device));
  if (!d->pile.d_counts)
    return fail (d, "fetch_pileup: no index");
  TRY (pemap_dev_sync (d));
  TRY (pile_fold (d));
  TRY (drain_ins (d));
  if (counts)
    {
      const uint64_t chunk = 48ull << 20;       // positions per round (6 counters each)
      DevTmp < uint16_t > d_tmp;
      TRY (dev_alloc (d, &d_tmp.p, (size_t) (d->ix.gsize < chunk ? d->ix.gsize : chunk) * 6));
      for (uint64_t o = 0; o < d->ix.gsize; o += chunk)
        {
          const uint64_t m = d->ix.gsize - o < chunk ? d->ix.gsize - o : chunk;
          hipLaunchKernelGGL (pile_to_u16_kernel, dim3 ((unsigned) ((m * 6 + 255) / 256)), dim3 (256), 0, d->stream, pile_of (d), o, m, d_tmp);
          HIPCHK (d, hipStreamSynchronize (d->stream));
          HIPCHK (d, hipMemcpy (counts + o * 6, d_tmp, m * 6 * sizeof (uint16_t), hipMemcpyDeviceToHost));
        }
    }
  if (cb)
    {
      size_t at = 0;
      const std::vector < uint8_t > &L = d->pile.h_ins;
      char buf[512];
      while (at + 8 <= L.size ())
        {
          uint32_t pos, len;
          memcpy (&pos, &L[at], 4);
          memcpy (&len, &L[at + 4], 4);
          if (len == 0 || len > 300 || at + 8 + len > L.size ())
            return fail (d, "fetch_pileup: corrupt insertion log at byte %zu", at);
          memcpy (buf, &L[at + 8], len);
          buf[len] = 0;
          cb (user, pos, buf, (int) len);
          at += 8 + ((len + 3u) & ~3u);
        }
    }
  return 0;
}

// What pemap_dev_fetch_records and pemap_dev_fetch_records_gz begin with: the checks of the range, the fold of plane 0, the sites' counts
// per tile of PR_BLOCK positions and their scan.  `who` names the entry in the messages.  *total = 0 and no arrays for a range of no
// positions; else d_to holds the tiles' first records.  ev2 (may be NULL): two events, recorded around the two kernels.
static int pile_count_range (pemap_dev * d, const char *who, uint64_t first, uint64_t count, DevTmp < uint64_t > &d_to, uint64_t * total, hipEvent_t * ev2)
{
  HIPCHK (d, hipSetDevice (d->device));
  *total = 0;
  if (!d->pile.d_counts)
    return fail (d, "%s: no index", who);
  if (first + count > d->ix.gsize || first + count < first)
    return fail (d, "%s: range beyond the genome", who);
  if (count == 0)
    return 0;
  if (count > (1ull << 31))
    return fail (d, "%s: at most 2^31 sites per call", who);
  TRY (pile_fold (d));          // (on the ALU stream, behind everything queued, and waited for)
  HIPCHK (d, hipStreamSynchronize (d->stream));
  const uint64_t n_tiles = (count + PR_BLOCK - 1) / PR_BLOCK;
  DevTmp < uint64_t > d_total;
  DevTmp < uint32_t > d_tc;
  TRY (dev_alloc (d, &d_tc.p, n_tiles));
  TRY (dev_alloc (d, &d_to.p, n_tiles));
  TRY (dev_alloc (d, &d_total.p, 1));
  if (ev2)
    HIPCHK (d, hipEventRecord (ev2[0], d->stream));
  hipLaunchKernelGGL (pile_count_kernel, dim3 ((unsigned) n_tiles), dim3 (PR_BLOCK), 0, d->stream, pile_of (d), first, count, d_tc);
  hipLaunchKernelGGL (ix_scan_tiles_kernel, dim3 (1), dim3 (1024), 0, d->stream, d_tc, d_to, n_tiles, d_total);
  if (ev2)
    HIPCHK (d, hipEventRecord (ev2[1], d->stream));
  HIPCHK (d, hipMemcpyAsync (total, d_total, 8, hipMemcpyDeviceToHost, d->stream));
  HIPCHK (d, hipStreamSynchronize (d->stream));
  return 0;
}

extern "C" int pemap_dev_fetch_records (pemap_dev * d, uint64_t first, uint64_t count, void *out, uint64_t out_capacity,
                                        uint64_t * n_records)
{
  DevTmp < uint64_t > d_to;
  uint64_t total = 0;
  TRY (pile_count_range (d, "fetch_records", first, count, d_to, &total, nullptr));
  *n_records = total;
  if (!out || !total)
    return 0;
  if (total > out_capacity)
    return fail (d, "fetch_records: %llu records do not fit the caller's %llu", (unsigned long long) total,
                 (unsigned long long) out_capacity);
  const uint64_t n_tiles = (count + PR_BLOCK - 1) / PR_BLOCK;
  DevTmp < PileRec > d_out;
  TRY (dev_alloc (d, &d_out.p, (size_t) total));
  hipLaunchKernelGGL (pile_emit_kernel, dim3 ((unsigned) n_tiles), dim3 (PR_BLOCK), 0, d->stream, pile_of (d), first, count, d_to,
                      d_out, total);
  if (hipStreamSynchronize (d->stream) != hipSuccess
      || hipMemcpy (out, d_out, total * sizeof (PileRec), hipMemcpyDeviceToHost) != hipSuccess)
    return fail (d, "fetch_records: copy failed");
  return 0;
}

// the timing events of one pemap_dev_fetch_records_gz, destroyed on every return
struct PmGzEvents
{
  hipEvent_t e[12] = {};
  ~PmGzEvents ()
  {
    for (hipEvent_t & x : e)
      pm_event_free (x);
  }
};

// device bytes to the caller's buffer: directly where the caller pinned it, else through the object's two page-locked blocks, the
// copy of block k + 1 under the host's memcpy of block k
static int gz_to_host (pemap_dev * d, char *out, const char *d_src, size_t bytes)
{
  if (pm_host_pin_lookup (out, bytes))
    {
      HIPCHK (d, hipMemcpyAsync (out, d_src, bytes, hipMemcpyDeviceToHost, d->stream));
      HIPCHK (d, hipStreamSynchronize (d->stream));
      return 0;
    }
  for (char *&h : d->gz.h_block)
    if (!h)
      HIPCHK (d, hipHostMalloc ((void **) &h, PM_GZ_BLOCK, hipHostMallocDefault));
  size_t prev_o = 0, prev_m = 0;
  int k = 0;
  for (size_t o = 0; o < bytes; o += PM_GZ_BLOCK, k++)
    {
      const size_t m = bytes - o < PM_GZ_BLOCK ? bytes - o : PM_GZ_BLOCK;
      // (block k & 1 was copied out of in the turn before the last: the stream is waited for in every turn)
      HIPCHK (d, hipMemcpyAsync (d->gz.h_block[k & 1], d_src + o, m, hipMemcpyDeviceToHost, d->stream));
      if (prev_m)
        memcpy (out + prev_o, d->gz.h_block[(k & 1) ^ 1], prev_m);
      HIPCHK (d, hipStreamSynchronize (d->stream));
      prev_o = o;
      prev_m = m;
    }
  if (prev_m)
    memcpy (out + prev_o, d->gz.h_block[(k & 1) ^ 1], prev_m);
  return 0;
}

// The records of pemap_dev_fetch_records stay on the device: their insertion sites are compacted, the records deflated piece by
// piece into BGZF members (pemap_gz.hip.h, the rule: pemap_gz_rule.h), the members packed; the packed bytes and the sites come back.
extern "C" int pemap_dev_fetch_records_gz (pemap_dev * d, uint64_t first, uint64_t count, void *gz_out, uint64_t gz_capacity, uint64_t * gz_bytes,
                                           uint64_t * n_records, void *ins_records, uint64_t ins_capacity, uint64_t * n_ins)
{
  if (!d)
    return 1;
  if (!gz_bytes || !n_records || !n_ins)
    return fail (d, "fetch_records_gz: gz_bytes, n_records and n_ins must not be NULL");
  HIPCHK (d, hipSetDevice (d->device));         // (before the events are made)
  *gz_bytes = *n_records = *n_ins = 0;
  memset (d->gz.ms, 0, sizeof d->gz.ms);
  PmGzEvents E;
  for (hipEvent_t & x : E.e)
    if (hipEventCreate (&x) != hipSuccess)
      return fail (d, "fetch_records_gz: hipEventCreate failed");
  int n_ev = 2;                 // (0 and 1: around the count and its scan, pile_count_range)
  auto stamp = [&] () { return hipEventRecord (E.e[n_ev++], d->stream); };
  auto between = [&] (int a, int b, float *ms) -> int
  {
    float v = 0.f;
    HIPCHK (d, hipEventElapsedTime (&v, E.e[a], E.e[b]));
    *ms += v;
    return 0;
  };
  // ---- the records (the kernels of pemap_dev_fetch_records)
  DevTmp < uint64_t > d_to, d_total;
  uint64_t total = 0;
  TRY (pile_count_range (d, "fetch_records_gz", first, count, d_to, &total, E.e));
  *n_records = total;
  if (!total)
    return 0;
  const uint64_t n_tiles = (count + PR_BLOCK - 1) / PR_BLOCK;
  TRY (dev_alloc (d, &d_total.p, 3));   // [1] insertion sites, [2] packed bytes
  const uint64_t n_pieces = pmz_pieces (total), n_itiles = (total + PMZ_BLOCK - 1) / PMZ_BLOCK;
  const uint64_t slot_bytes = n_pieces * PMZ_SLOT + PMZ_SLOT_SLACK;
  DevTmp < uint4 > d_rec, d_ins;
  DevTmp < unsigned char >d_slots, d_gz;
  DevTmp < uint32_t > d_mlen, d_ic;
  DevTmp < uint64_t > d_mat, d_io;
  TRY (dev_alloc (d, &d_rec.p, (size_t) total));
  TRY (dev_alloc (d, &d_slots.p, (size_t) slot_bytes));
  TRY (dev_alloc (d, &d_mlen.p, (size_t) n_pieces));
  TRY (dev_alloc (d, &d_mat.p, (size_t) n_pieces));
  TRY (dev_alloc (d, &d_ic.p, (size_t) n_itiles));
  TRY (dev_alloc (d, &d_io.p, (size_t) n_itiles));
  HIPCHK (d, stamp ());         // 2
  hipLaunchKernelGGL (pile_emit_kernel, dim3 ((unsigned) n_tiles), dim3 (PR_BLOCK), 0, d->stream, pile_of (d), first, count, d_to, (PileRec *) d_rec.p, total);
  HIPCHK (d, stamp ());         // 3
  // ---- the insertion sites' counts, the members, their places
  hipLaunchKernelGGL (pmz_ins_count_kernel, dim3 ((unsigned) n_itiles), dim3 (PMZ_BLOCK), 0, d->stream, d_rec, total, d_ic);
  hipLaunchKernelGGL (ix_scan_tiles_kernel, dim3 (1), dim3 (1024), 0, d->stream, d_ic, d_io, n_itiles, d_total.p + 1);
  HIPCHK (d, stamp ());         // 4
  hipLaunchKernelGGL (pmz_deflate_kernel, dim3 ((unsigned) n_pieces), dim3 (PMZ_BLOCK), 0, d->stream, d_rec, total, d_slots, n_pieces, d_mlen);
  HIPCHK (d, stamp ());         // 5
  hipLaunchKernelGGL (ix_scan_tiles_kernel, dim3 (1), dim3 (1024), 0, d->stream, d_mlen, d_mat, n_pieces, d_total.p + 2);
  HIPCHK (d, stamp ());         // 6
  uint64_t two[2] = { 0, 0 };
  HIPCHK (d, hipMemcpyAsync (two, d_total.p + 1, 16, hipMemcpyDeviceToHost, d->stream));
  HIPCHK (d, hipStreamSynchronize (d->stream));
  HIPCHK (d, hipGetLastError ());
  const uint64_t ins = two[0], packed = two[1];
  if (ins > total || packed < n_pieces * (PMZ_HEAD + PMZ_TAIL) || packed > n_pieces * PMZ_MEMBER_MAX)
    return fail (d, "internal: fetch_records_gz: %llu insertion sites and %llu bytes for %llu records", (unsigned long long) ins, (unsigned long long) packed,
                 (unsigned long long) total);
  *n_ins = ins;
  *gz_bytes = packed;
  // (nothing has been written to the caller's buffers so far, and nothing is unless both hold what they have to)
  if (gz_out && packed > gz_capacity)
    return fail (d, "fetch_records_gz: %llu bytes of members do not fit the caller's %llu", (unsigned long long) packed, (unsigned long long) gz_capacity);
  if (gz_out && ins_records && ins > ins_capacity)
    return fail (d, "fetch_records_gz: %llu insertion records do not fit the caller's %llu", (unsigned long long) ins, (unsigned long long) ins_capacity);
  TRY (between (0, 1, &d->gz.ms[0]));
  TRY (between (2, 3, &d->gz.ms[0]));
  TRY (between (3, 4, &d->gz.ms[1]));
  TRY (between (4, 5, &d->gz.ms[2]));
  TRY (between (5, 6, &d->gz.ms[3]));
  if (!gz_out)
    return 0;                   // (the sizes only: no insertion list, no packed array)
  TRY (dev_alloc (d, &d_ins.p, (size_t) ins));
  TRY (dev_alloc (d, &d_gz.p, (size_t) packed + 16));
  HIPCHK (d, stamp ());         // 7
  hipLaunchKernelGGL (pmz_ins_emit_kernel, dim3 ((unsigned) n_itiles), dim3 (PMZ_BLOCK), 0, d->stream, d_rec, total, d_io, d_ins, ins);
  HIPCHK (d, stamp ());         // 8
  hipLaunchKernelGGL (pmz_pack_kernel, dim3 ((unsigned) n_pieces), dim3 (PMZ_BLOCK), 0, d->stream, d_slots, n_pieces, slot_bytes, d_mat, d_mlen, d_gz, packed);
  HIPCHK (d, stamp ());         // 9
  HIPCHK (d, hipStreamSynchronize (d->stream));
  HIPCHK (d, hipGetLastError ());
  TRY (between (7, 8, &d->gz.ms[1]));
  TRY (between (8, 9, &d->gz.ms[3]));
  TRY (gz_to_host (d, (char *) gz_out, (const char *) d_gz.p, (size_t) packed));
  if (ins_records && ins)
    HIPCHK (d, hipMemcpy (ins_records, d_ins, (size_t) ins * sizeof (uint4), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int pemap_dev_fetch_gz_ms (pemap_dev * d, float *ms4)
{
  memcpy (ms4, d->gz.ms, sizeof d->gz.ms);
  return 0;
}

// ------------------------------------------------------------------------------------------------------------
extern "C" int pemap_dev_synth_genome (pemap_dev * d, uint64_t seed, uint64_t genome_size, int n_contigs, double repeat_frac,
                                       void **d_genome_out, uint32_t * contig_len)
{
  HIPCHK (d, hipSetDevice (d->device));
  if (n_contigs < 1 || genome_size < (uint64_t) n_contigs * 1000)
    return fail (d, "synth_genome: bad sizes");
  // hg38-like relative contig lengths (chr1..22, X, Y, M in Mbp) when 25 contigs are asked for, equal split otherwise
  static const double hg[25] = { 248.9, 242.2, 198.3, 190.2, 181.5, 170.8, 159.3, 145.1, 138.4, 133.8, 135.1, 133.3, 114.4, 107.0,
    102.0, 90.3, 83.3, 80.4, 58.6, 64.4, 46.7, 50.8, 156.0, 57.2, 0.0166
  };
  std::vector < uint64_t > real (n_contigs + 1);
  double tot = 0;
  for (int c = 0; c < n_contigs; c++)
    tot += (n_contigs == 25) ? hg[c] : 1.0;
  real[0] = 0;
  uint64_t used = 0;
  for (int c = 0; c < n_contigs; c++)
    {
      uint64_t ln = (uint64_t) ((double) genome_size * ((n_contigs == 25) ? hg[c] : 1.0) / tot);
      if (ln < 64)
        ln = 64;
      if (c == n_contigs - 1)
        ln = genome_size - used;
      contig_len[c] = (uint32_t) ln;
      used += ln;
      real[c + 1] = used;
    }
  if (used != genome_size)
    return fail (d, "synth_genome: contig split failed");
  uint8_t *g = nullptr;
  TRY (dev_alloc (d, &g, genome_size + 512));
  DevTmp < uint64_t > d_real;
  TRY (dev_alloc (d, &d_real.p, (size_t) n_contigs + 1));
  HIPCHK (d, hipMemcpy (d_real, real.data (), (n_contigs + 1) * 8, hipMemcpyHostToDevice));
  unsigned thr = (unsigned) (repeat_frac * 16777216.0);
  hipLaunchKernelGGL (sy_genome_kernel, dim3 ((unsigned) ((genome_size + 255) / 256)), dim3 (256), 0, d->stream, seed, g, genome_size, d_real,
                      n_contigs, thr);
  HIPCHK (d, hipStreamSynchronize (d->stream));
  *d_genome_out = g;
  return 0;
}

extern "C" int pemap_dev_free (pemap_dev * d, void *d_ptr)
{
  HIPCHK (d, hipSetDevice (d->device));
  HIPCHK (d, hipFree (d_ptr));
  return 0;
}

static int synth_reads (pemap_dev * d, uint64_t seed, int n, int read_len, int paired, double sub_rate, double indel_rate, double one_indel_frac,
                        uint64_t first_read)
{
  HIPCHK (d, hipSetDevice (d->device));
  if (!d->ix.ready)
    return fail (d, "synth_reads: needs the resident genome");
  if (read_len < PEMAP_MIN_READ || read_len > PEMAP_MAX_READ || n <= 0)
    return fail (d, "synth_reads: bad n/read_len");
  if (d->ix.gsize < 2000)
    return fail (d, "synth_reads: genome too small");
  int stride = (read_len + 15) & ~15;
  TRY (ring_leave (d, n, stride, paired));
  d->paired = paired ? 1 : 0;   // (behind the deliveries of ring_leave, which read the old value)
  int ends = paired ? 2 * n : n;
  hipLaunchKernelGGL (sy_reads_kernel, dim3 ((ends + 255) / 256), dim3 (256), 0, d->stream, seed, d->ix.d_genome, d->ix.gsize, n, read_len, paired,
                      (unsigned) (sub_rate * 16777216.0), (unsigned) (indel_rate * 16777216.0), first_read, d->rd.d_rows[0], d->rd.d_len[0],
                      d->rd.d_rows[1], d->rd.d_len[1], stride, (unsigned) (one_indel_frac * 16777216.0));
  HIPCHK (d, hipStreamSynchronize (d->stream));
  d->rd.h_len[0].assign (n, read_len);
  d->rd.h_len[1].assign (paired ? n : 0, read_len);
  reads_staged (d, n, paired, read_len, read_len);
  return 0;
}

extern "C" int pemap_dev_synth_reads (pemap_dev * d, uint64_t seed, int n, int read_len, int paired, double sub_rate,
                                      double indel_rate, uint64_t first_read)
{
  return synth_reads (d, seed, n, read_len, paired, sub_rate, indel_rate, 0.0, first_read);
}

extern "C" int pemap_dev_synth_reads_indel (pemap_dev * d, uint64_t seed, int n, int read_len, int paired, double sub_rate,
                                            double indel_read_frac, uint64_t first_read)
{
  return synth_reads (d, seed, n, read_len, paired, sub_rate, 0.0, indel_read_frac, first_read);
}

extern "C" int pemap_dev_staged_reads (pemap_dev * d, char *reads1, int *len1, char *reads2, int *len2, int stride)
{
  HIPCHK (d, hipSetDevice (d->device));
  if (d->rd.n <= 0)
    return fail (d, "staged_reads: nothing staged");
  if (stride != d->rd.stride)
    return fail (d, "staged_reads: the staged row stride is %d", d->rd.stride);
  HIPCHK (d, hipStreamSynchronize (d->stream));
  char *const rows[2] = { reads1, reads2 };
  int *const lens[2] = { len1, len2 };
  for (int m = 0; m < (d->rd.paired && reads2 ? 2 : 1); m++)
    {
      HIPCHK (d, hipMemcpy (rows[m], d->rd.d_rows[m], (size_t) d->rd.n * stride, hipMemcpyDeviceToHost));
      HIPCHK (d, hipMemcpy (lens[m], d->rd.d_len[m], (size_t) d->rd.n * 4, hipMemcpyDeviceToHost));
    }
  return 0;
}

extern "C" int pemap_dev_staged_info (pemap_dev * d, int *n, int *stride, int *paired)
{
  *n = d->rd.n;
  *stride = d->rd.stride;
  *paired = d->rd.paired;
  return 0;
}

// ---- fastq text -> read rows on the device -----------------------------------------------------------------
// pemap_dev_stage_fastq and pemap_dev_submit_fastq are pemap_dev_stage_reads and pemap_dev_submit_batch with the rows made by the
// kernels of pemap_fastq.hip.h instead of fill_rows (pemapper_main.c).  Both are fq_parse (text up, stages 1-3, the control blocks
// back: the result but for `consumed`) and, when the batch holds a pair at least, fq_rows (stage 4 into the staged arrays, the lengths
// and `consumed` back); they differ in the stream and in where the rows go.
struct PmFastqArgs
{
  const char *text[2];
  uint64_t bytes[2];
  int state[2];
  int trim_start, trim_end, max_records, stride;
};

// the arrays of the parse that share `cap` hold `need` elements each at least (their contents are not kept); cap is set behind the last
template < class ... T > static int fq_grow (pemap_dev * d, size_t & cap, size_t need, T * &... p)
{
  if (cap >= need && (... && p))
    return 0;
  pm_free (p...);
  cap = 0;
  int rc = 0;
  ((rc = rc ? rc : dev_alloc (d, &p, need)), ...);
  cap = rc ? 0 : need;
  return rc;
}

static int fq_check_args (pemap_dev * d, const char *who, const PmFastqArgs & a, const pemap_fastq_result * res)
{
  if (!res || !a.text[0])
    return fail (d, "%s: a required pointer is NULL", who);
  if (d->paired && !a.text[1])
    return fail (d, "%s: paired mode needs the second text", who);
  if (a.stride < PEMAP_MIN_READ || a.stride < PEMAP_MAX_READ)
    return fail (d, "%s: stride %d is below the longest read a row may hold (%d)", who, a.stride, PEMAP_MAX_READ);
  if (a.max_records <= 0)
    return fail (d, "%s: max_records = %d", who, a.max_records);
  if (a.trim_start < 0 || a.trim_end < 0)
    return fail (d, "%s: trims %d / %d", who, a.trim_start, a.trim_end);
  for (int m = 0; m < (d->paired ? 2 : 1); m++)
    {
      if (a.state[m] != 0 && a.state[m] != 1)
        return fail (d, "%s: state %d of text %d (0: the beginning of a stream, 1: behind a sequence line)", who, a.state[m], m + 1);
      if (a.bytes[m] > PFQ_MAX_TEXT)
        return fail (d, "%s: text %d has %llu bytes, more than %u a call", who, m + 1, (unsigned long long) a.bytes[m], PFQ_MAX_TEXT);
    }
  return 0;
}

static int fq_parse (pemap_dev * d, hipStream_t st, const PmFastqArgs & a, pemap_fastq_result * res)
{
  PmFastq & F = d->fq;
  const int mates = d->paired ? 2 : 1;
  if (!F.d_ctl)
    {
      TRY (dev_alloc (d, &F.d_ctl, 2));
      HIPCHK (d, hipHostMalloc ((void **) &F.h, sizeof (*F.h), hipHostMallocDefault));
    }
  memset (res, 0, sizeof (*res));
  HIPCHK (d, hipMemsetAsync (F.d_ctl, 0, 2 * sizeof (PfqCtl), st));
  // stage 1, first half: the number of lines
  for (int m = 0; m < mates; m++)
    {
      PmFastqMate & M = F.mate[m];
      const unsigned bytes = (unsigned) a.bytes[m];
      HIPCHK (d, hipMemsetAsync (&F.d_ctl[m].stop, 0xff, sizeof (F.d_ctl[m].stop), st));
      if (!bytes)
        continue;
      const size_t padded = (((size_t) bytes + 15) & ~(size_t) 15) + 16;        // every 16-byte load that begins inside the text stays inside
      TRY (fq_grow (d, M.text_cap, padded, M.d_text));
      HIPCHK (d, hipMemcpyAsync (M.d_text, a.text[m], bytes, hipMemcpyHostToDevice, st));
      const unsigned nt = (bytes + PFQ_TILE - 1) / PFQ_TILE;
      TRY (fq_grow (d, M.tile_cap, nt, M.d_tile_cnt));
      hipLaunchKernelGGL (pfq_nl_count_kernel, dim3 (nt), dim3 (PFQ_BLOCK), 0, st, (const uint4 *) M.d_text, bytes, M.d_tile_cnt);
      hipLaunchKernelGGL (pfq_sum_top_kernel, dim3 (1), dim3 (PFQ_TOP), 0, st, M.d_tile_cnt, nt, &F.d_ctl[m].n_lines);
    }
  HIPCHK (d, hipGetLastError ());
  HIPCHK (d, hipMemcpyAsync (F.h->ctl, F.d_ctl, 2 * sizeof (PfqCtl), hipMemcpyDeviceToHost, st));
  HIPCHK (d, hipStreamSynchronize (st));
  // the rest of stage 1, stages 2 and 3
  unsigned rec_limit[2] = { 0, 0 };
  for (int m = 0; m < mates; m++)
    {
      PmFastqMate & M = F.mate[m];
      const unsigned bytes = (unsigned) a.bytes[m], nl = F.h->ctl[m].n_lines;
      if (!nl)
        continue;
      if (nl > bytes)
        return fail (d, "internal: %u lines in %u bytes", nl, bytes);
      // (a text has no more records than lines: an array of that many serves whatever max_records is)
      const unsigned lim = rec_limit[m] = nl < (unsigned) a.max_records ? nl : (unsigned) a.max_records;
      const unsigned nt = (bytes + PFQ_TILE - 1) / PFQ_TILE, nlt = (nl + PFQ_LINE_TILE - 1) / PFQ_LINE_TILE;
      TRY (fq_grow (d, M.line_cap, (size_t) nl + 1, M.d_line_start));
      TRY (fq_grow (d, M.ltile_cap, nlt, M.d_sums, M.d_tile_in));
      TRY (fq_grow (d, M.rec_cap, lim, M.d_rec_off, M.d_rec_next, M.d_rec_len));
      hipLaunchKernelGGL (pfq_nl_apply_kernel, dim3 (nt), dim3 (PFQ_BLOCK), 0, st, (const uint4 *) M.d_text, bytes, (const unsigned *) M.d_tile_cnt, nl, M.d_line_start);
      hipLaunchKernelGGL (pfq_role_sum_kernel, dim3 (nlt), dim3 (PFQ_BLOCK), 0, st, (const uint8_t *) M.d_text, bytes, (const unsigned *) M.d_line_start, nl, M.d_sums);
      hipLaunchKernelGGL (pfq_role_top_kernel, dim3 (1), dim3 (PFQ_TOP), 0, st, (const PfqTileSum *) M.d_sums, nlt, a.state[m], M.d_tile_in, &F.d_ctl[m]);
      hipLaunchKernelGGL (pfq_records_kernel, dim3 (nlt), dim3 (PFQ_BLOCK), 0, st, (const uint8_t *) M.d_text, bytes, (const unsigned *) M.d_line_start, nl,
                          (const uint2 *) M.d_tile_in, a.trim_start, a.trim_end, m == 0 ? 1 : 0, lim, M.d_rec_off, M.d_rec_len, M.d_rec_next, &F.d_ctl[m]);
    }
  HIPCHK (d, hipGetLastError ());
  HIPCHK (d, hipMemcpyAsync (F.h->ctl, F.d_ctl, 2 * sizeof (PfqCtl), hipMemcpyDeviceToHost, st));
  HIPCHK (d, hipStreamSynchronize (st));
  for (int m = 0; m < mates; m++)
    {
      const PfqCtl & c = F.h->ctl[m];
      const unsigned seen = c.n_records < rec_limit[m] ? c.n_records : rec_limit[m];    // records that were examined
      if (c.stop != PFQ_NO_STOP)
        {
          const unsigned k = (unsigned) (c.stop >> 32);
          if (k >= seen)
            return fail (d, "internal: record %u stops text %d, which has %u", k, m + 1, seen);
          res->got[m] = (int) k;
          res->end[m] = (c.stop & PFQ_STOP_BAD_LEN) ? PFQ_END_BAD_LEN : PFQ_END_SHORT_FIRST;
          res->bad_len[m] = res->end[m] == PFQ_END_BAD_LEN ? (int) (c.stop & (PFQ_STOP_BAD_LEN - 1u)) : 0;
        }
      else
        {
          res->got[m] = (int) seen;
          res->end[m] = pfq_end_unstopped (res->got[m], a.max_records);
        }
    }
  res->n = pfq_pairs (res->got[0], res->got[1], d->paired);
  return 0;
}

// records [0, n) of the last fq_parse into rows / lens on the device (per mate), the lengths into h_len[m] as well; res->consumed
static int fq_rows (pemap_dev * d, hipStream_t st, const PmFastqArgs & a, int n, uint8_t * const rows[2], int *const lens[2], int *const h_len[2], int *mx, int *mn,
                    pemap_fastq_result * res)
{
  PmFastq & F = d->fq;
  const int mates = d->paired ? 2 : 1;
  const unsigned per_block = PFQ_BLOCK / PFQ_ROW_LANES;
  for (int m = 0; m < mates; m++)
    {
      PmFastqMate & M = F.mate[m];
      if ((size_t) n > M.rec_cap)
        return fail (d, "internal: %d rows of %zu records", n, M.rec_cap);
      hipLaunchKernelGGL (pfq_rows_kernel, dim3 (((unsigned) n + per_block - 1) / per_block), dim3 (PFQ_BLOCK), 0, st, (const uint8_t *) M.d_text, (unsigned) a.bytes[m],
                          (const unsigned *) M.d_rec_off, (const int *) M.d_rec_len, (unsigned) n, (unsigned) a.stride, rows[m], lens[m]);
      HIPCHK (d, hipGetLastError ());
      HIPCHK (d, hipMemcpyAsync (h_len[m], lens[m], (size_t) n * sizeof (int), hipMemcpyDeviceToHost, st));
      HIPCHK (d, hipMemcpyAsync (&F.h->next[m], M.d_rec_next + (n - 1), sizeof (unsigned), hipMemcpyDeviceToHost, st));
    }
  HIPCHK (d, hipStreamSynchronize (st));
  for (int m = 0; m < mates; m++)
    {
      res->consumed[m] = F.h->next[m];
      TRY (check_lengths (d, h_len[m], n, mx, mn));
    }
  return 0;
}

extern "C" int pemap_dev_stage_fastq (pemap_dev * d, const char *text1, uint64_t bytes1, int state1, const char *text2, uint64_t bytes2, int state2, int trim_start,
                                      int trim_end, int max_records, int stride, pemap_fastq_result * res)
{
  HIPCHK (d, hipSetDevice (d->device));
  const PmFastqArgs a = { { text1, text2 }, { bytes1, bytes2 }, { state1, state2 }, trim_start, trim_end, max_records, stride };
  TRY (fq_check_args (d, "stage_fastq", a, res));
  TRY (fq_parse (d, d->stream, a, res));
  const int n = res->n;
  if (n == 0)
    return 0;
  TRY (ring_leave (d, n, stride, d->paired));
  d->rd.h_len[0].assign ((size_t) n, 0);
  d->rd.h_len[1].assign (d->paired ? (size_t) n : 0, 0);
  int *const h_len[2] = { d->rd.h_len[0].data (), d->rd.h_len[1].data () };
  int mx = 0, mn = 1 << 30;
  TRY (fq_rows (d, d->stream, a, n, d->rd.d_rows, d->rd.d_len, h_len, &mx, &mn, res));
  reads_staged (d, n, d->paired, mx, mn);
  return 0;
}

extern "C" int pemap_dev_submit_fastq (pemap_dev * d, const char *text1, uint64_t bytes1, int state1, const char *text2, uint64_t bytes2, int state2, int trim_start,
                                       int trim_end, int max_records, int stride, uint32_t * m1, uint32_t * m2, int *mapping_type, pemap_fastq_result * res,
                                       uint64_t * ticket)
{
  std::unique_lock < std::mutex > sub (d->submit_mu);
  std::unique_lock < std::mutex > lk (d->mu);
  HIPCHK (d, hipSetDevice (d->device));
  if (!d->ix.ready)
    return fail (d, "submit_fastq: no index loaded");
  const PmFastqArgs a = { { text1, text2 }, { bytes1, bytes2 }, { state1, state2 }, trim_start, trim_end, max_records, stride };
  TRY (fq_check_args (d, "submit_fastq", a, res));
  if (!m1 || !mapping_type || !ticket || (d->paired && !m2))
    return fail (d, "submit_fastq: a required pointer is NULL");
  if (!d->rg.stream_h2d)
    HIPCHK (d, hipStreamCreateWithFlags (&d->rg.stream_h2d, hipStreamNonBlocking));
  // text and parse kernels on the copy stream: the batches in flight keep the pipeline's streams busy meanwhile
  TRY (fq_parse (d, d->rg.stream_h2d, a, res));
  const int n = res->n;
  if (n == 0)
    return 0;
  PmSlotTake t;
  TRY (ring_take (d, n, stride, lk, t));
  PmRingSlot & r = *t.r;
  int mx = 0, mn = 1 << 30;
  TRY (fq_rows (d, d->rg.stream_h2d, a, n, t.rows, t.lens, t.h_len, &mx, &mn, res));
  for (int m = 0; m < (d->paired ? 2 : 1); m++)
    memcpy (&d->rd.h_len[m][t.first], t.h_len[m], (size_t) n * sizeof (int));
  // the rows are on the device already: every slice's event is the same point of the copy stream
  int slice;
  TRY (ring_slices (d, r, n, mx, mn, &slice));
  for (int k = 0; k * slice < n; k++)
    HIPCHK (d, hipEventRecord (r.ev_copy[k], d->rg.stream_h2d));
  return ring_queue_run (d, r, t.first, n, m1, m2, mapping_type, ticket);
}
