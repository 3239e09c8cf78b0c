// pemap_fastq.hip.h -- read rows made on the device from one mate's fastq text (pemap_dev_stage_fastq / pemap_dev_submit_fastq).
//
// The host walk this stands for is fill_rows of pemapper_main.c (in the reference the read loop of pemapper.c:649-748): a memchr per
// line and a copy per sequence.  The rule itself -- which lines are reads, how long they are, where a mate stops -- is
// pemap_fastq_rule.h, shared with the host.  Here, over a text that lies in device memory:
//   1. line ends  pfq_nl_count_kernel    a lane takes 16 bytes with one aligned 16-byte load and counts its '\n' bytes (the mask is cut
//                                        at the text's length: nothing behind it is ever looked at); a count per tile of PFQ_TILE bytes
//                 pfq_sum_top_kernel     one block turns the tile counts into the tiles' first line indices, PFQ_TOP at a time, and
//                                        leaves the number of lines in PfqCtl
//                 pfq_nl_apply_kernel    every tile again: line j + 1 begins behind the j-th '\n'; line_start[0 .. n_lines], so a
//                                        line's length is the next start minus 1 minus its own
//   2. roles      pfq_role_sum_kernel    a line's effect on the walk is one of two maps of five states onto five states (15 bits); a
//                                        lane composes the maps of its PFQ_LINES_PER_LANE lines, the block scans them, and a tile of
//                                        PFQ_LINE_TILE lines leaves its map and, for each of the five states it may be entered in, its
//                                        number of sequence lines
//                 pfq_role_top_kernel    one block, PFQ_TOP tiles at a time: a scan over the composed maps gives every tile the state it
//                                        is entered in (given state_in), a prefix sum over the counts that belong to that state its
//                                        first record index
//   3. records    pfq_records_kernel     every tile again with its entry state: the same two scans inside the block give every line its
//                                        state and every sequence line its record index; records below max_records get their row's
//                                        offset and length (the trim arithmetic of the rule) or, where the length stops the mate, enter
//                                        the lowest stopping index with an atomicMin on a 64-bit word of PfqCtl (as PcmCtl::bad)
//   4. rows       pfq_rows_kernel        launched once n is known: PFQ_ROW_LANES lanes a record copy the trimmed bytes into the row
//                                        and write its length, for records below n only
// An offset becomes an address only after it was checked against the text's length, a line index against n_lines, a record index
// against max_records (stage 3) or n (stage 4), a length against the row stride.  Offsets are 32-bit: PFQ_MAX_TEXT bytes a text at most.
// Footprint (the kernels run on the copy stream beside the seed stage's ten persistent waves per CU): no scratch, at most 128 VGPRs
// and 10,240 bytes of static LDS per workgroup, each; tests/test_fastq_kernel_resources_cpu.py reads the compiler's remarks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/pemap_hip.h"
#include "pemap_fastq_rule.h"

#define PFQ_BLOCK 256
#define PFQ_TILE (PFQ_BLOCK * 16)       // bytes of text a block of the line-end scan takes
#define PFQ_TOP 1024                    // tile counts (or tile maps) the one top-level block takes at a time
#define PFQ_LINES_PER_LANE 4
#define PFQ_LINE_TILE (PFQ_BLOCK * PFQ_LINES_PER_LANE)  // lines a block of the role and record scans takes
#define PFQ_ROW_LANES 32
#define PFQ_NO_STOP 0xffffffffffffffffull
#define PFQ_STOP_BAD_LEN (1u << 31)     // PfqCtl.stop = record index << 32 | PFQ_STOP_BAD_LEN (end 3, else end 2) | sl (< 2^30)

struct PfqCtl
{
  unsigned long long stop;      // the lowest record index whose length stops the mate, with what it stops it; PFQ_NO_STOP: none
  unsigned n_lines, n_records;  // complete lines of the text; sequence lines among them
};

struct PfqTileSum
{
  unsigned map, pad;            // the tile's lines composed
  unsigned long long cnt;       // 12 bits per entry state: sequence lines of the tile when it is entered in that state
};

// bit k: byte k of the lane's 16 is '\n'; `valid` bytes of them belong to the text
__device__ __forceinline__ unsigned pfq_nl_mask (const uint4 v, unsigned valid)
{
  const unsigned w[4] = { v.x, v.y, v.z, v.w };
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 16; k++)
    m |= (((w[k >> 2] >> (8 * (k & 3))) & 0xffu) == (unsigned) '\n' ? 1u : 0u) << k;
  return valid >= 16u ? m : m & ((1u << valid) - 1u);
}

// the lane's mask of line ends: its 16 bytes are loaded only if they begin inside the text (the allocation is padded to whole loads)
__device__ __forceinline__ unsigned pfq_lane_mask (const uint4 * __restrict__ text16, unsigned bytes, unsigned g)
{
  const unsigned long long off = (unsigned long long) g * 16u;
  return off < bytes ? pfq_nl_mask (text16[g], bytes - (unsigned) off) : 0u;
}

// exclusive prefix sum over the block's threads (all of them call); ws: NT / 64 words of LDS; *total: the block's sum
template < int NT > __device__ __forceinline__ unsigned pfq_block_scan_sum (unsigned v, unsigned *ws, unsigned *total)
{
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1)
    {
      const unsigned u = __shfl_up (inc, o, 64);
      if (lane >= (unsigned) o)
        inc += u;
    }
  __syncthreads ();             // (ws may still be read from the call before)
  if (lane == 63u)
    ws[w] = inc;
  __syncthreads ();
  unsigned base = 0, tot = 0;
#pragma unroll
  for (unsigned k = 0; k < NT / 64; k++)
    {
      const unsigned s = ws[k];
      base += k < w ? s : 0u;
      tot += s;
    }
  *total = tot;
  return base + inc - v;
}

// the same over composed maps: returns the composition of the maps of the threads before this one (the identity for thread 0)
template < int NT > __device__ __forceinline__ unsigned pfq_block_scan_map (unsigned m, unsigned *ws, unsigned *total)
{
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  unsigned inc = m;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1)
    {
      const unsigned u = __shfl_up (inc, o, 64);
      if (lane >= (unsigned) o)
        inc = pfq_map_then (u, inc);
    }
  __syncthreads ();
  if (lane == 63u)
    ws[w] = inc;
  __syncthreads ();
  unsigned base = PFQ_MAP_IDENTITY, tot = PFQ_MAP_IDENTITY;
#pragma unroll
  for (unsigned k = 0; k < NT / 64; k++)
    {
      const unsigned s = ws[k];
      if (k < w)
        base = pfq_map_then (base, s);
      tot = pfq_map_then (tot, s);
    }
  *total = tot;
  const unsigned before = __shfl_up (inc, 1, 64);
  return lane ? pfq_map_then (base, before) : base;
}

// ---- 1. line ends
__global__ void __launch_bounds__ (PFQ_BLOCK) pfq_nl_count_kernel (const uint4 * __restrict__ text16, unsigned bytes, unsigned *__restrict__ tile_cnt)
{
  __shared__ unsigned ws[PFQ_BLOCK / 64];
  unsigned tot;
  (void) pfq_block_scan_sum < PFQ_BLOCK > ((unsigned) __popc (pfq_lane_mask (text16, bytes, blockIdx.x * PFQ_BLOCK + threadIdx.x)), ws, &tot);
  if (threadIdx.x == 0)
    tile_cnt[blockIdx.x] = tot;
}

// one block: cnt[0 .. n) become their exclusive prefix sums, PFQ_TOP at a time; *total their sum
__global__ void __launch_bounds__ (PFQ_TOP) pfq_sum_top_kernel (unsigned *__restrict__ cnt, unsigned n, unsigned *__restrict__ total)
{
  __shared__ unsigned ws[PFQ_TOP / 64];
  unsigned carry = 0;
  for (unsigned b = 0; b < n; b += PFQ_TOP)
    {
      const unsigned i = b + threadIdx.x;
      const unsigned own = i < n ? cnt[i] : 0u;
      unsigned tot;
      const unsigned ex = pfq_block_scan_sum < PFQ_TOP > (own, ws, &tot);
      if (i < n)
        cnt[i] = carry + ex;
      carry += tot;
    }
  if (threadIdx.x == 0)
    *total = carry;
}

// line_start[n_lines + 1]: line j + 1 begins behind the j-th '\n'
__global__ void __launch_bounds__ (PFQ_BLOCK) pfq_nl_apply_kernel (const uint4 * __restrict__ text16, unsigned bytes, const unsigned *__restrict__ tile_off, unsigned n_lines,
                                                                   unsigned *__restrict__ line_start)
{
  __shared__ unsigned ws[PFQ_BLOCK / 64];
  const unsigned g = blockIdx.x * PFQ_BLOCK + threadIdx.x;
  unsigned m = pfq_lane_mask (text16, bytes, g);
  unsigned tot;
  unsigned j = tile_off[blockIdx.x] + pfq_block_scan_sum < PFQ_BLOCK > ((unsigned) __popc (m), ws, &tot);
  if (g == 0)
    line_start[0] = 0u;
  while (m)
    {
      const unsigned k = (unsigned) __ffs (m) - 1u;
      m &= m - 1u;
      if (j < n_lines)          // (it is: the counts were made from the same masks)
        line_start[j + 1] = g * 16u + k + 1u;
      j++;
    }
}

// ---- 2. roles
// The lane's lines j0 .. j0 + PFQ_LINES_PER_LANE - 1 (those below n_lines): bit k of the return value = line j0 + k begins with '@'.
__device__ __forceinline__ unsigned pfq_lane_ats (const uint8_t * __restrict__ text, unsigned bytes, const unsigned *__restrict__ line_start, unsigned n_lines, unsigned j0)
{
  unsigned ats = 0;
#pragma unroll
  for (unsigned k = 0; k < PFQ_LINES_PER_LANE; k++)
    if (j0 + k < n_lines)
      {
        const unsigned s = line_start[j0 + k];
        if (s < bytes && text[s] == (uint8_t) '@')
          ats |= 1u << k;
      }
  return ats;
}

// the lane's lines composed, and per entry state (3 bits each) how many of them are met in SEQ
__device__ __forceinline__ unsigned pfq_lane_map (unsigned ats, unsigned n_lines, unsigned j0, unsigned *cnt_pack)
{
  unsigned map = 0, cnt = 0;
#pragma unroll
  for (int s0 = 0; s0 < PFQ_STATES; s0++)
    {
      int s = s0;
      unsigned c = 0;
#pragma unroll
      for (unsigned k = 0; k < PFQ_LINES_PER_LANE; k++)
        if (j0 + k < n_lines)
          {
            c += s == PFQ_SEQ ? 1u : 0u;
            s = pfq_next (s, (int) ((ats >> k) & 1u));
          }
      map |= (unsigned) s << (3 * s0);
      cnt |= c << (3 * s0);
    }
  *cnt_pack = cnt;
  return map;
}

__global__ void __launch_bounds__ (PFQ_BLOCK) pfq_role_sum_kernel (const uint8_t * __restrict__ text, unsigned bytes, const unsigned *__restrict__ line_start, unsigned n_lines,
                                                                   PfqTileSum * __restrict__ sums)
{
  __shared__ unsigned ws[PFQ_BLOCK / 64];
  __shared__ unsigned long long wc[PFQ_BLOCK / 64];
  const unsigned j0 = (blockIdx.x * PFQ_BLOCK + threadIdx.x) * PFQ_LINES_PER_LANE;
  unsigned cnt_pack, tile_map;
  const unsigned map = pfq_lane_map (pfq_lane_ats (text, bytes, line_start, n_lines, j0), n_lines, j0, &cnt_pack);
  const unsigned before = pfq_block_scan_map < PFQ_BLOCK > (map, ws, &tile_map);
  // entered in state s the tile reaches this lane in state before (s), and the lane then has cnt_pack's count of that state
  unsigned long long c = 0;
#pragma unroll
  for (int s = 0; s < PFQ_STATES; s++)
    c |= (unsigned long long) ((cnt_pack >> (3 * pfq_map_apply (before, s))) & 7u) << (12 * s);
  for (int o = 32; o > 0; o >>= 1)
    c += __shfl_down (c, o, 64);        // (no carry between the fields: a tile has PFQ_LINE_TILE < 2^12 lines)
  if ((threadIdx.x & 63u) == 0)
    wc[threadIdx.x >> 6] = c;
  __syncthreads ();
  if (threadIdx.x == 0)
    {
      PfqTileSum t;
      t.map = tile_map;
      t.pad = 0;
      t.cnt = wc[0] + wc[1] + wc[2] + wc[3];
      sums[blockIdx.x] = t;
    }
}
static_assert (PFQ_BLOCK == 256 && PFQ_LINE_TILE < (1 << 12), "four wave sums; 12-bit count fields");

// one block: tile_in[i] = { the state tile i is entered in, its first record index }; the number of records into PfqCtl
__global__ void __launch_bounds__ (PFQ_TOP) pfq_role_top_kernel (const PfqTileSum * __restrict__ sums, unsigned n_tiles, int state_in, uint2 * __restrict__ tile_in,
                                                                 PfqCtl * __restrict__ ctl)
{
  __shared__ unsigned ws[PFQ_TOP / 64];
  int state = pfq_state_in (state_in);
  unsigned rec = 0;
  for (unsigned b = 0; b < n_tiles; b += PFQ_TOP)
    {
      const unsigned i = b + threadIdx.x;
      PfqTileSum t;
      t.map = PFQ_MAP_IDENTITY;
      t.cnt = 0;
      if (i < n_tiles)
        t = sums[i];
      unsigned all_map, all_cnt;
      const int entry = pfq_map_apply (pfq_block_scan_map < PFQ_TOP > (t.map, ws, &all_map), state);
      const unsigned own = (unsigned) ((t.cnt >> (12 * entry)) & 0xfffull);
      const unsigned ex = pfq_block_scan_sum < PFQ_TOP > (own, ws, &all_cnt);
      if (i < n_tiles)
        tile_in[i] = make_uint2 ((unsigned) entry, rec + ex);
      state = pfq_map_apply (all_map, state);
      rec += all_cnt;
    }
  if (threadIdx.x == 0)
    ctl->n_records = rec;
}

// ---- 3. records: rec_off / rec_len / rec_next [max_records] = where record k's row begins in the text, its length, and the offset
// just behind its line's '\n' (rec_next for every record below max_records, the other two for those whose length counts)
__global__ void __launch_bounds__ (PFQ_BLOCK) pfq_records_kernel (const uint8_t * __restrict__ text, unsigned bytes, const unsigned *__restrict__ line_start, unsigned n_lines,
                                                                  const uint2 * __restrict__ tile_in, int trim_start, int trim_end, int first_mate, unsigned max_records,
                                                                  unsigned *__restrict__ rec_off, int *__restrict__ rec_len, unsigned *__restrict__ rec_next,
                                                                  PfqCtl * __restrict__ ctl)
{
  __shared__ unsigned ws[PFQ_BLOCK / 64];
  const uint2 in = tile_in[blockIdx.x];
  if (in.y >= max_records)
    return;                     // (the whole block: none of its records is examined)
  const unsigned j0 = (blockIdx.x * PFQ_BLOCK + threadIdx.x) * PFQ_LINES_PER_LANE;
  const unsigned ats = pfq_lane_ats (text, bytes, line_start, n_lines, j0);
  unsigned cnt_pack, all;
  const unsigned map = pfq_lane_map (ats, n_lines, j0, &cnt_pack);
  int state = pfq_map_apply (pfq_block_scan_map < PFQ_BLOCK > (map, ws, &all), (int) in.x);
  unsigned k = in.y + pfq_block_scan_sum < PFQ_BLOCK > ((cnt_pack >> (3 * state)) & 7u, ws, &all);
#pragma unroll
  for (unsigned q = 0; q < PFQ_LINES_PER_LANE; q++)
    if (j0 + q < n_lines)
      {
        if (state == PFQ_SEQ)
          {
            if (k < max_records)
              {
                const unsigned s = line_start[j0 + q], e = line_start[j0 + q + 1];      // e - 1: the line's '\n'
                long skip = 0, sl = 0;
                int cls = PFQ_END_BAD_LEN;
                if (s < e && e <= bytes)        // (always: a line start lies behind the '\n' before it)
                  {
                    sl = pfq_read_len ((long) (e - 1u - s), trim_start, trim_end, &skip);
                    cls = pfq_classify (sl, first_mate, PEMAP_MIN_READ, PEMAP_MAX_READ);
                  }
                rec_next[k] = e;
                if (cls == PFQ_COUNTS)
                  {
                    rec_off[k] = s + (unsigned) skip;
                    rec_len[k] = (int) sl;
                  }
                else
                  atomicMin (&ctl->stop, (unsigned long long) k << 32 | (cls == PFQ_END_BAD_LEN ? PFQ_STOP_BAD_LEN : 0u) | (unsigned) sl);
              }
            k++;
          }
        state = pfq_next (state, (int) ((ats >> q) & 1u));
      }
}

// ---- 4. rows: records [0, n) into rows[i * stride], len_out[i]; PFQ_ROW_LANES lanes a record
__global__ void __launch_bounds__ (PFQ_BLOCK) pfq_rows_kernel (const uint8_t * __restrict__ text, unsigned bytes, const unsigned *__restrict__ rec_off, const int *__restrict__ rec_len,
                                                               unsigned n, unsigned stride, uint8_t * __restrict__ rows, int *__restrict__ len_out)
{
  const unsigned i = blockIdx.x * (PFQ_BLOCK / PFQ_ROW_LANES) + threadIdx.x / PFQ_ROW_LANES, lane = threadIdx.x % PFQ_ROW_LANES;
  if (i >= n)
    return;
  const unsigned off = rec_off[i];
  int sl = rec_len[i];
  if (sl < 0 || (unsigned) sl > stride || off > bytes || (unsigned) sl > bytes - off)
    sl = 0;                     // (never: stage 3 made both from the text's own line starts, and the host refuses a stride below PEMAP_MAX_READ)
  uint8_t *row = rows + (size_t) i * stride;
  for (unsigned b = lane; b < (unsigned) sl; b += PFQ_ROW_LANES)
    row[b] = text[off + b];
  if (lane == 0)
    len_out[i] = sl;
}
