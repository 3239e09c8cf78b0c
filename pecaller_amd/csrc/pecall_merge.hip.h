// pecall_merge.hip.h -- pileup columns built on the device from per-sample record streams (pecall_dev_sites_stage_records).
//
// The host walk this stands for (merge_streams / merge_count / merge_columns of pecaller_main.c; in the reference find_lowest and the
// per-column loop, pecaller.c:865-923, 1820-1833) takes the records {u32 pos; u16 A,C,G,T,Del,Ins} of every sample over a range of
// positions [p0, p0 + span) and makes a column of every position at which some sample has a record: that sample's six counts where
// it has one, zeros where it has none.  Here, over records that lie on the device:
//   1. pcm_mark_kernel     a thread per record: the record is checked (inside the range, beyond its predecessor) and its slot marked
//                          with a plain byte store; a bad record marks nothing and leaves the lowest (sample, index) in PcmCtl
//   2. pcm_scan_*          exclusive prefix sum of the marks: per block of PCM_SCAN_TILE slots a count (16-byte loads), one block
//                          over the counts, then every block again for its slots' columns: col_of_slot, col_slot, and the columns'
//                          reference and chromosome bytes
//   3. pcm_tile_kernel     a workgroup per run of S slots and all samples: the run's tile [S][indiv][6] is zeroed in LDS, every
//                          sample's records of the run (found by bisection over its positions, loaded along the stream) dropped into
//                          it, and the marked slots' rows written to the column array as whole rows
// A record's position becomes an address only after the check of stage 1 has passed for it: stage 3 takes a record only if its
// position lies inside the workgroup's own run, and does nothing at all when stage 1 found a bad record.
//
// The guided form (pecall_dev_sites_stage_records_guided; the guide-file loop of the reference, pecaller.c:941-1039): the columns are
// the positions of a list of intervals, covered or not, not the records' positions.  Only stage 1 differs:
//   1a. pcm_guide_marks_kernel   a thread per 16 slots of the padded span: the marks and the chromosome bytes of its slots from the
//                                interval list, a 16-byte store each (the zeros too: no memset of the marks)
//   1b. pcm_mark_kernel          with marks = nullptr: every record checked as before, no mark stored
// Stages 2 and 3 run unchanged on those marks.  A record at a slot outside every interval lands in the tile of stage 3 and stays there
// (its slot has no column); a run whose marked slots hold no record is written as the zeros it was cleared to.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PCM_BLOCK 256
#define PCM_SCAN_TILE (PCM_BLOCK * 16)  // slots a block of the scan takes: 16 mark bytes per thread
#define PCM_MAX_SPAN (1u << 22)
#define PCM_MAX_SCAN_BLOCKS (PCM_MAX_SPAN / PCM_SCAN_TILE)      // 1024: one block scans the block counts
#define PCM_NO_BAD 0xffffffffffffffffull
#define PCM_BAD_SHIFT 48                // PcmCtl.bad = sample << 48 | record index

struct PcmCtl
{
  unsigned long long bad;       // lowest (sample, record index) that is out of order or out of range; PCM_NO_BAD: none
  unsigned n_cols, pad;
};

// slots per workgroup of pcm_tile_kernel: S x indiv x 12 bytes of LDS (24 KB at 64, 128 and 256 samples, 48 KB at 512)
static inline int pcm_tile_slots (int indiv)
{
  return indiv <= 64 ? 32 : indiv <= 128 ? 16 : 8;
}

// index of the letter in "ACGTDIMRWSYKEHN" (gen_to_int, pecaller.c:2869-2907), 255 for any other byte
__device__ __forceinline__ unsigned pcm_ref_code (unsigned char c)
{
  switch (c)
    {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    case 'D': return 4;
    case 'I': return 5;
    case 'M': return 6;
    case 'R': return 7;
    case 'W': return 8;
    case 'S': return 9;
    case 'Y': return 10;
    case 'K': return 11;
    case 'E': return 12;
    case 'H': return 13;
    case 'N': return 14;
    default: return 255;
    }
}

// grid (x, indiv): the records of sample blockIdx.y, a thread each; marks = nullptr: the check alone (the guided form)
__global__ void __launch_bounds__ (PCM_BLOCK) pcm_mark_kernel (const uint4 * __restrict__ recs, const unsigned long long *__restrict__ rec_off, unsigned p0, unsigned span,
                                                               uint8_t * __restrict__ marks, PcmCtl * __restrict__ ctl)
{
  const unsigned i = blockIdx.y;
  const unsigned long long b = rec_off[i], n = rec_off[i + 1] - b;
  const unsigned *pos = (const unsigned *) (recs + b);  // record j's position: pos[4 j]
  for (unsigned long long j = (unsigned long long) blockIdx.x * PCM_BLOCK + threadIdx.x; j < n; j += (unsigned long long) gridDim.x * PCM_BLOCK)
    {
      const unsigned p = pos[4 * j];
      bool ok = p >= p0 && p - p0 < span;
      if (ok && j > 0)
        ok = p > pos[4 * (j - 1)];
      if (ok)
        {
          if (marks)
            marks[p - p0] = 1;  // (every writer of a slot stores the same byte)
        }
      else
        atomicMin (&ctl->bad, ((unsigned long long) i << PCM_BAD_SHIFT) | j);
    }
}

// The guided form's marks.  Intervals k = 0 .. n_iv - 1 take the slots [iv_first[k], iv_first[k] + iv_count[k]): ascending, disjoint,
// inside the span and none empty (checked on the host: they become addresses).  A thread per 16 slots of the padded span: it finds the
// first interval that ends beyond its first slot by bisection (22 steps at most; the list is a few MB at most and lies in L2), then walks
// its 16 slots and the list together -- an interval holds a slot at least, so one step along the list per slot is enough -- and
// composes the 16 mark bytes and the 16 chromosome bytes in registers.  Two 16-byte stores a thread, consecutive along the wave,
// whatever the intervals' lengths; slots outside every interval, the padding among them, get zeros.  iv_chrom: nullptr = 0.
__global__ void __launch_bounds__ (PCM_BLOCK) pcm_guide_marks_kernel (const unsigned *__restrict__ iv_first, const unsigned *__restrict__ iv_count,
                                                                      const uint8_t * __restrict__ iv_chrom, unsigned n_iv, unsigned n16, uint4 * __restrict__ marks16,
                                                                      uint4 * __restrict__ chrom16)
{
  const unsigned g = blockIdx.x * PCM_BLOCK + threadIdx.x;
  if (g >= n16)
    return;
  const unsigned s0 = g * 16u;
  unsigned lo = 0, hi = n_iv;
  while (lo < hi)
    {
      const unsigned mid = (lo + hi) >> 1;
      if (iv_first[mid] + iv_count[mid] <= s0)
        lo = mid + 1;
      else
        hi = mid;
    }
  unsigned k = lo, f = ~0u, e = ~0u, c = 0;     // the interval at hand: [f, e), its byte
  if (k < n_iv)
    {
      f = iv_first[k];
      e = f + iv_count[k];
      c = iv_chrom ? iv_chrom[k] : 0u;
    }
  unsigned m[4] = { 0u, 0u, 0u, 0u }, y[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
  for (int j = 0; j < 16; j++)
    {
      const unsigned slot = s0 + (unsigned) j;
      if (slot >= e)
        {
          k++;
          f = e = ~0u;
          if (k < n_iv)
            {
              f = iv_first[k];
              e = f + iv_count[k];
              c = iv_chrom ? iv_chrom[k] : 0u;
            }
        }
      if (slot >= f && slot < e)
        {
          m[j >> 2] |= 1u << (8 * (j & 3));
          y[j >> 2] |= c << (8 * (j & 3));
        }
    }
  marks16[g] = make_uint4 (m[0], m[1], m[2], m[3]);
  chrom16[g] = make_uint4 (y[0], y[1], y[2], y[3]);
}

// the marks of 16 slots as four words of 0 / 1 bytes: how many are set
__device__ __forceinline__ unsigned pcm_count16 (const uint4 v)
{
  return (unsigned) (__popc (v.x) + __popc (v.y) + __popc (v.z) + __popc (v.w));
}

// marks: padded with zeros to a whole number of PCM_SCAN_TILE
__global__ void __launch_bounds__ (PCM_BLOCK) pcm_scan_reduce_kernel (const uint4 * __restrict__ marks16, unsigned *__restrict__ block_sum)
{
  __shared__ unsigned part[PCM_BLOCK / 64];
  unsigned c = pcm_count16 (marks16[(size_t) blockIdx.x * PCM_BLOCK + threadIdx.x]);
  for (int o = 32; o > 0; o >>= 1)
    c += __shfl_down (c, o, 64);
  if ((threadIdx.x & 63) == 0)
    part[threadIdx.x >> 6] = c;
  __syncthreads ();
  if (threadIdx.x == 0)
    block_sum[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// one block: the block counts become the blocks' first columns, their total the number of columns (nb <= PCM_MAX_SCAN_BLOCKS)
__global__ void __launch_bounds__ (PCM_MAX_SCAN_BLOCKS) pcm_scan_top_kernel (unsigned *__restrict__ block_sum, unsigned nb, PcmCtl * __restrict__ ctl)
{
  __shared__ unsigned s[PCM_MAX_SCAN_BLOCKS];
  const unsigned t = threadIdx.x;
  const unsigned own = t < nb ? block_sum[t] : 0u;
  s[t] = own;
  __syncthreads ();
  for (unsigned o = 1; o < PCM_MAX_SCAN_BLOCKS; o <<= 1)
    {
      const unsigned add = t >= o ? s[t - o] : 0u;
      __syncthreads ();
      s[t] += add;
      __syncthreads ();
    }
  if (t < nb)
    block_sum[t] = s[t] - own;
  if (t == PCM_MAX_SCAN_BLOCKS - 1)
    ctl->n_cols = s[t];
}

// the columns of a block's marked slots; letters[ref_len], chrom_slot[span] or nullptr
__global__ void __launch_bounds__ (PCM_BLOCK) pcm_scan_apply_kernel (const uint4 * __restrict__ marks16, const unsigned *__restrict__ block_off, unsigned span,
                                                                     const uint8_t * __restrict__ letters, unsigned ref_len, const uint8_t * __restrict__ chrom_slot,
                                                                     unsigned *__restrict__ col_of_slot, unsigned *__restrict__ col_slot, uint8_t * __restrict__ dom,
                                                                     uint8_t * __restrict__ chromy)
{
  __shared__ unsigned s[PCM_BLOCK];
  const unsigned t = threadIdx.x;
  const uint4 v = marks16[(size_t) blockIdx.x * PCM_BLOCK + t];
  const unsigned own = pcm_count16 (v);
  s[t] = own;
  __syncthreads ();
  for (unsigned o = 1; o < PCM_BLOCK; o <<= 1)
    {
      const unsigned add = t >= o ? s[t - o] : 0u;
      __syncthreads ();
      s[t] += add;
      __syncthreads ();
    }
  if (own == 0)
    return;
  unsigned col = block_off[blockIdx.x] + s[t] - own;
  const unsigned w[4] = { v.x, v.y, v.z, v.w };
  const unsigned slot0 = (blockIdx.x * PCM_BLOCK + t) * 16u;
#pragma unroll
  for (int k = 0; k < 16; k++)
    if ((w[k >> 2] >> (8 * (k & 3))) & 1u)
      {
        const unsigned slot = slot0 + (unsigned) k;
        if (slot >= span)
          break;                // (the padding carries no marks)
        col_of_slot[slot] = col;
        col_slot[col] = slot;
        dom[col] = (uint8_t) (slot < ref_len ? pcm_ref_code (letters[slot]) : 255u);
        chromy[col] = chrom_slot ? chrom_slot[slot] : (uint8_t) 0;
        col++;
      }
}

// a workgroup per run of S slots; dynamic LDS: S x indiv x 12 bytes of tile, then S column numbers, then indiv first-record indices
__global__ void __launch_bounds__ (PCM_BLOCK) pcm_tile_kernel (const uint4 * __restrict__ recs, const unsigned long long *__restrict__ rec_off, int indiv, unsigned p0, unsigned span,
                                                               int S, const uint8_t * __restrict__ marks, const unsigned *__restrict__ col_of_slot,
                                                               const PcmCtl * __restrict__ ctl, uint16_t * __restrict__ sreads)
{
  extern __shared__ uint4 pcm_lds[];
  unsigned *tile = (unsigned *) pcm_lds;        // [S][indiv][3] words
  const unsigned row_words = (unsigned) indiv * 3u;
  unsigned *col_of = tile + (size_t) S * row_words;     // [S]: the slot's column, ~0 = no column
  unsigned *first = col_of + S;                 // [indiv]: the sample's first record at or beyond the run
  const unsigned t = threadIdx.x;
  if (ctl->bad != PCM_NO_BAD)
    return;
  const unsigned s0 = blockIdx.x * (unsigned) S;
  int marked = 0;
  if (t < (unsigned) S)
    {
      const unsigned slot = s0 + t;
      marked = slot < span && marks[slot];
      col_of[t] = marked ? col_of_slot[slot] : ~0u;
    }
  // The early exit is on the marks, not on records.  Without a guide a marked slot has a record and the two are one; in the guided
  // form a run without marked slots has no column to write, whatever records lie in it, and a run with marked slots goes on even when
  // no sample has a record in it: its rows are the zeros below, and they are written.
  if (!__syncthreads_or (marked))
    return;                     // (no column in the run)
  {
    const unsigned n16 = (unsigned) S * row_words / 4u; // (S is a multiple of 8: whole 16-byte pieces)
    const uint4 z = make_uint4 (0u, 0u, 0u, 0u);
    for (unsigned k = t; k < n16; k += PCM_BLOCK)
      pcm_lds[k] = z;
  }
  const unsigned long long base = (unsigned long long) p0 + s0;
  for (unsigned i = t; i < (unsigned) indiv; i += PCM_BLOCK)
    {
      // (positions ascend strictly from p0 on: record j lies at p0 + j or beyond, so the first one of the run is record s0 at the latest)
      const unsigned long long b = rec_off[i], n = rec_off[i + 1] - b;
      const unsigned *pos = (const unsigned *) (recs + b);
      unsigned long long lo = 0, hi = n < s0 ? n : s0;
      while (lo < hi)
        {
          const unsigned long long mid = (lo + hi) >> 1;
          if ((unsigned long long) pos[4 * mid] < base)
            lo = mid + 1;
          else
            hi = mid;
        }
      first[i] = (unsigned) lo;
    }
  __syncthreads ();
  // the records of the run: at most S per sample, S consecutive lanes along a sample's stream
  for (unsigned k = t; k < (unsigned) indiv * (unsigned) S; k += PCM_BLOCK)
    {
      const unsigned i = k / (unsigned) S, q = k % (unsigned) S;
      const unsigned long long b = rec_off[i], n = rec_off[i + 1] - b, j = (unsigned long long) first[i] + q;
      if (j < n)
        {
          const uint4 r = recs[b + j];
          const unsigned long long p = r.x;
          if (p >= base && p - base < (unsigned long long) S)
            {
              unsigned *dst = tile + ((unsigned) (p - base) * (unsigned) indiv + i) * 3u;
              dst[0] = r.y;
              dst[1] = r.z;
              dst[2] = r.w;
            }
        }
    }
  __syncthreads ();
  // the marked slots' rows, whole: 16 bytes a lane where a row is a multiple of that (samples a multiple of 4), else a word a lane
  if ((indiv & 3) == 0)
    {
      const unsigned row16 = row_words / 4u;
      uint4 *out = (uint4 *) sreads;
      for (unsigned k = t; k < (unsigned) S * row16; k += PCM_BLOCK)
        {
          const unsigned q = k / row16, x = k % row16, col = col_of[q];
          if (col != ~0u)
            out[(size_t) col * row16 + x] = pcm_lds[q * row16 + x];
        }
    }
  else
    {
      unsigned *out = (unsigned *) sreads;
      for (unsigned k = t; k < (unsigned) S * row_words; k += PCM_BLOCK)
        {
          const unsigned q = k / row_words, x = k % row_words, col = col_of[q];
          if (col != ~0u)
            out[(size_t) col * row_words + x] = tile[q * row_words + x];
        }
    }
}

// columns cols[0 .. n) (nullptr: 0 .. n - 1) of the staged arrays, packed: reads[n][indiv][6], then ref[n], then chrom[n]
__global__ void __launch_bounds__ (PCM_BLOCK) pcm_gather_kernel (const uint16_t * __restrict__ sreads, const uint8_t * __restrict__ dom, const uint8_t * __restrict__ chromy,
                                                                 long n_staged, int indiv, const unsigned *__restrict__ cols, unsigned long long n,
                                                                 unsigned *__restrict__ reads_out, uint8_t * __restrict__ ref_out, uint8_t * __restrict__ chrom_out)
{
  const unsigned row_words = (unsigned) indiv * 3u;
  const unsigned *in = (const unsigned *) sreads;
  for (unsigned long long q = blockIdx.x; q < n; q += gridDim.x)
    {
      const unsigned long long col = cols ? cols[q] : q;
      const bool ok = col < (unsigned long long) n_staged;
      for (unsigned x = threadIdx.x; x < row_words; x += PCM_BLOCK)
        reads_out[q * row_words + x] = ok ? in[col * row_words + x] : 0u;
      if (threadIdx.x == 0)
        {
          ref_out[q] = ok ? dom[col] : (uint8_t) 255;
          chrom_out[q] = ok ? chromy[col] : (uint8_t) 0;
        }
    }
}
