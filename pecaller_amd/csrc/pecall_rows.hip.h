// pecall_rows.hip.h -- the rows of <outfile>.base.gz made on the device from the resident results of a call (pecall_dev_sites_base_text).
//
// The host loop this stands for (emit_rows of pecaller_main.c; in the reference the per-sample gzprintf loop, pecaller.c:1760-1775)
// writes per column "\n<contig>\t<pos>\t<ref>" and per sample "\t<call>\t<posterior>".  A column whose posteriors are all exactly 1
// -- nearly every column of real data -- is a fixed template, "\t<call>\t1" per sample (pecall_row_len.h).  Over the whole-run arrays
// d_call / d_type / d_post of the last call:
//   1. pcr_len_kernel      a wave per column: length 0 where the caller skipped the column (type < 0); length 0 and the HOLE flag
//                          where some sample's posterior is not exactly 1 (the predicate of pcs_sparse_kernel, over the same
//                          array: the host formats those rows); else the template's length
//   2. pcr_scan_*          exclusive prefix sum of the lengths into 64-bit byte offsets, and of the HOLE flags into the ascending
//                          list (column, byte offset at which the host's row belongs): per block of PCR_SCAN_TILE columns a sum,
//                          one block over the sums, then every block again for its columns
//   3. pcr_fill_kernel     a workgroup per run of R columns, whose text is one contiguous byte range: the run's bytes are put
//                          together in LDS -- the sample fields as aligned 32-bit words (a lane per sample: its own field and its
//                          left neighbour's, shifted by the row's byte phase), the heads and the few bytes that share a word with
//                          them by a lane per row -- and streamed out as aligned 16-byte stores, byte stores at the two ragged ends
// Contig numbers and positions are checked by the host before they come here (pecall_capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pecall_row_len.h"

#define PCR_BLOCK 256
#define PCR_SCAN_TILE (PCR_BLOCK * 4)   // columns a block of the scan takes: four lengths (16 bytes) per thread
#define PCR_TOP 1024                    // threads of the one block that scans the block sums, PCR_TOP at a time with a carry
#define PCR_HOLE 0x80000000u            // in a column's length word: the host formats this row
#define PCR_MAX_NAME 1024u              // bytes of a contig name
#define PCR_TILE_BUDGET 32768u          // LDS bytes of a run's text
#define PCR_MAX_RUN 64                  // columns per workgroup of the fill kernel at most (one lane of wave 0 per row's head)

struct PcrCtl
{
  unsigned long long n_text, n_holes;
};

// longest row of a call: 10 digits, the longest name
static inline unsigned pcr_row_max (unsigned max_name, int indiv)
{
  return (unsigned) pcr_row_len (max_name, PCR_MAX_POS, (uint32_t) indiv);
}

// columns per workgroup of pcr_fill_kernel: R rows and the 15 bytes in front of an unaligned start fit PCR_TILE_BUDGET
// (64 up to 126 samples, 15 at 512 with a short name, 10 with the longest)
static inline int pcr_fill_run (unsigned max_name, int indiv)
{
  const unsigned r = (PCR_TILE_BUDGET - 16u) / pcr_row_max (max_name, indiv);
  return r > PCR_MAX_RUN ? PCR_MAX_RUN : (int) r;
}

static inline unsigned pcr_fill_tile_bytes (unsigned max_name, int indiv)
{
  return ((unsigned) pcr_fill_run (max_name, indiv) * pcr_row_max (max_name, indiv) + 16u + 15u) & ~15u;
}

// "\t<call>\t1" as a little-endian word; a call of 14 or more prints 'N' (GEN = "ACGTDIMRWSYKEHN", int_to_gen, pecaller.c:2910-2943)
__device__ __forceinline__ unsigned pcr_field (int8_t call)
{
  const unsigned c = (unsigned) (uint8_t) call < 14u ? (unsigned) (uint8_t) call : 14u;
  const unsigned long long gen = c < 8u ? 0x524D494454474341ull : 0x004E48454B595357ull;
  const unsigned letter = (unsigned) (gen >> (8u * (c & 7u))) & 0xffu;
  return 0x31090009u | (letter << 8);
}

__global__ void __launch_bounds__ (PCR_BLOCK) pcr_len_kernel (const int8_t * __restrict__ type, const double *__restrict__ post, const int32_t * __restrict__ contig,
                                                              const uint32_t * __restrict__ pos, const uint32_t * __restrict__ name_off, long n, int N,
                                                              unsigned *__restrict__ len)
{
  const int lane = threadIdx.x & 63;
  const long wave = ((long) blockIdx.x * PCR_BLOCK + threadIdx.x) >> 6, n_waves = ((long) gridDim.x * PCR_BLOCK) >> 6;
  for (long c = wave; c < n; c += n_waves)
    {
      unsigned v = 0u;
      if (type[c] >= 0)
        {
          bool any = false;
          for (int i = lane; i < N; i += 64)
            any = any || post[c * N + i] != 1.0;
          if (__any (any))
            v = PCR_HOLE;
          else
            {
              const int ct = contig[c];
              v = (unsigned) pcr_row_len (name_off[ct + 1] - name_off[ct], pos[c], (uint32_t) N);
            }
        }
      if (lane == 0)
        len[c] = v;
    }
}

// len: padded with zeros to a whole number of PCR_SCAN_TILE
__global__ void __launch_bounds__ (PCR_BLOCK) pcr_scan_reduce_kernel (const uint4 * __restrict__ len4, unsigned long long *__restrict__ sum_bytes, unsigned *__restrict__ sum_holes)
{
  __shared__ unsigned part[2][PCR_BLOCK / 64];
  const uint4 v = len4[(size_t) blockIdx.x * PCR_BLOCK + threadIdx.x];
  // (a block's bytes: 1,024 rows of ~3 KB at most)
  unsigned b = (v.x & ~PCR_HOLE) + (v.y & ~PCR_HOLE) + (v.z & ~PCR_HOLE) + (v.w & ~PCR_HOLE);
  unsigned h = (v.x >> 31) + (v.y >> 31) + (v.z >> 31) + (v.w >> 31);
  for (int o = 32; o > 0; o >>= 1)
    {
      b += __shfl_down (b, o, 64);
      h += __shfl_down (h, o, 64);
    }
  if ((threadIdx.x & 63) == 0)
    {
      part[0][threadIdx.x >> 6] = b;
      part[1][threadIdx.x >> 6] = h;
    }
  __syncthreads ();
  if (threadIdx.x == 0)
    {
      sum_bytes[blockIdx.x] = (unsigned long long) part[0][0] + part[0][1] + part[0][2] + part[0][3];
      sum_holes[blockIdx.x] = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    }
}

// one block: the block sums become the blocks' first byte and first hole, their totals the text's length and the number of holes
__global__ void __launch_bounds__ (PCR_TOP) pcr_scan_top_kernel (unsigned long long *__restrict__ sum_bytes, unsigned *__restrict__ sum_holes, unsigned nb,
                                                                 PcrCtl * __restrict__ ctl)
{
  __shared__ unsigned long long sb[PCR_TOP];
  __shared__ unsigned sh[PCR_TOP];
  const unsigned t = threadIdx.x;
  unsigned long long carry_b = 0ull;
  unsigned carry_h = 0u;
  for (unsigned base = 0; base < nb; base += PCR_TOP)
    {
      const unsigned long long own_b = base + t < nb ? sum_bytes[base + t] : 0ull;
      const unsigned own_h = base + t < nb ? sum_holes[base + t] : 0u;
      sb[t] = own_b;
      sh[t] = own_h;
      __syncthreads ();
      for (unsigned o = 1; o < PCR_TOP; o <<= 1)
        {
          const unsigned long long add_b = t >= o ? sb[t - o] : 0ull;
          const unsigned add_h = t >= o ? sh[t - o] : 0u;
          __syncthreads ();
          sb[t] += add_b;
          sh[t] += add_h;
          __syncthreads ();
        }
      if (base + t < nb)
        {
          sum_bytes[base + t] = carry_b + sb[t] - own_b;
          sum_holes[base + t] = carry_h + sh[t] - own_h;
        }
      carry_b += sb[PCR_TOP - 1];
      carry_h += sh[PCR_TOP - 1];
      __syncthreads ();         // (everyone has the carry before the next piece overwrites it)
    }
  if (t == 0)
    {
      ctl->n_text = carry_b;
      ctl->n_holes = carry_h;
    }
}

// every padded column's byte offset (off[n] = the text's length: n lies inside the padding), and the list of holes
__global__ void __launch_bounds__ (PCR_BLOCK) pcr_scan_apply_kernel (const uint4 * __restrict__ len4, const unsigned long long *__restrict__ block_bytes,
                                                                     const unsigned *__restrict__ block_holes, unsigned long long *__restrict__ off,
                                                                     uint32_t * __restrict__ hole_site, unsigned long long *__restrict__ hole_at)
{
  __shared__ unsigned sb[PCR_BLOCK], sh[PCR_BLOCK];
  const unsigned t = threadIdx.x;
  const uint4 v = len4[(size_t) blockIdx.x * PCR_BLOCK + t];
  const unsigned w[4] = { v.x, v.y, v.z, v.w };
  const unsigned own_b = (v.x & ~PCR_HOLE) + (v.y & ~PCR_HOLE) + (v.z & ~PCR_HOLE) + (v.w & ~PCR_HOLE);
  const unsigned own_h = (v.x >> 31) + (v.y >> 31) + (v.z >> 31) + (v.w >> 31);
  sb[t] = own_b;
  sh[t] = own_h;
  __syncthreads ();
  for (unsigned o = 1; o < PCR_BLOCK; o <<= 1)
    {
      const unsigned add_b = t >= o ? sb[t - o] : 0u, add_h = t >= o ? sh[t - o] : 0u;
      __syncthreads ();
      sb[t] += add_b;
      sh[t] += add_h;
      __syncthreads ();
    }
  unsigned long long at = block_bytes[blockIdx.x] + (sb[t] - own_b);
  unsigned hole = block_holes[blockIdx.x] + (sh[t] - own_h);
  const size_t col0 = ((size_t) blockIdx.x * PCR_BLOCK + t) * 4u;
#pragma unroll
  for (int k = 0; k < 4; k++)
    {
      off[col0 + k] = at;
      if (w[k] & PCR_HOLE)
        {
          hole_site[hole] = (uint32_t) (col0 + k);
          hole_at[hole] = at;
          hole++;
        }
      at += w[k] & ~PCR_HOLE;
    }
}

// A workgroup per run of R columns; dynamic LDS: tile_bytes of text, then R words (where each row's sample fields begin).  The tile's
// byte 0 stands for the 16-byte boundary at or in front of the run's first byte of `text`, so that a 16-byte piece of the tile is an
// aligned 16-byte piece of `text`.
__global__ void __launch_bounds__ (PCR_BLOCK) pcr_fill_kernel (const unsigned *__restrict__ len, const unsigned long long *__restrict__ off, const int8_t * __restrict__ call,
                                                               const int32_t * __restrict__ contig, const uint32_t * __restrict__ pos, const char *__restrict__ ref_char,
                                                               const char *__restrict__ names, const uint32_t * __restrict__ name_off, long n, int N, int R,
                                                               unsigned tile_bytes, char *__restrict__ text)
{
  extern __shared__ uint4 pcr_lds[];
  char *tile = (char *) pcr_lds;
  unsigned *fields_at = (unsigned *) (tile + tile_bytes);       // [R]; ~0: the row is not in the text (skipped, or a hole)
  const unsigned t = threadIdx.x;
  const long c0 = (long) blockIdx.x * R;
  const int m = n - c0 < (long) R ? (int) (n - c0) : R;
  const unsigned long long b0 = off[c0], b1 = off[c0 + m];
  if (b1 == b0)
    return;                     // (no row of the run is in the text)
  const unsigned long long a0 = b0 & ~15ull;
  // ---- the heads, a lane per row: '\n' name '\t' position '\t' letter; and the sample bytes that share a word with a head -- those
  //      in front of the first word boundary of the fields, and those behind the last
  if (t < (unsigned) m)
    {
      const long c = c0 + t;
      const unsigned l = len[c] & ~PCR_HOLE;
      const unsigned r0 = (unsigned) (off[c] - a0);
      unsigned s0 = ~0u;
      if (l != 0u && r0 + l <= tile_bytes)
        {
          const int ct = contig[c];
          const unsigned nb = name_off[ct], nl = name_off[ct + 1] - nb;
          const uint32_t p = pos[c];
          const int nd = pcr_pos_digits (p);
          char *w = tile + r0;
          *w++ = '\n';
          // (a byte at a time: the row begins at any byte of the tile, and the name at any byte of the blob)
#pragma clang loop vectorize(disable) unroll(disable)
          for (unsigned k = 0; k < nl; k++)
            *w++ = names[nb + k];
          *w++ = '\t';
          pcr_put_digits (w, p, nd);
          w += nd;
          *w++ = '\t';
          *w++ = ref_char[c];
          s0 = (unsigned) (w - tile);
          const unsigned ph = s0 & 3u;
          if (ph)
            {
              const unsigned first = pcr_field (call[c * N]), last = pcr_field (call[c * N + (N - 1)]);
              for (unsigned x = 0; x < 4u - ph; x++)
                tile[s0 + x] = (char) (first >> (8u * x));
              for (unsigned x = 4u - ph; x < 4u; x++)
                tile[s0 + 4u * (unsigned) (N - 1) + x] = (char) (last >> (8u * x));
            }
        }
      fields_at[t] = s0;
    }
  __syncthreads ();
  // ---- the sample fields, a lane per sample: the aligned word k of a row's fields holds the last ph bytes of field k - 1 and the
  //      first 4 - ph of field k (ph = the fields' byte phase; 0: the word is field k).  Thread index = index into the run's calls.
  {
    unsigned q = t / (unsigned) N, i = t % (unsigned) N;
    const unsigned dq = PCR_BLOCK / (unsigned) N, di = PCR_BLOCK % (unsigned) N;
    const int8_t *cl = call + c0 * N;
    for (unsigned k = t; k < (unsigned) m * (unsigned) N; k += PCR_BLOCK)
      {
        const unsigned s0 = fields_at[q];
        const unsigned ph = s0 & 3u;
        if (s0 != ~0u && (i > 0u || ph == 0u))
          {
            const unsigned long long two = ((unsigned long long) pcr_field (cl[k]) << 32) | (i > 0u ? pcr_field (cl[k - 1]) : 0u);
            *(unsigned *) (tile + (s0 & ~3u) + 4u * i) = (unsigned) (two >> (8u * (4u - ph)));
          }
        q += dq;
        i += di;
        if (i >= (unsigned) N)
          {
            i -= (unsigned) N;
            q++;
          }
      }
  }
  __syncthreads ();
  // ---- out: whole 16-byte pieces inside [lo, hi), bytes in front of the first and behind the last
  const unsigned lo = (unsigned) (b0 - a0), hi = (unsigned) (b1 - a0);
  const unsigned first16 = (lo + 15u) & ~15u, last16 = hi & ~15u;
  char *g = text + a0;
  for (unsigned k = first16 / 16u + t; k < last16 / 16u; k += PCR_BLOCK)
    ((uint4 *) g)[k] = pcr_lds[k];
  const unsigned head_end = first16 < hi ? first16 : hi;
  if (lo + t < head_end)
    g[lo + t] = tile[lo + t];
  if (last16 >= first16 && last16 + t < hi)
    g[last16 + t] = tile[last16 + t];
}
