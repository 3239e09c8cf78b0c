// pecall_gz.hip.h -- the device-made text of <outfile>.base.gz (pecall_rows.hip.h) deflated on the device into gzip members
// (pecall_dev_sites_base_gz).  The rule -- pieces, parse, codes, CRC -- is pecall_gz_rule.h; its serial statement pcg_encode_piece is
// what these kernels reproduce byte for byte.  Over the text in d_text, the columns' offsets and the holes of pcr_scan_apply_kernel:
//   1. pcg_runs_kernel     a thread per run (the text between two holes, or between a text end and a hole): its number of pieces
//   2. pcg_scan_*          exclusive prefix sum of 64-bit values in place, hand-written as pcr_scan_* are: per block of PCG_SCAN_TILE
//                          values a sum, one block over the sums, then every block again for its values.  Over the runs' pieces it
//                          gives each run's first piece and the number of pieces; over the members' lengths, further down, each
//                          member's place in the packed array and the packed length
//   3. pcg_table_kernel    a thread per piece: its run by binary search over the runs' first pieces, its first byte and its length
//   4. pcg_deflate_kernel  a workgroup per piece, the piece and everything made of it in LDS: 16-byte loads; per byte the row distance
//                          D, then the two candidates' equality flags and their run lengths to the right (a thread per PCG_CHUNK
//                          bytes, the carries between chunks by one lane); one lane walks the token starts; a thread per few tokens
//                          takes their bit lengths, a block scan places them, LDS atomics put the bits into the member; the CRC-32
//                          from per-thread slice CRCs and a log-step combine; the member leaves for its slot -- a range of worst-case
//                          size at a place known beforehand -- as aligned 16-byte stores
//   5. pcg_pack_kernel     a workgroup per member: from its slot to its place in the packed array, aligned 16-byte stores between
//                          byte stores at the two ragged ends
//   6. pcg_holes_kernel    a thread per hole: the packed offset of the first member behind it
// An offset becomes an address only after a check against the text's length, the piece count or the slot area's size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pecall_gz_rule.h"

#define PCG_BLOCK 256
#define PCG_CHUNK (PCG_PIECE / PCG_BLOCK)       // bytes a thread of the deflate kernel takes: 28
#define PCG_SCAN_TILE (PCG_BLOCK * 4)
#define PCG_TOP 1024
#define PCG_SLOT_PITCH 64u      // slot b begins at (the piece's first byte + PCG_SLOT_PITCH * b) & ~15: room for the piece, the 23 bytes around it and the alignment
#define PCG_TILE16 ((PCG_PIECE + 15u + 15u) / 16u)      // 16-byte pieces of LDS for a piece that begins at any byte
#define PCG_OUT_WORDS ((PCG_MEMBER_MAX + 15u) / 16u * 4u)
#define PCG_NONE 0xffffffffu

static_assert (PCG_PIECE % PCG_BLOCK == 0 && PCG_PIECE <= 32768u, "a thread takes a whole number of bytes; every distance is a deflate distance");

struct PcgCtl
{
  unsigned long long n_pieces, n_gz;
};

static inline size_t pcg_slot_bytes (size_t n_text, size_t max_pieces)
{
  return n_text + (size_t) PCG_SLOT_PITCH * (max_pieces + 1) + 64;
}

__device__ __forceinline__ unsigned long long pcg_run_begin (const unsigned long long *__restrict__ hole_at, unsigned long long j)
{
  return j ? hole_at[j - 1] : 0ull;
}

__device__ __forceinline__ unsigned long long pcg_run_end (const unsigned long long *__restrict__ hole_at, unsigned long long j, unsigned long long n_holes,
                                                           unsigned long long n_text)
{
  return j < n_holes ? hole_at[j] : n_text;
}

// val: n_pad entries, n_pad a multiple of PCG_SCAN_TILE beyond the n_holes + 1 runs
__global__ void __launch_bounds__ (PCG_BLOCK) pcg_runs_kernel (const unsigned long long *__restrict__ hole_at, unsigned long long n_holes, unsigned long long n_text,
                                                               unsigned long long n_pad, unsigned long long *__restrict__ val)
{
  const unsigned long long j = (unsigned long long) blockIdx.x * PCG_BLOCK + threadIdx.x;
  if (j >= n_pad)
    return;
  unsigned long long v = 0ull;
  if (j <= n_holes)
    {
      const unsigned long long a = pcg_run_begin (hole_at, j), b = pcg_run_end (hole_at, j, n_holes, n_text);
      if (a <= b && b <= n_text)
        v = pcg_run_pieces (b - a);
    }
  val[j] = v;
}

__global__ void __launch_bounds__ (PCG_BLOCK) pcg_scan_reduce_kernel (const ulonglong4 * __restrict__ val4, unsigned long long *__restrict__ sum)
{
  __shared__ unsigned long long part[PCG_BLOCK / 64];
  const ulonglong4 v = val4[(size_t) blockIdx.x * PCG_BLOCK + threadIdx.x];
  unsigned long long s = v.x + v.y + v.z + v.w;
  for (int o = 32; o > 0; o >>= 1)
    s += __shfl_down (s, o, 64);
  if ((threadIdx.x & 63) == 0)
    part[threadIdx.x >> 6] = s;
  __syncthreads ();
  if (threadIdx.x == 0)
    sum[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// one block: the block sums become the blocks' first values, their total goes to *total
__global__ void __launch_bounds__ (PCG_TOP) pcg_scan_top_kernel (unsigned long long *__restrict__ sum, unsigned nb, unsigned long long *__restrict__ total)
{
  __shared__ unsigned long long sb[PCG_TOP];
  const unsigned t = threadIdx.x;
  unsigned long long carry = 0ull;
  for (unsigned base = 0; base < nb; base += PCG_TOP)
    {
      const unsigned long long own = base + t < nb ? sum[base + t] : 0ull;
      sb[t] = own;
      __syncthreads ();
      for (unsigned o = 1; o < PCG_TOP; o <<= 1)
        {
          const unsigned long long add = t >= o ? sb[t - o] : 0ull;
          __syncthreads ();
          sb[t] += add;
          __syncthreads ();
        }
      if (base + t < nb)
        sum[base + t] = carry + sb[t] - own;
      carry += sb[PCG_TOP - 1];
      __syncthreads ();
    }
  if (t == 0)
    *total = carry;
}

// in place: val[k] becomes the sum of the values in front of it
__global__ void __launch_bounds__ (PCG_BLOCK) pcg_scan_apply_kernel (ulonglong4 * __restrict__ val4, const unsigned long long *__restrict__ block_first)
{
  __shared__ unsigned long long sb[PCG_BLOCK];
  const unsigned t = threadIdx.x;
  const size_t at4 = (size_t) blockIdx.x * PCG_BLOCK + t;
  const ulonglong4 v = val4[at4];
  const unsigned long long own = v.x + v.y + v.z + v.w;
  sb[t] = own;
  __syncthreads ();
  for (unsigned o = 1; o < PCG_BLOCK; o <<= 1)
    {
      const unsigned long long add = t >= o ? sb[t - o] : 0ull;
      __syncthreads ();
      sb[t] += add;
      __syncthreads ();
    }
  ulonglong4 r;
  r.x = block_first[blockIdx.x] + (sb[t] - own);
  r.y = r.x + v.x;
  r.z = r.y + v.y;
  r.w = r.z + v.z;
  val4[at4] = r;
}

// run_first: the scanned piece counts, n_holes + 2 entries at least (run_first[n_holes + 1] = the number of pieces)
__global__ void __launch_bounds__ (PCG_BLOCK) pcg_table_kernel (const unsigned long long *__restrict__ hole_at, unsigned long long n_holes, unsigned long long n_text,
                                                                const unsigned long long *__restrict__ run_first, const PcgCtl * __restrict__ ctl,
                                                                unsigned long long max_pieces, unsigned long long *__restrict__ piece_at, unsigned *__restrict__ piece_len)
{
  const unsigned long long b = (unsigned long long) blockIdx.x * PCG_BLOCK + threadIdx.x;
  if (b >= max_pieces)
    return;
  unsigned long long at = 0ull;
  unsigned len = 0u;
  if (b < ctl->n_pieces)
    {
      // the last run j of 0 .. n_holes with run_first[j] <= b (runs without a piece share their successor's value)
      unsigned long long lo = 0ull, hi = n_holes + 1ull;
      while (hi - lo > 1ull)
        {
          const unsigned long long mid = lo + (hi - lo) / 2ull;
          if (run_first[mid] <= b)
            lo = mid;
          else
            hi = mid;
        }
      const unsigned long long r0 = pcg_run_begin (hole_at, lo), r1 = pcg_run_end (hole_at, lo, n_holes, n_text);
      const unsigned long long a = r0 + (b - run_first[lo]) * PCG_PIECE;
      if (r1 <= n_text && a < r1)
        {
          at = a;
          len = r1 - a < PCG_PIECE ? (unsigned) (r1 - a) : PCG_PIECE;
        }
    }
  piece_at[b] = at;
  piece_len[b] = len;
}

// A workgroup per piece.  text_alloc: bytes of `text` that may be read (a multiple of 16 beyond the text's length); slot_bytes: of `slots`.
__global__ void __launch_bounds__ (PCG_BLOCK) pcg_deflate_kernel (const char *__restrict__ text, unsigned long long n_text, unsigned long long text_alloc,
                                                                  const unsigned long long *__restrict__ piece_at, const unsigned *__restrict__ piece_len,
                                                                  const PcgCtl * __restrict__ ctl, unsigned char *__restrict__ slots, unsigned long long slot_bytes,
                                                                  unsigned long long *__restrict__ member_len)
{
  __shared__ uint4 tile4[PCG_TILE16];
  __shared__ uint4 out4[PCG_OUT_WORDS / 4];
  __shared__ uint16_t sd[PCG_PIECE], sa[PCG_PIECE], sb[PCG_PIECE];      // D, then a token's distance; candidate A's length, then a token's position; B's, then its length
  __shared__ unsigned crc_tab[256], w1[PCG_BLOCK], w2[PCG_BLOCK], w3[PCG_BLOCK], w4[PCG_BLOCK];
  __shared__ unsigned n_tok_s;
  const unsigned t = threadIdx.x;
  const unsigned long long b = blockIdx.x;
  if (b >= ctl->n_pieces)
    return;
  const unsigned long long p0 = piece_at[b];
  const unsigned n = piece_len[b];
  const unsigned long long a0 = p0 & ~15ull, slot_at = (p0 + (unsigned long long) PCG_SLOT_PITCH * b) & ~15ull;
  const unsigned lo = (unsigned) (p0 - a0);
  const unsigned n16 = (lo + n + 15u) / 16u;
  if (n == 0u || n > PCG_PIECE || p0 + n > n_text || a0 + 16ull * n16 > text_alloc || slot_at + ((PCG_HEAD + 5u + n + PCG_TAIL + 15u) & ~15u) > slot_bytes)
    {
      if (t == 0)
        member_len[b] = 0ull;
      return;
    }
  const uint8_t *T = (const uint8_t *) tile4 + lo;
  unsigned *out = (unsigned *) out4;
  // ---- the piece, the CRC table, a member of zeros
  for (unsigned k = t; k < n16; k += PCG_BLOCK)
    tile4[k] = ((const uint4 *) (text + a0))[k];
  crc_tab[t] = pcg_crc_table_entry (t);
  for (unsigned k = t; k < PCG_OUT_WORDS / 4u; k += PCG_BLOCK)
    out4[k] = make_uint4 (0u, 0u, 0u, 0u);
  __syncthreads ();
  const unsigned c0 = t * PCG_CHUNK < n ? t * PCG_CHUNK : n, c1 = c0 + PCG_CHUNK < n ? c0 + PCG_CHUNK : n;      // this thread's bytes
  // ---- the slice CRCs: slices of PCG_CHUNK bytes that end where the piece ends, so that only the first one is ragged
  unsigned crc;
  {
    const int e1 = (int) n - (int) (PCG_CHUNK * (PCG_BLOCK - 1u - t)), e0 = e1 - (int) PCG_CHUNK;
    const unsigned q0 = e0 > 0 ? (unsigned) e0 : 0u, q1 = e1 > 0 ? (unsigned) e1 : 0u;
    crc = pcg_crc_slice (crc_tab, T + q0, q1 - q0);
  }
  // ---- D: the last two row starts at or in front of each byte.  Per chunk its last two, one lane carries them across the chunks
  {
    unsigned last = PCG_NONE, second = PCG_NONE;
    for (unsigned i = c0; i < c1; i++)
      if (T[i] == '\n')
        {
          second = last;
          last = i;
        }
    w1[t] = last;
    w2[t] = second;
  }
  __syncthreads ();
  if (t == 0)
    {
      unsigned s = PCG_NONE, p = PCG_NONE;
      for (unsigned k = 0; k < PCG_BLOCK; k++)
        {
          const unsigned last = w1[k], second = w2[k];
          w3[k] = s;
          w4[k] = p;
          if (last != PCG_NONE)
            {
              p = second != PCG_NONE ? second : s;
              s = last;
            }
        }
    }
  __syncthreads ();
  {
    unsigned s = w3[t], p = w4[t];
    for (unsigned i = c0; i < c1; i++)
      {
        if (T[i] == '\n')
          {
            p = s;
            s = i;
          }
        sd[i] = (uint16_t) (p != PCG_NONE ? s - p : 0u);
      }
  }
  __syncthreads ();
  // ---- the candidates' flags, and how far each chunk's run of set flags reaches from its first byte
#define PCG_E4(i) ((i) >= 4u && T[i] == T[(i) - 4u])
#define PCG_ER(i) (sd[i] != 0u && T[i] == T[(i) - sd[i]])
#define PCG_STOPR(i) (!PCG_ER (i) || ((i) > 0u && sd[i] != sd[(i) - 1u]))
  {
    unsigned l4 = 0u, lr = 0u;
    while (c0 + l4 < c1 && PCG_E4 (c0 + l4))
      l4++;
    while (c0 + lr < c1 && !PCG_STOPR (c0 + lr))
      lr++;
    w1[t] = l4;
    w2[t] = lr;
  }
  __syncthreads ();
  // (one lane each: the run length at the first byte of the chunk to the right)
  if (t == 0 || t == 64)
    {
      unsigned *lead = t == 0 ? w1 : w2, *in = t == 0 ? w3 : w4;
      unsigned next = 0u;
      for (int k = PCG_BLOCK - 1; k >= 0; k--)
        {
          const unsigned k0 = (unsigned) k * PCG_CHUNK < n ? (unsigned) k * PCG_CHUNK : n, k1 = k0 + PCG_CHUNK < n ? k0 + PCG_CHUNK : n;
          in[k] = next;
          next = lead[k] == k1 - k0 ? k1 - k0 + next : lead[k];
        }
    }
  __syncthreads ();
  {
    unsigned r4 = w3[t], rr = w4[t];
    for (unsigned i = c1; i-- > c0;)
      {
        r4 = PCG_E4 (i) ? r4 + 1u : 0u;
        sa[i] = (uint16_t) r4;
        sb[i] = (uint16_t) (PCG_ER (i) ? 1u + rr : 0u);
        rr = PCG_STOPR (i) ? 0u : 1u + rr;
      }
  }
  __syncthreads ();
  // ---- the greedy walk over the token starts.  Token k lies at or in front of byte i: its record takes the side arrays' entry k
  if (t == 0)
    {
      unsigned k = 0u;
      for (unsigned i = 0u; i < n;)
        {
          const unsigned room = n - i < PCG_MAX_MATCH ? n - i : PCG_MAX_MATCH;
          const unsigned l4 = sa[i] < room ? sa[i] : room, lr = sb[i] < room ? sb[i] : room;
          unsigned dist;
          const unsigned len = pcg_choose (l4, lr, sd[i], &dist);
          sa[k] = (uint16_t) i;
          sb[k] = (uint16_t) len;
          sd[k] = (uint16_t) dist;
          k++;
          i += len;
        }
      n_tok_s = k;
    }
  __syncthreads ();
  // ---- the tokens' bits: a thread per `per` tokens, a block scan of the threads' sums
  const unsigned n_tok = n_tok_s;
  const unsigned per = (n_tok + PCG_BLOCK - 1u) / PCG_BLOCK;
  const unsigned k0 = t * per < n_tok ? t * per : n_tok, k1 = k0 + per < n_tok ? k0 + per : n_tok;
  unsigned own = 0u;
  for (unsigned k = k0; k < k1; k++)
    {
      int nb;
      pcg_token (sb[k], sd[k], T[sa[k]], &nb);
      own += (unsigned) nb;
    }
  w1[t] = own;
  __syncthreads ();
  for (unsigned o = 1; o < PCG_BLOCK; o <<= 1)
    {
      const unsigned add = t >= o ? w1[t - o] : 0u;
      __syncthreads ();
      w1[t] += add;
      __syncthreads ();
    }
  const unsigned fixed = pcg_fixed_bytes (w1[PCG_BLOCK - 1]);
  const bool stored = fixed >= 5u + n;
  const unsigned body = stored ? 5u + n : fixed;
  uint8_t *outb = (uint8_t *) out;
  if (stored)
    {
      if (t < 5u)
        outb[PCG_HEAD + t] = t == 0u ? 1u : t == 1u ? (uint8_t) n : t == 2u ? (uint8_t) (n >> 8) : t == 3u ? (uint8_t) ~n : (uint8_t) (~n >> 8);
      for (unsigned i = t; i < n; i += PCG_BLOCK)
        outb[PCG_HEAD + 5u + i] = T[i];
    }
  else
    {
      unsigned at = 8u * PCG_HEAD + 3u + (w1[t] - own);
      if (t == 0)
        atomicOr (&out[PCG_HEAD / 4u], 3u << (8u * (PCG_HEAD % 4u)));   // final block, fixed codes
      for (unsigned k = k0; k < k1; k++)
        {
          int nb;
          const unsigned long long v = (unsigned long long) pcg_token (sb[k], sd[k], T[sa[k]], &nb) << (at & 31u);
          atomicOr (&out[at >> 5], (unsigned) v);
          if (v >> 32)
            atomicOr (&out[(at >> 5) + 1u], (unsigned) (v >> 32));
          at += (unsigned) nb;
        }
    }
  // ---- the piece's CRC: at step o a slice group takes in the group of o slices to its right, all whole (or the left one is empty)
  w2[t] = crc;
  __syncthreads ();
  {
    unsigned xp = pcg_xpow8 (PCG_CHUNK);
    for (unsigned o = 1; o < PCG_BLOCK; o <<= 1)
      {
        if ((t & (2u * o - 1u)) == 0u)
          w2[t] = pcg_mulmod (xp, w2[t]) ^ w2[t + o];
        xp = pcg_mulmod (xp, xp);
        __syncthreads ();
      }
  }
  // ---- the ten bytes in front, the eight behind; out
  if (t < PCG_HEAD)
    outb[t] = pcg_head_byte (t);
  if (t >= 64u && t < 64u + PCG_TAIL)
    {
      const unsigned k = t - 64u;
      outb[PCG_HEAD + body + k] = (uint8_t) ((k < 4u ? w2[0] : n) >> (8u * (k & 3u)));
    }
  __syncthreads ();
  const unsigned m = PCG_HEAD + body + PCG_TAIL;
  uint4 *slot4 = (uint4 *) (slots + slot_at);
  for (unsigned k = t; k < (m + 15u) / 16u; k += PCG_BLOCK)
    slot4[k] = out4[k];
  if (t == 0)
    member_len[b] = m;
#undef PCG_E4
#undef PCG_ER
#undef PCG_STOPR
}

// member_at: the scanned lengths, one entry beyond the pieces at least.  A workgroup per member.
__global__ void __launch_bounds__ (PCG_BLOCK) pcg_pack_kernel (const unsigned char *__restrict__ slots, unsigned long long slot_bytes,
                                                               const unsigned long long *__restrict__ piece_at, const unsigned long long *__restrict__ member_at,
                                                               const PcgCtl * __restrict__ ctl, unsigned char *__restrict__ gz, unsigned long long gz_bytes)
{
  const unsigned t = threadIdx.x;
  const unsigned long long b = blockIdx.x;
  if (b >= ctl->n_pieces)
    return;
  const unsigned long long g0 = member_at[b], g1 = member_at[b + 1], slot_at = (piece_at[b] + (unsigned long long) PCG_SLOT_PITCH * b) & ~15ull;
  if (g1 <= g0 || g1 - g0 > PCG_MEMBER_MAX || g1 > gz_bytes || slot_at + ((g1 - g0 + 15ull) & ~15ull) + 16ull > slot_bytes)
    return;
  const unsigned m = (unsigned) (g1 - g0);
  const unsigned char *src = slots + slot_at;
  unsigned char *dst = gz + g0;
  // dst + head is the first 16-byte boundary; whole 16-byte pieces up to `last`
  const unsigned head = (unsigned) ((16ull - (g0 & 15ull)) & 15ull) < m ? (unsigned) ((16ull - (g0 & 15ull)) & 15ull) : m;
  const unsigned whole = (m - head) / 16u;
  if (t < head)
    dst[t] = src[t];
  const unsigned sh = 8u * (head & 3u);
  const unsigned *sw = (const unsigned *) src + head / 4u;
  for (unsigned k = t; k < whole; k += PCG_BLOCK)
    {
      unsigned w[5];
#pragma unroll
      for (int x = 0; x < 5; x++)
        w[x] = sw[4u * k + x];          // (the fifth word lies inside the slot area: 16 bytes are kept beyond a slot's last piece)
      uint4 r;
      if (sh)
        r = make_uint4 ((w[0] >> sh) | (w[1] << (32u - sh)), (w[1] >> sh) | (w[2] << (32u - sh)), (w[2] >> sh) | (w[3] << (32u - sh)), (w[3] >> sh) | (w[4] << (32u - sh)));
      else
        r = make_uint4 (w[0], w[1], w[2], w[3]);
      ((uint4 *) (dst + head))[k] = r;
    }
  const unsigned done = head + 16u * whole;
  if (done + t < m)
    dst[done + t] = src[done + t];
}

// the host's row of hole k belongs in front of the first member of run k + 1
__global__ void __launch_bounds__ (PCG_BLOCK) pcg_holes_kernel (const unsigned long long *__restrict__ run_first, const unsigned long long *__restrict__ member_at,
                                                                unsigned long long n_holes, unsigned long long max_pieces, unsigned long long *__restrict__ hole_gz_at)
{
  const unsigned long long k = (unsigned long long) blockIdx.x * PCG_BLOCK + threadIdx.x;
  if (k >= n_holes)
    return;
  const unsigned long long b = run_first[k + 1];
  hole_gz_at[k] = member_at[b <= max_pieces ? b : max_pieces];
}
