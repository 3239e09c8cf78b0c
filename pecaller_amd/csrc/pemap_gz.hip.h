// pemap_gz.hip.h -- the compacted pileup records (pile_emit_kernel, pemap_aux.hip.h) deflated on the device into the BGZF members of
// <out>.pileup.gz (pemap_dev_fetch_records_gz).  The rule -- pieces, parse, codes, member layout -- is pemap_gz_rule.h; its serial
// statement pmz_encode_piece is what these kernels reproduce byte for byte.  Over the n_rec records of a call, 16 bytes each:
//   1. pmz_ins_count_kernel / pmz_ins_emit_kernel   the records with an insertion count (c[5] > 0) compacted in order, the way
//                          pile_count_kernel / pile_emit_kernel compact the sites: counts per tile of PMZ_BLOCK records, their scan
//                          (ix_scan_tiles_kernel), 16-byte loads and stores
//   2. pmz_deflate_kernel  a workgroup per piece of PMZ_PIECE_RECORDS records, everything in LDS.  A thread owns PMZ_CHUNK = 32 bytes
//                          (two records): its 32 equality flags (byte i against byte i - 16) are one word; the run of set flags a byte
//                          lies in comes from that word and, where the run leaves it, from the neighbours' words (pmz_word_token), so
//                          the tokens need no walk.  The tokens' bits under the fixed code and every preset code are summed over
//                          the block, the smallest form is chosen (pmz_choose), a block scan places the winner's bits and LDS atomics
//                          put them into the member; the CRC-32 from per-thread slice CRCs and a log-step combine, as
//                          pcg_deflate_kernel does; the member leaves for slot b -- PMZ_SLOT bytes, the worst case, at a place known
//                          beforehand -- as aligned 16-byte stores
//   3. (ix_scan_tiles_kernel over the members' lengths: each member's place in the packed array and the packed length)
//   4. pmz_pack_kernel     a workgroup per member: from its slot to its place in the packed array, aligned 16-byte stores between
//                          byte stores at the two ragged ends
// An offset becomes an address only after a check against the record count, the piece count, the slot area's or the packed array's size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pemap_gz_rule.h"

#define PMZ_BLOCK 256
#define PMZ_CHUNK (PMZ_PIECE / PMZ_BLOCK)       // bytes a thread of the deflate kernel takes: 32, one flag word
#define PMZ_SLOT ((PMZ_MEMBER_MAX + 15u) & ~15u)        // bytes of a member's slot
#define PMZ_OUT16 (PMZ_SLOT / 16u + 1u) // 16-byte pieces of LDS for a member (one more: the word behind a token's last bit)
#define PMZ_SLOT_SLACK 64u      // bytes kept behind the last slot (pmz_pack_kernel reads one word beyond a member's 16-byte pieces)

static_assert (PMZ_CHUNK == 32u && PMZ_RECORD == 16u, "a thread's flags are one 32-bit word; a record is one 16-byte load");
static_assert (PMZ_HDR_BYTES <= PMZ_BLOCK && PMZ_CODES >= 1u && PMZ_CODES <= 4u, "a thread per header byte");

// ---- 1. the insertion sites
__device__ __forceinline__ bool pmz_has_ins (const uint4 & r)
{
  return (r.w >> 16) != 0u;     // c[5], bytes 14 and 15
}

__global__ void __launch_bounds__ (PMZ_BLOCK) pmz_ins_count_kernel (const uint4 * __restrict__ rec, unsigned long long n_rec, uint32_t * __restrict__ tile_count)
{
  __shared__ unsigned s_wave[PMZ_BLOCK / 64];
  const unsigned long long i = (unsigned long long) blockIdx.x * PMZ_BLOCK + threadIdx.x;
  const bool has = i < n_rec && pmz_has_ins (rec[i]);
  const unsigned long long bal = __ballot (has);
  if ((threadIdx.x & 63) == 0)
    s_wave[threadIdx.x >> 6] = (unsigned) __popcll (bal);
  __syncthreads ();
  if (threadIdx.x == 0)
    tile_count[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

__global__ void __launch_bounds__ (PMZ_BLOCK) pmz_ins_emit_kernel (const uint4 * __restrict__ rec, unsigned long long n_rec, const uint64_t * __restrict__ tile_offset,
                                                                   uint4 * __restrict__ out, unsigned long long cap)
{
  __shared__ unsigned s_wave[PMZ_BLOCK / 64];
  const unsigned long long i = (unsigned long long) blockIdx.x * PMZ_BLOCK + threadIdx.x;
  uint4 r = make_uint4 (0u, 0u, 0u, 0u);
  if (i < n_rec)
    r = rec[i];
  const bool has = i < n_rec && pmz_has_ins (r);
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long bal = __ballot (has);
  if (lane == 0)
    s_wave[wv] = (unsigned) __popcll (bal);
  __syncthreads ();
  unsigned before = (unsigned) __popcll (bal & ((1ull << lane) - 1ull));
  for (unsigned w = 0; w < wv; w++)
    before += s_wave[w];
  if (has)
    {
      const unsigned long long at = tile_offset[blockIdx.x] + before;
      if (at < cap)
        out[at] = r;
    }
}

// ---- 2. deflate
// byte j of the 32 a thread owns, from its eight words
#define PMZ_BYTE(w, j) (((w)[(j) >> 2] >> (8u * ((j) & 3u))) & 0xffu)

// rec: the call's records; slots: n_slots slots of PMZ_SLOT bytes.  A workgroup per piece.
__global__ void __launch_bounds__ (PMZ_BLOCK) pmz_deflate_kernel (const uint4 * __restrict__ rec, unsigned long long n_rec, unsigned char *__restrict__ slots,
                                                                  unsigned long long n_slots, uint32_t * __restrict__ member_len)
{
  __shared__ uint4 tile4[PMZ_PIECE_RECORDS];
  __shared__ uint4 out4[PMZ_OUT16];
  __shared__ unsigned code_tab[PMZ_CODES][286];  // a symbol's reversed code, its length from bit 16 on
  __shared__ unsigned crc_tab[256], flag_w[PMZ_BLOCK], w1[PMZ_BLOCK / 64], w2[PMZ_BLOCK];
  __shared__ unsigned part[PMZ_FORMS][PMZ_BLOCK / 64];
  const unsigned t = threadIdx.x;
  const unsigned long long b = blockIdx.x;
  const unsigned long long r0 = b * PMZ_PIECE_RECORDS;
  if (r0 >= n_rec || b >= n_slots)
    return;
  const unsigned nr = n_rec - r0 < PMZ_PIECE_RECORDS ? (unsigned) (n_rec - r0) : PMZ_PIECE_RECORDS;
  const unsigned n = PMZ_RECORD * nr;
  unsigned *out = (unsigned *) out4;
  uint8_t *outb = (uint8_t *) out4;
  const uint8_t *T = (const uint8_t *) tile4;
  // ---- the piece (zeros behind its end), the tables, a member of zeros
  for (unsigned k = t; k < PMZ_PIECE_RECORDS; k += PMZ_BLOCK)
    tile4[k] = k < nr ? rec[r0 + k] : make_uint4 (0u, 0u, 0u, 0u);
  crc_tab[t] = pcg_crc_table_entry (t);
  for (unsigned k = t; k < PMZ_CODES * 286u; k += PMZ_BLOCK)
    {
      const unsigned c = k / 286u, s = k - 286u * c;
      code_tab[c][s] = (unsigned) pmz_ll_code[c][s] | ((unsigned) pmz_ll_len[c][s] << 16);
    }
  for (unsigned k = t; k < PMZ_OUT16; k += PMZ_BLOCK)
    out4[k] = make_uint4 (0u, 0u, 0u, 0u);
  __syncthreads ();
  // ---- this thread's bytes [c0, c1), its two records and the one in front, its flags
  const unsigned c0 = t * PMZ_CHUNK < n ? t * PMZ_CHUNK : n, c1 = c0 + PMZ_CHUNK < n ? c0 + PMZ_CHUNK : n;
  unsigned w[8], m = 0u;
  {
    const uint4 a = tile4[2u * t], c = tile4[2u * t + 1u];
    const uint4 p = t ? tile4[2u * t - 1u] : make_uint4 (0u, 0u, 0u, 0u);
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = c.x, w[5] = c.y, w[6] = c.z, w[7] = c.w;
    const unsigned q[8] = { p.x, p.y, p.z, p.w, a.x, a.y, a.z, a.w };
#pragma unroll
    for (unsigned j = 0; j < PMZ_CHUNK; j++)
      if (PMZ_BYTE (w, j) == PMZ_BYTE (q, j) && c0 + j >= PMZ_DIST && c0 + j < c1)
        m |= 1u << j;
  }
  flag_w[t] = m;
  // ---- the slice CRCs: slices of PMZ_CHUNK bytes that end where the piece ends, so that only the first one is ragged
  unsigned crc;
  {
    const int e1 = (int) n - (int) (PMZ_CHUNK * (PMZ_BLOCK - 1u - t)), e0 = e1 - (int) PMZ_CHUNK;
    const unsigned q0 = e0 > 0 ? (unsigned) e0 : 0u, q1 = e1 > 0 ? (unsigned) e1 : 0u;
    crc = pcg_crc_slice (crc_tab, T + q0, q1 - q0);
  }
  __syncthreads ();
  // ---- how far the runs of set flags reach beyond the chunk's two ends (in real records at most 18 bytes: one neighbour's word)
  const unsigned left = (m & 1u) ? pmz_reach_left (flag_w, t) : 0u, right = (m >> 31) ? pmz_reach_right (flag_w, t, PMZ_BLOCK) : 0u;
  // ---- the tokens' bits under the fixed code and every preset code, summed over the block
  unsigned own[PMZ_FORMS];
#pragma unroll
  for (unsigned f = 0; f < PMZ_FORMS; f++)
    own[f] = 0u;
  for (unsigned j = 0; c0 + j < c1; j++)
    {
      const unsigned len = pmz_word_token (m, j, left, right);
      if (!len)
        continue;
      int nb;
      pmz_token_fixed (len, T[c0 + j], &nb);
      own[PMZ_FORM_FIXED] += (unsigned) nb;
      unsigned sym = T[c0 + j], extra = 0u, ev;
      if (len >= PCG_MIN_MATCH)
        {
          sym = pmz_len_sym (len, &extra, &ev);
          extra += 2u;          // the distance symbol's two extra bits
        }
#pragma unroll
      for (unsigned c = 0; c < PMZ_CODES; c++)
        own[2u + c] += (code_tab[c][sym] >> 16) + extra + (len >= PCG_MIN_MATCH ? (unsigned) pmz_d_len[c][PMZ_DIST_SYM] : 0u);
    }
#pragma unroll
  for (unsigned f = 1; f < PMZ_FORMS; f++)
    {
      unsigned s = own[f];
      for (int o = 32; o > 0; o >>= 1)
        s += __shfl_down (s, o, 64);
      if ((t & 63u) == 0u)
        part[f][t >> 6] = s;
    }
  __syncthreads ();
  unsigned bytes[PMZ_FORMS], hdr_bits = 3u;
  bytes[PMZ_FORM_STORED] = pmz_form_bytes (PMZ_FORM_STORED, n, 0u, 0u, 0u);
  bytes[PMZ_FORM_FIXED] = pmz_form_bytes (PMZ_FORM_FIXED, n, part[1][0] + part[1][1] + part[1][2] + part[1][3], 3u, 7u);
#pragma unroll
  for (unsigned c = 0; c < PMZ_CODES; c++)
    bytes[2u + c] = pmz_form_bytes (2u + c, n, part[2u + c][0] + part[2u + c][1] + part[2u + c][2] + part[2u + c][3], pmz_hdr_bits[c], code_tab[c][256] >> 16);
  const unsigned form = pmz_choose (bytes);
  unsigned body = bytes[0], mine = 0u;
#pragma unroll
  for (unsigned f = 1; f < PMZ_FORMS; f++)
    if (form == f)
      {
        body = bytes[f];
        mine = own[f];
        hdr_bits = f == PMZ_FORM_FIXED ? 3u : pmz_hdr_bits[f - 2u];
      }
  // ---- the winner's bits: a block scan of the threads' sums (a scan inside each wave, the waves' totals through LDS), then LDS atomics
  unsigned incl = mine;
  for (int o = 1; o < 64; o <<= 1)
    {
      const unsigned up = __shfl_up (incl, o, 64);
      if ((t & 63u) >= (unsigned) o)
        incl += up;
    }
  if ((t & 63u) == 63u)
    w1[t >> 6] = incl;
  __syncthreads ();
  for (unsigned k = 0; k < (t >> 6); k++)
    incl += w1[k];
  if (form == PMZ_FORM_STORED)
    {
      if (t < 5u)
        outb[PMZ_HEAD + t] = t == 0u ? 1u : t == 1u ? (uint8_t) n : t == 2u ? (uint8_t) (n >> 8) : t == 3u ? (uint8_t) ~n : (uint8_t) (~n >> 8);
      for (unsigned i = t; i < n; i += PMZ_BLOCK)
        outb[PMZ_HEAD + 5u + i] = T[i];
    }
  else
    {
      const unsigned c = form - 2u;     // (read only where form >= 2)
      if (form == PMZ_FORM_FIXED)
        {
          if (t == 0)
            atomicOr (&out[PMZ_HEAD / 4u], 3u << (8u * (PMZ_HEAD % 4u)));       // final block, fixed codes
        }
      else if (t < (hdr_bits + 7u) / 8u)
        atomicOr (&out[(PMZ_HEAD + t) / 4u], (unsigned) pmz_hdr[c][t] << (8u * ((PMZ_HEAD + t) % 4u)));
      unsigned at = 8u * PMZ_HEAD + hdr_bits + (incl - mine);
      const unsigned d_bits = form == PMZ_FORM_FIXED ? 0u : (unsigned) pmz_d_len[c][PMZ_DIST_SYM], d_code = form == PMZ_FORM_FIXED ? 0u : (unsigned) pmz_d_code[c][PMZ_DIST_SYM];
      // one more turn for the thread that holds the piece's last byte: the end-of-block code (the fixed code's is seven zeros)
      const bool last = c1 == n && c0 < n;
      for (unsigned j = 0; c0 + j < c1 + (last ? 1u : 0u); j++)
        {
          const bool eob = c0 + j == n;
          const unsigned len = eob ? 1u : pmz_word_token (m, j, left, right);
          if (!len)
            continue;
          const unsigned byte = eob ? 256u : T[c0 + j];
          int nb;
          unsigned v;
          if (form == PMZ_FORM_FIXED)
            v = eob ? pcg_sym (256u, &nb) : pmz_token_fixed (len, byte, &nb);
          else
            {
              unsigned sym = byte, eb = 0u, ev = 0u;
              if (len >= PCG_MIN_MATCH)
                sym = pmz_len_sym (len, &eb, &ev);
              const unsigned e = code_tab[c][sym];
              unsigned bits = e >> 16;
              v = e & 0xffffu;
              if (len >= PCG_MIN_MATCH)
                {
                  v |= ev << bits;
                  bits += eb;
                  v |= d_code << bits;
                  bits += d_bits;
                  v |= 3u << bits;
                  bits += 2u;
                }
              nb = (int) bits;
            }
          const unsigned long long vv = (unsigned long long) v << (at & 31u);
          if ((at >> 5) + 1u < PMZ_OUT16 * 4u)
            {
              atomicOr (&out[at >> 5], (unsigned) vv);
              if (vv >> 32)
                atomicOr (&out[(at >> 5) + 1u], (unsigned) (vv >> 32));
            }
          at += (unsigned) nb;
        }
    }
  // ---- the piece's CRC: at step o a slice group takes in the group of o slices to its right, all whole (or the left one is empty)
  w2[t] = crc;
  __syncthreads ();
  {
    // (a thread that sits out a step sits out every later one: only the threads that still combine square the power)
    unsigned xp = (t & 1u) ? 0u : pcg_xpow8 (PMZ_CHUNK);
    bool active = !(t & 1u);
    for (unsigned o = 1; o < PMZ_BLOCK; o <<= 1)
      {
        active = active && (t & (2u * o - 1u)) == 0u;
        if (active)
          {
            w2[t] = pcg_mulmod (xp, w2[t]) ^ w2[t + o];
            xp = pcg_mulmod (xp, xp);
          }
        __syncthreads ();
      }
  }
  // ---- the eighteen bytes in front, the eight behind; out
  const unsigned mlen = PMZ_HEAD + body + PMZ_TAIL;
  if (t < PMZ_HEAD)
    outb[t] = pmz_head_byte (t, mlen);
  if (t >= 64u && t < 64u + PMZ_TAIL)
    {
      const unsigned k = t - 64u;
      outb[PMZ_HEAD + body + k] = (uint8_t) ((k < 4u ? w2[0] : n) >> (8u * (k & 3u)));
    }
  __syncthreads ();
  uint4 *slot4 = (uint4 *) (slots + b * PMZ_SLOT);
  if (mlen <= PMZ_MEMBER_MAX)
    for (unsigned k = t; k < (mlen + 15u) / 16u; k += PMZ_BLOCK)
      slot4[k] = out4[k];
  if (t == 0)
    member_len[b] = mlen <= PMZ_MEMBER_MAX ? mlen : 0u;
}

// ---- 4. pack.  member_at: the scanned lengths; slot_bytes: n_slots * PMZ_SLOT + PMZ_SLOT_SLACK.  A workgroup per member.
__global__ void __launch_bounds__ (PMZ_BLOCK) pmz_pack_kernel (const unsigned char *__restrict__ slots, unsigned long long n_slots, unsigned long long slot_bytes,
                                                               const uint64_t * __restrict__ member_at, const uint32_t * __restrict__ member_len,
                                                               unsigned char *__restrict__ gz, unsigned long long gz_bytes)
{
  const unsigned t = threadIdx.x;
  const unsigned long long b = blockIdx.x;
  if (b >= n_slots)
    return;
  const unsigned long long g0 = member_at[b], slot_at = b * PMZ_SLOT;
  const unsigned m = member_len[b];
  if (m == 0u || m > PMZ_MEMBER_MAX || g0 + m > gz_bytes || slot_at + ((m + 15ull) & ~15ull) + 16ull > slot_bytes)
    return;
  const unsigned char *src = slots + slot_at;
  unsigned char *dst = gz + g0;
  // dst + head is the first 16-byte boundary; whole 16-byte pieces behind it
  const unsigned head = (unsigned) ((16ull - (g0 & 15ull)) & 15ull) < m ? (unsigned) ((16ull - (g0 & 15ull)) & 15ull) : m;
  const unsigned whole = (m - head) / 16u;
  if (t < head)
    dst[t] = src[t];
  const unsigned sh = 8u * (head & 3u);
  const unsigned *sw = (const unsigned *) src + head / 4u;
  for (unsigned k = t; k < whole; k += PMZ_BLOCK)
    {
      unsigned w[5];
#pragma unroll
      for (int x = 0; x < 5; x++)
        w[x] = sw[4u * k + x];          // (the fifth word lies inside the slot area: checked above)
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
