/*
 * pecall_gz_rule.h -- how the device-made text of <outfile>.base.gz becomes gzip members (pecall_dev_sites_base_gz), stated once.
 * Plain C, no HIP types: the kernels of pecall_gz.hip.h call these on the device, pecaller_main.c and tests/csrc/gz_rule_check.c
 * on the host.  pcg_encode_piece is the serial statement the kernels are held to, byte for byte.
 *
 * Pieces.  A run of text is the bytes between two holes, or between a text end and a hole.  A run of n bytes is cut into
 * ceil (n / PCG_PIECE) pieces: piece k is the run's bytes [k * PCG_PIECE, min (n, (k + 1) * PCG_PIECE)).  An empty run has no
 * piece.  A piece becomes one complete gzip member (RFC 1952): the 10 bytes 1f 8b 08 00 00 00 00 00 00 03 (deflate, no flags,
 * mtime 0, no extra flags, OS 3), one final deflate block, the CRC-32 of the piece and its length, both little-endian.
 *
 * Parse.  With t[0 .. n) the piece, a position i has up to two candidate distances:
 *   A  4, if i >= 4;
 *   B  D (i) = s - p, where s is the largest index <= i with t[s] == '\n' and p the largest index < s with t[p] == '\n' (the byte at
 *      the same offset in the previous row); none if the piece has no such s or p.  Bytes in front of the piece do not exist:
 *      a piece that begins inside a row has no candidate B before its second '\n'.
 * The match of candidate A at i is the longest m <= min (258, n - i) with t[i + k] == t[i + k - 4] for all k < m.  The match of
 * candidate B is the longest m <= min (258, n - i) with t[i + k] == t[i + k - D (i)] and, for 0 < k, D (i + k) == D (i): it ends in
 * front of a row start at which the row distance changes.  (So both are run lengths of per-byte flags, which is how the kernel
 * finds them.)  The longer match wins; equal lengths go to the smaller distance; a winner of fewer than 3 bytes is dropped and the
 * byte goes as a literal.  Greedy: after a match of m the parse goes on at i + m, after a literal at i + 1; nothing is deferred.
 * There is no third candidate.
 *
 * Encoding.  Fixed Huffman codes (RFC 1951, 3.2.6): the block's three header bits 1, 1, 0, the tokens, the end-of-block code.
 * If that block would take no fewer bytes than the stored form (5 + n), the piece goes as one stored block (01, n, ~n, the bytes):
 * PCG_PIECE is below 65,536, so one is enough, and no member is longer than PCG_HEAD + 5 + n + PCG_TAIL.
 *
 * CRC-32.  Of a piece from the CRCs of its slices: pcg_crc_slice over a 256-entry table (pcg_crc_table_entry), and
 * pcg_crc_combine (crc (A), crc (B), len (B)) = crc (A || B): crc (A) times x^(8 len (B)) modulo the polynomial, plus crc (B); the
 * product is a carry-less multiply in software (pcg_mulmod), the power comes from squarings (pcg_xpow8).
 */
#ifndef PECALL_GZ_RULE_H
#define PECALL_GZ_RULE_H
#include <stdint.h>

#ifdef __HIPCC__
#define PCG_FN __host__ __device__
#else
#define PCG_FN
#endif

#define PCG_PIECE 7168u         /* bytes of a piece at most: with its three 16-bit side arrays and the member, under 64 KB of LDS */
#define PCG_MIN_MATCH 3u
#define PCG_MAX_MATCH 258u
#define PCG_HEAD 10u            /* bytes of a member in front of its deflate block */
#define PCG_TAIL 8u             /* and behind it: CRC-32, ISIZE */
#define PCG_MEMBER_MAX (PCG_HEAD + 5u + PCG_PIECE + PCG_TAIL)
#define PCG_CRC_POLY 0xedb88320u

/* the pieces of a run of n bytes */
static inline PCG_FN uint64_t
pcg_run_pieces (uint64_t n)
{
  return (n + PCG_PIECE - 1u) / PCG_PIECE;
}

/* the member's first ten bytes */
static inline PCG_FN uint8_t
pcg_head_byte (uint32_t k)
{
  return k == 0u ? 0x1fu : k == 1u ? 0x8bu : k == 2u ? 0x08u : k == 9u ? 0x03u : 0u;
}

/* the low n bits of x in reverse order (Huffman codes go into the stream most significant bit first) */
static inline PCG_FN uint32_t
pcg_rev (uint32_t x, int n)
{
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
  x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
  x = (x >> 16) | (x << 16);
  return x >> (32 - n);
}

/* floor (log2 (x)), x > 0 */
static inline PCG_FN int
pcg_log2 (uint32_t x)
{
  return 31 - __builtin_clz (x);
}

/* a literal or length symbol 0 .. 287 as its fixed code, reversed: *bits = 7, 8 or 9 */
static inline PCG_FN uint32_t
pcg_sym (uint32_t sym, int *bits)
{
  if (sym < 144u)
    {
      *bits = 8;
      return pcg_rev (0x30u + sym, 8);
    }
  if (sym < 256u)
    {
      *bits = 9;
      return pcg_rev (0x190u + (sym - 144u), 9);
    }
  if (sym < 280u)
    {
      *bits = 7;
      return pcg_rev (sym - 256u, 7);
    }
  *bits = 8;
  return pcg_rev (0xc0u + (sym - 280u), 8);
}

/* A token as its bits in stream order, bit 0 first: len 1 = the literal `byte`, else a match of len 3 .. 258 at dist 1 .. 32768.
   At most 8 + 5 + 5 + 13 = 31 bits. */
static inline PCG_FN uint32_t
pcg_token (uint32_t len, uint32_t dist, uint32_t byte, int *bits)
{
  if (len < PCG_MIN_MATCH)
    return pcg_sym (byte, bits);
  /* length: codes 257 .. 264 one length each, then four codes per extra bit, 285 for 258 alone */
  const uint32_t l = len - 3u;
  uint32_t code, eb = 0u, ev = 0u;
  if (len == PCG_MAX_MATCH)
    code = 285u;
  else if (l < 8u)
    code = 257u + l;
  else
    {
      eb = (uint32_t) pcg_log2 (l) - 2u;
      code = 257u + 4u * eb + (l >> eb);
      ev = l & ((1u << eb) - 1u);
    }
  int n;
  uint32_t v = pcg_sym (code, &n);
  v |= ev << n;
  n += (int) eb;
  /* distance: codes 0 .. 3 one distance each, then two codes per extra bit; five bits each */
  const uint32_t dd = dist - 1u;
  uint32_t dcode = dd, deb = 0u, dev = 0u;
  if (dd >= 4u)
    {
      deb = (uint32_t) pcg_log2 (dd) - 1u;
      dcode = 2u * (deb + 1u) + ((dd >> deb) & 1u);
      dev = dd & ((1u << deb) - 1u);
    }
  v |= pcg_rev (dcode, 5) << n;
  n += 5;
  v |= dev << n;
  n += (int) deb;
  *bits = n;
  return v;
}

/* of the two candidates' match lengths (each already at most min (258, what is left of the piece)), with d_row = 0 where there is
   no candidate B: the token's length (1: a literal) and distance */
static inline PCG_FN uint32_t
pcg_choose (uint32_t len4, uint32_t len_row, uint32_t d_row, uint32_t *dist)
{
  uint32_t best = len4, d = 4u;
  if (d_row != 0u && (len_row > best || (len_row == best && d_row < 4u)))
    {
      best = len_row;
      d = d_row;
    }
  if (best < PCG_MIN_MATCH)
    {
      *dist = 0u;
      return 1u;
    }
  *dist = d;
  return best;
}

/* bytes of the fixed-Huffman block of token bits that sum to `bits`: three header bits, the seven of the end-of-block code */
static inline PCG_FN uint32_t
pcg_fixed_bytes (uint64_t bits)
{
  return (uint32_t) ((3u + bits + 7u + 7u) >> 3);
}

/* ---- CRC-32 (reflected, polynomial PCG_CRC_POLY) */

static inline PCG_FN uint32_t
pcg_crc_table_entry (uint32_t i)
{
  uint32_t c = i;
  for (int k = 0; k < 8; k++)
    c = (c & 1u) ? (c >> 1) ^ PCG_CRC_POLY : c >> 1;
  return c;
}

/* the CRC-32 of n bytes (what zlib's crc32 (0, p, n) gives); table[i] = pcg_crc_table_entry (i) */
static inline PCG_FN uint32_t
pcg_crc_slice (const uint32_t * table, const uint8_t * p, uint32_t n)
{
  uint32_t c = 0xffffffffu;
  for (uint32_t k = 0; k < n; k++)
    c = table[(c ^ p[k]) & 0xffu] ^ (c >> 8);
  return c ^ 0xffffffffu;
}

/* a times b modulo the polynomial; bit 31 is the coefficient of x^0 */
static inline PCG_FN uint32_t
pcg_mulmod (uint32_t a, uint32_t b)
{
  uint32_t p = 0u;
  for (int k = 31; k >= 0; k--)
    {
      if ((a >> k) & 1u)
        p ^= b;
      b = (b & 1u) ? (b >> 1) ^ PCG_CRC_POLY : b >> 1;
    }
  return p;
}

/* x^(8 n) modulo the polynomial */
static inline PCG_FN uint32_t
pcg_xpow8 (uint64_t n)
{
  uint32_t r = 0x80000000u, b = 0x00800000u;    /* x^0, x^8 */
  for (; n; n >>= 1)
    {
      if (n & 1u)
        r = pcg_mulmod (r, b);
      b = pcg_mulmod (b, b);
    }
  return r;
}

/* crc (A || B) from crc (A), crc (B) and the length of B; a B of no bytes has CRC 0 */
static inline PCG_FN uint32_t
pcg_crc_combine (uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
  return pcg_mulmod (pcg_xpow8 (len_b), crc_a) ^ crc_b;
}

/* ---- the serial statement (host) */
#ifndef __HIP_DEVICE_COMPILE__

/* D (i) of the piece at d[0 .. n): 0 where there is no candidate B */
static inline void
pcg_row_dist (const uint8_t * t, uint32_t n, uint16_t * d)
{
  int64_t s = -1, p = -1;
  for (uint32_t i = 0; i < n; i++)
    {
      if (t[i] == '\n')
        {
          p = s;
          s = i;
        }
      d[i] = (uint16_t) (p >= 0 ? s - p : 0);
    }
}

/* the tokens of piece t[0 .. n), n <= PCG_PIECE, at tok_pos / tok_len / tok_dist [n at most]; a literal has length 1 and distance 0 */
static inline uint32_t
pcg_parse (const uint8_t * t, uint32_t n, uint16_t * tok_pos, uint16_t * tok_len, uint16_t * tok_dist)
{
  uint16_t d[PCG_PIECE];
  uint32_t k = 0;
  pcg_row_dist (t, n, d);
  for (uint32_t i = 0; i < n;)
    {
      const uint32_t room = n - i < PCG_MAX_MATCH ? n - i : PCG_MAX_MATCH;
      uint32_t l4 = 0, lr = 0, dist;
      if (i >= 4u)
        while (l4 < room && t[i + l4] == t[i + l4 - 4u])
          l4++;
      if (d[i])
        while (lr < room && t[i + lr] == t[i + lr - d[i]] && (lr == 0u || d[i + lr] == d[i + lr - 1u]))
          lr++;
      const uint32_t len = pcg_choose (l4, lr, d[i], &dist);
      tok_pos[k] = (uint16_t) i;
      tok_len[k] = (uint16_t) len;
      tok_dist[k] = (uint16_t) dist;
      k++;
      i += len;
    }
  return k;
}

/* piece t[0 .. n), 0 < n <= PCG_PIECE, as a gzip member at out[0 .. PCG_MEMBER_MAX) -> the member's length */
static inline uint32_t
pcg_encode_piece (const uint8_t * t, uint32_t n, uint8_t * out)
{
  uint16_t tp[PCG_PIECE], tl[PCG_PIECE], td[PCG_PIECE];
  uint32_t table[256];
  const uint32_t nt = pcg_parse (t, n, tp, tl, td);
  uint64_t bits = 0;
  int b;
  for (uint32_t k = 0; k < nt; k++)
    {
      pcg_token (tl[k], td[k], t[tp[k]], &b);
      bits += (uint64_t) b;
    }
  for (uint32_t k = 0; k < PCG_HEAD; k++)
    out[k] = pcg_head_byte (k);
  uint32_t at = PCG_HEAD;
  const uint32_t fixed = pcg_fixed_bytes (bits);
  if (fixed >= 5u + n)
    {
      out[at++] = 1u;
      out[at++] = (uint8_t) n;
      out[at++] = (uint8_t) (n >> 8);
      out[at++] = (uint8_t) ~n;
      out[at++] = (uint8_t) (~n >> 8);
      for (uint32_t k = 0; k < n; k++)
        out[at++] = t[k];
    }
  else
    {
      uint64_t acc = 3u;        /* final block, fixed codes */
      int have = 3;
      for (uint32_t k = 0; k <= nt; k++)
        {
          const uint32_t v = k < nt ? pcg_token (tl[k], td[k], t[tp[k]], &b) : pcg_sym (256u, &b);
          acc |= (uint64_t) v << have;
          have += b;
          for (; have >= 8; have -= 8, acc >>= 8)
            out[at++] = (uint8_t) acc;
        }
      if (have)
        out[at++] = (uint8_t) acc;
    }
  for (uint32_t k = 0; k < 256u; k++)
    table[k] = pcg_crc_table_entry (k);
  const uint32_t crc = pcg_crc_slice (table, t, n);
  for (int k = 0; k < 4; k++)
    out[at++] = (uint8_t) (crc >> (8 * k));
  for (int k = 0; k < 4; k++)
    out[at++] = (uint8_t) (n >> (8 * k));
  return at;
}

#endif
#endif
