/*
 * pecall_row_len.h -- the arithmetic of a template row of <outfile>.base.gz.  A column whose samples all have posterior exactly 1
 * prints as "\n<contig>\t<pos>\t<ref>" followed by "\t<call>\t1" per sample (emit_rows of pecaller_main.c; in the reference the
 * gzprintf loop of pecaller.c:1760-1775): its length is known from the contig name's length, the position's digits and the number
 * of samples.  Plain C, no HIP types: the kernels of pecall_rows.hip.h call these on the device, pecaller_main.c and
 * tests/csrc/row_len_check.c on the host.  Positions are what "%d" prints of a non-negative int: 0 .. 2^31 - 1.
 */
#ifndef PECALL_ROW_LEN_H
#define PECALL_ROW_LEN_H
#include <stdint.h>

#ifdef __HIPCC__
#define PCR_FN __host__ __device__
#else
#define PCR_FN
#endif

#define PCR_MAX_POS 2147483647u /* (int) pos is printed: nothing beyond this is a position */
#define PCR_MAX_DIGITS 10

/* decimal digits of pos: 1 for 0 .. 9, 10 from 1000000000 on */
static inline PCR_FN int
pcr_pos_digits (uint32_t pos)
{
  int n = 1;
  if (pos >= 100000000u)
    {
      n += 8;
      pos /= 100000000u;
    }
  if (pos >= 10000u)
    {
      n += 4;
      pos /= 10000u;
    }
  if (pos >= 100u)
    {
      n += 2;
      pos /= 100u;
    }
  if (pos >= 10u)
    n += 1;
  return n;
}

/* the n = pcr_pos_digits (pos) digits of pos at dst[0 .. n), most significant first; no terminator */
static inline PCR_FN void
pcr_put_digits (char *dst, uint32_t pos, int n)
{
  for (int k = n - 1; k >= 0; k--)
    {
      dst[k] = (char) ('0' + pos % 10u);
      pos /= 10u;
    }
}

/* bytes of a row's head: '\n', the contig name, '\t', the position, '\t', the reference letter */
static inline PCR_FN uint32_t
pcr_head_len (uint32_t name_len, uint32_t pos)
{
  return 1u + name_len + 1u + (uint32_t) pcr_pos_digits (pos) + 1u + 1u;
}

/* bytes of a template row: the head, then '\t' call '\t' '1' per sample */
static inline PCR_FN uint64_t
pcr_row_len (uint32_t name_len, uint32_t pos, uint32_t indiv)
{
  return (uint64_t) pcr_head_len (name_len, pos) + 4u * (uint64_t) indiv;
}

#endif
