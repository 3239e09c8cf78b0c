/*
 * pemap_pile_diff.h -- the difference form of one pileup counter plane.  A plane (PmPile, pemap_kernels.hip.h) holds the reference's
 * unsigned short counters c[p] (pemapper.c:53-58), two positions to a 32-bit word: position p is half (p & 1) of word p >> 1.  In
 * difference form the same words hold D[p] = c[p] - c[p-1] modulo 2^16, with c[-1] = 0, and the counts come back as the running sum
 * modulo 2^16.  Everything is linear modulo 2^16, so "add 1 to c[a..b]" is D[a] += 1, D[b+1] -= 1 whatever the counters hold, wraps
 * included.  No bias: a plane of zeros is a plane of zeros in both forms.  Plain C, no HIP types: the pile and conversion kernels
 * (pemap_sw.hip.h, pemap_aux.hip.h) call it on the device, tests/csrc/pile_diff_check.c on the host.
 */
#ifndef PEMAP_PILE_DIFF_H
#define PEMAP_PILE_DIFF_H
#include <stdint.h>

#ifdef __HIPCC__
#define PM_PILE_DIFF_FN __host__ __device__
#else
#define PM_PILE_DIFF_FN
#endif

/* What a 32-bit add must add to a word to change one half by sign = +1 or -1: the high half (odd positions) wraps by itself; the low
   half's carry (+1 onto 0xFFFF) or borrow (-1 from 0) lands in its neighbour and is taken back, pm_diff_takeback. */
static inline PM_PILE_DIFF_FN uint32_t
pm_diff_addend (int odd, int sign)
{
  return sign > 0 ? (odd ? 0x00010000u : 0x00000001u) : (odd ? 0xFFFF0000u : 0xFFFFFFFFu);
}

/* `old` is the word before the add of `addend` (what an atomic add returns).  The result is the second addend that undoes what the
   low half carried or borrowed into the high one, 0 when it did neither (always for the high half's addends). */
static inline PM_PILE_DIFF_FN uint32_t
pm_diff_takeback (uint32_t old, uint32_t addend)
{
  if (addend == 0x00000001u && (old & 0xFFFFu) == 0xFFFFu)
    return 0xFFFF0000u;         /* -0x10000 */
  if (addend == 0xFFFFFFFFu && (old & 0xFFFFu) == 0u)
    return 0x00010000u;
  return 0u;
}

/* unfold, one word: the count word and the count of the position before it (the previous word's high half) -> the difference word */
static inline PM_PILE_DIFF_FN uint32_t
pm_diff_unfold_word (uint32_t counts, uint32_t prev_high)
{
  const uint32_t lo = counts & 0xFFFFu, hi = counts >> 16;
  return ((lo - prev_high) & 0xFFFFu) | ((hi - lo) << 16);
}

/* the sum of a difference word's two halves, and of two such sums (tiles): what a word, or a tile, adds to the running sum */
static inline PM_PILE_DIFF_FN uint32_t
pm_diff_word_sum (uint32_t diffs)
{
  return ((diffs & 0xFFFFu) + (diffs >> 16)) & 0xFFFFu;
}

static inline PM_PILE_DIFF_FN uint32_t
pm_diff_combine (uint32_t sum_a, uint32_t sum_b)
{
  return (sum_a + sum_b) & 0xFFFFu;
}

/* fold, one word: the difference word and the running sum carried in (the count of the position before it) -> the count word; the
   sum carried out is its high half, pm_diff_combine (carry_in, pm_diff_word_sum (diffs)) */
static inline PM_PILE_DIFF_FN uint32_t
pm_diff_fold_word (uint32_t diffs, uint32_t carry_in)
{
  const uint32_t lo = (carry_in + (diffs & 0xFFFFu)) & 0xFFFFu;
  return lo | ((lo + (diffs >> 16)) << 16);
}

#endif
