/*
 * pemap_pile_add.h -- the sum of two pileup words.  A word of the counter planes (PmPile, pemap_kernels.hip.h) holds two of the
 * reference's unsigned short counters (pemapper.c:53-58): the sum of two objects' words is the two 16-bit sums, each modulo 2^16,
 * with no carry from the low counter into the high one.  Plain C, no HIP types: pm_pile_add_kernel (pemap_aux.hip.h) calls it on
 * the device, tests/csrc/pile_add_check.c on the host.
 */
#ifndef PEMAP_PILE_ADD_H
#define PEMAP_PILE_ADD_H
#include <stdint.h>

#ifdef __HIPCC__
#define PM_PILE_ADD_FN __host__ __device__
#else
#define PM_PILE_ADD_FN
#endif

/* Bits 0..14 of each half are added in place (0x7FFF + 0x7FFF = 0xFFFE: the carry of a half stops in its own bit 15); bit 15 of
   each half is then a ^ b ^ that carry, and its own carry is dropped. */
static inline PM_PILE_ADD_FN uint32_t
pm_add_u16x2 (uint32_t a, uint32_t b)
{
  const uint32_t low15 = (a & 0x7FFF7FFFu) + (b & 0x7FFF7FFFu);
  return low15 ^ ((a ^ b) & 0x80008000u);
}

#endif
