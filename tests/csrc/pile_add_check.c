/* pile_add_check.c -- pm_add_u16x2 (pecaller_amd/csrc/pemap_pile_add.h), the per-word arithmetic of pm_pile_add_kernel, against two
   separate uint16_t additions: every pair of the edge values in each half independently (49 x 49 word pairs), then 1 M words of a
   fixed-seed generator.  Exit status 0 only when all agree.  Built by tests/test_pile_add_cpu.py with -fsanitize=address,undefined. */
#include <stdio.h>
#include <stdint.h>
#include "../../pecaller_amd/csrc/pemap_pile_add.h"

static uint32_t
two_adds (uint32_t a, uint32_t b)
{
  const uint16_t lo = (uint16_t) ((uint16_t) (a & 0xFFFFu) + (uint16_t) (b & 0xFFFFu));
  const uint16_t hi = (uint16_t) ((uint16_t) (a >> 16) + (uint16_t) (b >> 16));
  return (uint32_t) lo | ((uint32_t) hi << 16);
}

static int
check (uint32_t a, uint32_t b)
{
  const uint32_t got = pm_add_u16x2 (a, b), want = two_adds (a, b);
  if (got != want)
    {
      printf ("pm_add_u16x2 (%08x, %08x) = %08x, two u16 additions give %08x\n", a, b, got, want);
      return 1;
    }
  return 0;
}

int
main (void)
{
  static const uint32_t edge[7] = { 0, 1, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF, 40000 };
  long bad = 0, n = 0;
  for (int al = 0; al < 7; al++)
    for (int bl = 0; bl < 7; bl++)
      for (int ah = 0; ah < 7; ah++)
        for (int bh = 0; bh < 7; bh++, n++)
          bad += check (edge[al] | (edge[ah] << 16), edge[bl] | (edge[bh] << 16));
  uint64_t x = 0x9E3779B97F4A7C15ull;   /* xorshift64, fixed seed */
  for (int i = 0; i < 1000000; i++, n++)
    {
      x ^= x << 13;
      x ^= x >> 7;
      x ^= x << 17;
      bad += check ((uint32_t) x, (uint32_t) (x >> 32));
    }
  printf ("%ld word pairs, %ld disagree\n", n, bad);
  return bad ? 1 : 0;
}
