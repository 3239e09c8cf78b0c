/* row_len_check.c -- the row arithmetic of pecall_row_len.h against sprintf, stand-alone (its own main): digit counts and digit bytes
   of positions, and the length of a template row of <outfile>.base.gz as emit_rows of pecaller_main.c builds it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../pecaller_amd/csrc/pecall_row_len.h"

static long checked = 0, bad = 0;

static void
check_pos (uint32_t pos)
{
  char want[32], got[32];
  const int n = sprintf (want, "%d", (int) pos);
  const int d = pcr_pos_digits (pos);
  memset (got, '#', sizeof got);
  pcr_put_digits (got + 1, pos, d);
  checked++;
  if (d != n || memcmp (got + 1, want, (size_t) n) != 0 || got[0] != '#' || got[1 + d] != '#')
    {
      bad++;
      printf ("position %u: %d digits, sprintf has %d (%s)\n", pos, d, n, want);
    }
}

/* a row the way emit_rows writes it, every posterior 1 */
static size_t
sprintf_row (char *w, const char *name, uint32_t pos, int indiv)
{
  char *w0 = w;
  w += sprintf (w, "\n%s\t%d\t%c", name, (int) pos, 'A');
  for (int i = 0; i < indiv; i++)
    w += sprintf (w, "\t%c\t%s", "ACGTDIMRWSYKEHN"[i % 15], "1");
  return (size_t) (w - w0);
}

int
main (void)
{
  static const int indivs[] = { 1, 3, 64, 65, 512 };
  static const char *names[] = { "c", "chr12_KI270904v1_altern" };      /* 1 and 23 bytes */
  /* every digit boundary: 0, 9, 10, 99, 100, ..., 999999999, 1000000000, and the last position */
  check_pos (0);
  for (uint64_t p = 10; p <= 1000000000ull; p *= 10)
    {
      check_pos ((uint32_t) (p - 1));
      check_pos ((uint32_t) p);
      check_pos ((uint32_t) (p + 1));
    }
  check_pos (PCR_MAX_POS - 1);
  check_pos (PCR_MAX_POS);
  uint64_t x = 88172645463325252ull;
  for (int k = 0; k < 6000; k++)
    {
      x ^= x << 13;
      x ^= x >> 7;
      x ^= x << 17;
      check_pos ((uint32_t) (x >> (33 + k % 31)) & PCR_MAX_POS);        /* (all magnitudes) */
    }
  long rows = 0;
  char *buf = (char *) malloc (64 + 32 + 4 * 512 + 16);
  if (!buf)
    return 2;
  for (size_t a = 0; a < sizeof indivs / sizeof indivs[0]; a++)
    for (size_t b = 0; b < 2; b++)
      for (uint64_t p = 1; p <= 10000000000ull; p *= 10)
        {
          const uint32_t pos = (uint32_t) (p > PCR_MAX_POS ? PCR_MAX_POS : p - 1);
          const size_t want = sprintf_row (buf, names[b], pos, indivs[a]);
          rows++;
          if (strlen (buf) != want || pcr_row_len ((uint32_t) strlen (names[b]), pos, (uint32_t) indivs[a]) != (uint64_t) want
              || pcr_head_len ((uint32_t) strlen (names[b]), pos) + 4u * (uint32_t) indivs[a] != want)
            {
              bad++;
              printf ("row of %d samples, name %s, position %u: %llu bytes, sprintf has %zu\n", indivs[a], names[b], pos,
                      (unsigned long long) pcr_row_len ((uint32_t) strlen (names[b]), pos, (uint32_t) indivs[a]), want);
            }
        }
  free (buf);
  /* 2^22 columns of 512 samples: the sum needs 64 bits */
  const uint64_t big = pcr_row_len (23, PCR_MAX_POS, 512) * (uint64_t) (1u << 22);
  if (big != (uint64_t) 2085 * 4194304ull || big <= 0xffffffffull)
    {
      bad++;
      printf ("2^22 rows of 512 samples: %llu bytes\n", (unsigned long long) big);
    }
  printf ("%ld positions, %ld rows, %ld disagree\n", checked, rows, bad);
  return bad ? 1 : 0;
}
