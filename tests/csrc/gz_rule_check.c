/*
 * gz_rule_check.c -- the serial statement of pecall_gz_rule.h as a program of its own (its own main; nothing of it is loaded into
 * Python):
 *   gz_rule_check encode <text> <out> [<cuts>]   the members pcg_encode_piece makes of the file <text>, written to <out>; <cuts>: a
 *                                                file of ascending byte offsets, one per line, each standing for a hole (the text is
 *                                                cut into runs there; equal offsets give empty runs, which make no member).
 *                                                Prints "pieces P bytes B".
 *   gz_rule_check crc <text> <slices>            the CRC-32 of the file from <slices> slices of equal length (the last one shorter
 *                                                or empty) put together with pcg_crc_combine, and from one slice; prints both in hex
 *   gz_rule_check piece                          prints PCG_PIECE
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../pecaller_amd/csrc/pecall_gz_rule.h"

static uint8_t *
slurp (const char *path, size_t *n)
{
  FILE *f = fopen (path, "rb");
  if (!f)
    {
      fprintf (stderr, "gz_rule_check: cannot open %s\n", path);
      exit (2);
    }
  fseek (f, 0, SEEK_END);
  const long len = ftell (f);
  fseek (f, 0, SEEK_SET);
  uint8_t *p = malloc ((size_t) len + 1);
  if (!p || fread (p, 1, (size_t) len, f) != (size_t) len)
    {
      fprintf (stderr, "gz_rule_check: cannot read %s\n", path);
      exit (2);
    }
  fclose (f);
  *n = (size_t) len;
  return p;
}

static int
encode (const char *text_path, const char *out_path, const char *cuts_path)
{
  size_t n, n_cuts = 0, cap = 0;
  uint8_t *t = slurp (text_path, &n);
  size_t *cut = NULL;
  if (cuts_path)
    {
      FILE *f = fopen (cuts_path, "r");
      unsigned long long v;
      if (!f)
        {
          fprintf (stderr, "gz_rule_check: cannot open %s\n", cuts_path);
          return 2;
        }
      while (fscanf (f, "%llu", &v) == 1)
        {
          if (n_cuts == cap)
            {
              cap = cap ? 2 * cap : 64;
              cut = realloc (cut, cap * sizeof *cut);
              if (!cut)
                return 2;
            }
          if (v > n || (n_cuts && v < cut[n_cuts - 1]))
            {
              fprintf (stderr, "gz_rule_check: cut %llu is beyond the text or descends\n", v);
              return 2;
            }
          cut[n_cuts++] = (size_t) v;
        }
      fclose (f);
    }
  FILE *o = fopen (out_path, "wb");
  if (!o)
    {
      fprintf (stderr, "gz_rule_check: cannot write %s\n", out_path);
      return 2;
    }
  uint8_t *member = malloc (PCG_MEMBER_MAX);
  unsigned long long pieces = 0, bytes = 0;
  for (size_t r = 0; r <= n_cuts; r++)
    {
      const size_t r0 = r ? cut[r - 1] : 0, r1 = r < n_cuts ? cut[r] : n;
      const uint64_t np = pcg_run_pieces (r1 - r0);
      for (uint64_t k = 0; k < np; k++)
        {
          const size_t a = r0 + k * PCG_PIECE, len = r1 - a < PCG_PIECE ? r1 - a : PCG_PIECE;
          const uint32_t m = pcg_encode_piece (t + a, (uint32_t) len, member);
          if (m > PCG_HEAD + 5u + len + PCG_TAIL || fwrite (member, 1, m, o) != m)
            {
              fprintf (stderr, "gz_rule_check: a member of %u bytes for a piece of %zu, or a failed write\n", m, len);
              return 1;
            }
          pieces++;
          bytes += m;
        }
    }
  if (fclose (o))
    return 2;
  printf ("pieces %llu bytes %llu\n", pieces, bytes);
  free (member);
  free (cut);
  free (t);
  return 0;
}

static int
crc (const char *text_path, long slices)
{
  size_t n;
  uint8_t *t = slurp (text_path, &n);
  uint32_t table[256];
  for (uint32_t k = 0; k < 256u; k++)
    table[k] = pcg_crc_table_entry (k);
  if (slices < 1)
    return 2;
  const size_t each = (n + (size_t) slices - 1) / (size_t) slices;
  uint32_t c = 0;
  for (long s = 0; s < slices; s++)
    {
      const size_t a = (size_t) s * each < n ? (size_t) s * each : n, len = n - a < each ? n - a : each;
      const uint32_t cs = pcg_crc_slice (table, t + a, (uint32_t) len);
      c = s ? pcg_crc_combine (c, cs, len) : cs;
    }
  printf ("%08x %08x\n", c, pcg_crc_slice (table, t, (uint32_t) n));
  free (t);
  return 0;
}

int
main (int argc, char **argv)
{
  if (argc >= 4 && !strcmp (argv[1], "encode"))
    return encode (argv[2], argv[3], argc > 4 ? argv[4] : NULL);
  if (argc == 4 && !strcmp (argv[1], "crc"))
    return crc (argv[2], atol (argv[3]));
  if (argc == 2 && !strcmp (argv[1], "piece"))
    {
      printf ("%u\n", PCG_PIECE);
      return 0;
    }
  fprintf (stderr, "usage: gz_rule_check encode <text> <out> [<cuts>] | crc <text> <slices> | piece\n");
  return 2;
}
