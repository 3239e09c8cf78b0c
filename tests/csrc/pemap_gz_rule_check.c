/*
 * pemap_gz_rule_check.c -- the serial statement of pemap_gz_rule.h as a program of its own (its own main; nothing of it is loaded
 * into Python):
 *   pemap_gz_rule_check encode <bytes> <out>   the members pmz_encode_bytes makes of the file <bytes> (records, or any bytes), cut
 *                                              into pieces of PMZ_PIECE bytes, written to <out>.  For every piece the tokens of the
 *                                              run-length closed form (pmz_parse) are compared with a greedy parse that goes byte by
 *                                              byte, and with the tokens taken from the flags held as 32-bit words, as the kernel
 *                                              holds them (exit status 1 where they differ).  Prints "pieces P bytes B forms S F P0 P1 ..",
 *                                              the pieces that went out stored, with the fixed code and with each preset code.
 *   pemap_gz_rule_check tables                 every preset table: lengths within 1 .. 15 (distance: 0 .. 15), both codes complete,
 *                                              the committed codes the canonical ones of the lengths, the header bits within the
 *                                              committed bytes, a token within 31 bits; prints "tables N ok"
 *   pemap_gz_rule_check eof <out>              the 28-byte empty member
 *   pemap_gz_rule_check consts                 prints PMZ_PIECE_RECORDS PMZ_CODES PMZ_MEMBER_MAX
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../pecaller_amd/csrc/pemap_gz_rule.h"

static uint8_t *
slurp (const char *path, size_t *n)
{
  FILE *f = fopen (path, "rb");
  if (!f)
    {
      fprintf (stderr, "pemap_gz_rule_check: cannot open %s\n", path);
      exit (2);
    }
  fseek (f, 0, SEEK_END);
  const long len = ftell (f);
  fseek (f, 0, SEEK_SET);
  uint8_t *p = malloc ((size_t) len + 1);
  if (!p || fread (p, 1, (size_t) len, f) != (size_t) len)
    {
      fprintf (stderr, "pemap_gz_rule_check: cannot read %s\n", path);
      exit (2);
    }
  fclose (f);
  *n = (size_t) len;
  return p;
}

/* the rule's parse as its definition reads: at every position the longest match at distance 16, then on behind it */
static uint32_t
greedy_parse (const uint8_t * t, uint32_t n, uint16_t * tok_pos, uint16_t * tok_len)
{
  uint32_t k = 0;
  for (uint32_t i = 0; i < n;)
    {
      const uint32_t room = n - i < PCG_MAX_MATCH ? n - i : PCG_MAX_MATCH;
      uint32_t m = 0;
      if (i >= PMZ_DIST)
        while (m < room && t[i + m] == t[i + m - PMZ_DIST])
          m++;
      if (m < PCG_MIN_MATCH)
        m = 1;
      tok_pos[k] = (uint16_t) i;
      tok_len[k++] = (uint16_t) m;
      i += m;
    }
  return k;
}

/* the same tokens from the flags held as 32-bit words, the way the deflate kernel holds them (a word per thread) */
static uint32_t
word_parse (const uint8_t * t, uint32_t n, uint16_t * tok_pos, uint16_t * tok_len)
{
  uint32_t flag_w[PMZ_PIECE / 32u], k = 0;
  memset (flag_w, 0, sizeof flag_w);
  for (uint32_t i = PMZ_DIST; i < n; i++)
    if (t[i] == t[i - PMZ_DIST])
      flag_w[i / 32u] |= 1u << (i % 32u);
  for (uint32_t i = 0; i < n; i++)
    {
      const uint32_t w = i / 32u, len = pmz_word_token (flag_w[w], i % 32u, pmz_reach_left (flag_w, w), pmz_reach_right (flag_w, w, PMZ_PIECE / 32u));
      if (len)
        {
          tok_pos[k] = (uint16_t) i;
          tok_len[k++] = (uint16_t) len;
        }
    }
  return k;
}

static int
encode (const char *in_path, const char *out_path)
{
  size_t n;
  uint8_t *t = slurp (in_path, &n);
  FILE *o = fopen (out_path, "wb");
  if (!o)
    {
      fprintf (stderr, "pemap_gz_rule_check: cannot write %s\n", out_path);
      return 2;
    }
  uint8_t *member = malloc (PMZ_MEMBER_MAX);
  uint16_t *pa = malloc (4 * PMZ_PIECE * sizeof (uint16_t)), *la = pa + PMZ_PIECE, *pb = la + PMZ_PIECE, *lb = pb + PMZ_PIECE;
  unsigned long long pieces = 0, bytes = 0, forms[PMZ_FORMS];
  memset (forms, 0, sizeof forms);
  for (size_t a = 0; a < n; a += PMZ_PIECE)
    {
      const uint32_t len = (uint32_t) (n - a < PMZ_PIECE ? n - a : PMZ_PIECE);
      const uint32_t na = pmz_parse (t + a, len, pa, la), nb = greedy_parse (t + a, len, pb, lb);
      int differ = na != nb || memcmp (pa, pb, na * sizeof (uint16_t)) || memcmp (la, lb, na * sizeof (uint16_t));
      const uint32_t nw = word_parse (t + a, len, pb, lb);
      differ |= na != nw || memcmp (pa, pb, na * sizeof (uint16_t)) || memcmp (la, lb, na * sizeof (uint16_t));
      if (differ)
        {
          fprintf (stderr, "pemap_gz_rule_check: piece %llu: the closed form gives %u tokens, the greedy parse %u, the parse by flag words %u, or they differ\n", pieces, na, nb, nw);
          return 1;
        }
      uint32_t form;
      const uint32_t m = pmz_encode_bytes (t + a, len, member, &form);
      if (m > PMZ_HEAD + 5u + len + PMZ_TAIL || form >= PMZ_FORMS || fwrite (member, 1, m, o) != m)
        {
          fprintf (stderr, "pemap_gz_rule_check: a member of %u bytes for a piece of %u, or a failed write\n", m, len);
          return 1;
        }
      forms[form]++;
      pieces++;
      bytes += m;
    }
  if (fclose (o))
    return 2;
  printf ("pieces %llu bytes %llu forms", pieces, bytes);
  for (uint32_t f = 0; f < PMZ_FORMS; f++)
    printf (" %llu", forms[f]);
  printf ("\n");
  free (pa);
  free (member);
  free (t);
  return 0;
}

/* lengths len[0 .. n) -> 1 if their Kraft sum is exactly 1 and code[] holds their canonical codes, bit-reversed */
static int
code_ok (const uint8_t * len, const uint16_t * code, uint32_t n)
{
  uint32_t count[16], next[16], c = 0;
  uint64_t kraft = 0;
  memset (count, 0, sizeof count);
  for (uint32_t s = 0; s < n; s++)
    {
      if (len[s] > 15u)
        return 0;
      if (len[s])
        {
          count[len[s]]++;
          kraft += 1ull << (15u - len[s]);
        }
    }
  if (kraft != 1ull << 15)
    return 0;
  next[0] = 0;
  for (uint32_t b = 1; b < 16u; b++)
    {
      c = (c + (b > 1u ? count[b - 1u] : 0u)) << 1;
      next[b] = c;
    }
  for (uint32_t s = 0; s < n; s++)
    if (len[s] && code[s] != pcg_rev (next[len[s]]++, len[s]))
      return 0;
  return 1;
}

static int
tables (void)
{
  for (uint32_t c = 0; c < PMZ_CODES; c++)
    {
      int bad = 0, b, widest = 0;
      for (uint32_t s = 0; s < 286u; s++)
        bad |= pmz_ll_len[c][s] < 1u || pmz_ll_len[c][s] > 15u;
      bad |= !code_ok (pmz_ll_len[c], pmz_ll_code[c], 286u) || !code_ok (pmz_d_len[c], pmz_d_code[c], 30u);
      bad |= pmz_d_len[c][PMZ_DIST_SYM] == 0u;
      uint32_t used = 0;
      for (uint32_t s = 0; s < 30u; s++)
        used += pmz_d_len[c][s] != 0u;
      bad |= used < 2u;
      bad |= pmz_hdr_bits[c] == 0u || (pmz_hdr_bits[c] + 7u) / 8u > PMZ_HDR_BYTES || (pmz_hdr[c][0] & 7u) != 5u;     /* BFINAL 1, BTYPE 10 */
      for (uint32_t len = 1; len <= PCG_MAX_MATCH; len = len == 1u ? 3u : len + 1u)
        for (uint32_t byte = 0; byte < (len == 1u ? 257u : 1u); byte++)
          {
            pmz_token_preset (c, len, byte, &b);
            widest = b > widest ? b : widest;
          }
      bad |= widest > 31;
      if (bad)
        {
          fprintf (stderr, "pemap_gz_rule_check: preset table %u is not a pair of complete canonical codes within 15 bits\n", c);
          return 1;
        }
    }
  printf ("tables %u ok\n", PMZ_CODES);
  return 0;
}

int
main (int argc, char **argv)
{
  if (argc == 4 && !strcmp (argv[1], "encode"))
    return encode (argv[2], argv[3]);
  if (argc == 2 && !strcmp (argv[1], "tables"))
    return tables ();
  if (argc == 3 && !strcmp (argv[1], "eof"))
    {
      FILE *o = fopen (argv[2], "wb");
      if (!o)
        return 2;
      for (uint32_t k = 0; k < PMZ_EOF_BYTES; k++)
        fputc (pmz_eof_byte (k), o);
      return fclose (o) ? 2 : 0;
    }
  if (argc == 2 && !strcmp (argv[1], "consts"))
    {
      printf ("%u %u %u\n", PMZ_PIECE_RECORDS, PMZ_CODES, PMZ_MEMBER_MAX);
      return 0;
    }
  fprintf (stderr, "usage: pemap_gz_rule_check encode <bytes> <out> | tables | eof <out> | consts\n");
  return 2;
}
