/* fastq_rule_check.c -- walks fastq texts line by line with pecaller_amd/csrc/pemap_fastq_rule.h and prints what the rule makes of them
 * (tests/test_fastq_rule_cpu.py compares the output with the Python model of tests/fastq_cases.py).  Stand-alone, its own main.
 *
 *   fastq_rule_check MANIFEST
 * Every line of the manifest is one of
 *   mate FILE STATE TRIM_START TRIM_END FIRST_MATE MAX_RECORDS   -> "mate GOT END BAD_LEN", then a "rec OFFSET LEN NEXT" per counted record
 *   pair GOT1 GOT2 PAIRED                                         -> "pair N"
 * Beside the walk the program composes the lines' maps (pfq_map_of_line, pfq_map_then) and checks after every line that the composed
 * map sends the walk's first state to its current one: exit status 2 if it ever does not. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../pecaller_amd/csrc/pemap_fastq_rule.h"

#define MIN_READ 16
#define MAX_READ 278

static int
one_mate (const char *path, int state_in, int trim_start, int trim_end, int first_mate, int max_records)
{
  FILE *f = fopen (path, "rb");
  if (!f)
    return 3;
  fseek (f, 0, SEEK_END);
  long bytes = ftell (f);
  fseek (f, 0, SEEK_SET);
  char *text = (char *) malloc (bytes > 0 ? (size_t) bytes : 1);
  if (bytes > 0 && fread (text, 1, (size_t) bytes, f) != (size_t) bytes)
    return 3;
  fclose (f);
  long *offs = (long *) malloc (sizeof (long) * 3 * (size_t) (bytes + 1));
  const int first_state = pfq_state_in (state_in);
  int state = first_state, got = 0, end = -1, bad_len = 0;
  long k = 0, pos = 0;
  unsigned composed = PFQ_MAP_IDENTITY;
  while (pos < bytes)
    {
      const char *nl = (const char *) memchr (text + pos, '\n', (size_t) (bytes - pos));
      if (!nl)
        break;                  /* an incomplete line is never looked at */
      const long full = (long) (nl - (text + pos));
      const int at = full > 0 && text[pos] == '@';
      if (state == PFQ_SEQ)
        {
          if (k < max_records && end < 0)
            {
              long skip;
              const long sl = pfq_read_len (full, trim_start, trim_end, &skip);
              const int cls = pfq_classify (sl, first_mate, MIN_READ, MAX_READ);
              if (cls == PFQ_COUNTS)
                {
                  offs[3 * got] = pos + skip;
                  offs[3 * got + 1] = sl;
                  offs[3 * got + 2] = pos + full + 1;
                  got++;
                }
              else
                {
                  end = cls;
                  if (cls == PFQ_END_BAD_LEN)
                    bad_len = (int) sl;
                }
            }
          k++;
        }
      state = pfq_next (state, at);
      composed = pfq_map_then (composed, pfq_map_of_line (at));
      if (pfq_map_apply (composed, first_state) != state)
        return 2;
      pos += full + 1;
    }
  if (end < 0)
    end = pfq_end_unstopped (got, max_records);
  printf ("mate %d %d %d\n", got, end, bad_len);
  for (int i = 0; i < got; i++)
    printf ("rec %ld %ld %ld\n", offs[3 * i], offs[3 * i + 1], offs[3 * i + 2]);
  free (offs);
  free (text);
  return 0;
}

int
main (int argc, char **argv)
{
  if (argc != 2)
    return 1;
  FILE *m = fopen (argv[1], "r");
  if (!m)
    return 1;
  /* the maps: composition is associative, the identity is neutral, and a map applied is pfq_next */
  const unsigned a = pfq_map_of_line (0), b = pfq_map_of_line (1);
  const unsigned three[3] = { a, b, PFQ_MAP_IDENTITY };
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      for (int l = 0; l < 3; l++)
        if (pfq_map_then (pfq_map_then (three[i], three[j]), three[l]) != pfq_map_then (three[i], pfq_map_then (three[j], three[l])))
          return 2;
  for (int s = 0; s < PFQ_STATES; s++)
    if (pfq_map_apply (a, s) != pfq_next (s, 0) || pfq_map_apply (b, s) != pfq_next (s, 1) || pfq_map_apply (PFQ_MAP_IDENTITY, s) != s)
      return 2;
  char word[16], path[4096];
  while (fscanf (m, "%15s", word) == 1)
    {
      if (!strcmp (word, "mate"))
        {
          int st, ts, te, fm, mr;
          if (fscanf (m, "%4095s %d %d %d %d %d", path, &st, &ts, &te, &fm, &mr) != 6)
            return 1;
          const int rc = one_mate (path, st, ts, te, fm, mr);
          if (rc)
            return rc;
        }
      else if (!strcmp (word, "pair"))
        {
          int g1, g2, paired;
          if (fscanf (m, "%d %d %d", &g1, &g2, &paired) != 3)
            return 1;
          printf ("pair %d\n", pfq_pairs (g1, g2, paired));
        }
      else
        return 1;
    }
  fclose (m);
  return 0;
}
