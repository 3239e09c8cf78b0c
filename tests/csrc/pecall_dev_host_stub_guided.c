/* The host-only stand-in of pecall_dev_host_stub.c with pecall_dev_call_records_guided beside it (include/pemap_hip.h), in plain C: a
   direct build of the guided columns -- a column at every slot of the intervals, a sample's record where it has one there, zeros
   where it has none, records outside every interval checked and ignored -- and the same "call" as the stand-in's
   (tests/test_pecaller_host_guided_cpu.py). */
#include "pecall_dev_host_stub.c"

int
pecall_dev_call_records_guided (pecall_dev * dev, const void *const *recs, const uint64_t * n_recs, int indiv, uint32_t p0, uint32_t span,
                                const char *ref_letters, uint32_t ref_len, const uint32_t * iv_first, const uint32_t * iv_count, const uint8_t * iv_chrom,
                                uint32_t n_iv, long *n_cols, uint32_t * col_slot, int haploid, double threshold, double theta, int8_t * call,
                                uint32_t * post_site, double *post_rows, uint64_t post_cap, uint64_t * n_post, int8_t * site_type, int32_t * allele_count,
                                int8_t * n_pass, int32_t * denovo)
{
  (void) iv_chrom, (void) haploid, (void) threshold, (void) theta, (void) post_site, (void) post_rows, (void) post_cap;
  *n_cols = 0;
  *n_post = 0;
  if (span < 1 || span > (1u << 22) || ref_len > span)
    {
      snprintf (dev->err, sizeof dev->err, "pecall_dev_host_stub: span %u, %u letters", span, ref_len);
      return 1;
    }
  uint64_t next = 0;
  for (uint32_t k = 0; k < n_iv; k++)
    {
      if (iv_count[k] < 1 || (uint64_t) iv_first[k] + iv_count[k] > span || iv_first[k] < next)
        {
          snprintf (dev->err, sizeof dev->err, "pecall_dev_host_stub: interval %u is empty, leaves the range or is out of order", k);
          return 1;
        }
      next = (uint64_t) iv_first[k] + iv_count[k];
    }
  if (n_iv == 0)
    return 0;
  /* slot -> column + 1, 0: no column */
  uint32_t *col_of = (uint32_t *) calloc (span, sizeof (uint32_t));
  long n = 0;
  for (uint32_t k = 0; k < n_iv; k++)
    for (uint32_t q = 0; q < iv_count[k]; q++)
      {
        const uint32_t slot = iv_first[k] + q;
        if (col_slot)
          col_slot[n] = slot;
        col_of[slot] = (uint32_t) ++n;
      }
  dev->n_cols = *n_cols = n;
  dev->indiv = indiv;
  dev->cols = (uint16_t *) realloc (dev->cols, (size_t) n * indiv * 6 * sizeof (uint16_t));
  memset (dev->cols, 0, (size_t) n * indiv * 6 * sizeof (uint16_t));
  for (int i = 0; i < indiv; i++)
    {
      uint64_t next_min = p0;
      for (uint64_t r = 0; r < n_recs[i]; r++)
        {
          const char *rec = (const char *) recs[i] + r * 16;
          uint32_t pos;
          memcpy (&pos, rec, 4);
          if (pos < next_min || (uint64_t) pos >= (uint64_t) p0 + span)
            {
              snprintf (dev->err, sizeof dev->err, "pecall_dev_host_stub: sample %d, record %llu out of order", i, (unsigned long long) r);
              free (col_of);
              dev->n_cols = *n_cols = 0;
              return PECALL_RC_UNORDERED;
            }
          next_min = (uint64_t) pos + 1;
          if (col_of[pos - p0])
            memcpy (dev->cols + ((size_t) (col_of[pos - p0] - 1) * indiv + i) * 6, rec + 4, 12);
        }
    }
  uint8_t *ref_base = (uint8_t *) malloc ((size_t) n);
  for (uint32_t slot = 0; slot < span; slot++)
    if (col_of[slot])
      {
        const char *p = slot < ref_len && ref_letters[slot] ? strchr ("ACGT", ref_letters[slot]) : NULL;
        ref_base[col_of[slot] - 1] = p ? (uint8_t) (p - "ACGT") : 255;
      }
  call_columns (ref_base, n, indiv, call, n_post, site_type, allele_count, n_pass, denovo);
  free (ref_base);
  free (col_of);
  return 0;
}
