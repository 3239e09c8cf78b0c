/* A host-only stand-in for the nine pecall_dev_* entries that pecaller_amd/csrc/pecaller_main.c uses (include/pemap_hip.h): plain C,
   no device.  Every column whose reference letter is A/C/G/T is "called" as that letter with posterior 1 and site type 1, so that the
   host program writes every such column to <out>.piles.gz and its stream walk can be read back exactly (tests/test_pecaller_host_cpu.py).
   pin_host / unpin_host keep a table: an unpin of a range that is not pinned, or a range still pinned at destroy, makes destroy
   print a line to stderr. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "../../include/pemap_hip.h"

#define MAX_PINS 256
struct pecall_dev
{
  const void *pin[MAX_PINS];
  int n_pins, bad_unpins;
  uint16_t *cols;               /* call_records: the merged columns [n_cols][indiv][6], kept for sites_gather */
  uint8_t *mark;
  long n_cols;
  int indiv;
  char err[256];
};

int
pecall_dev_create (pecall_dev ** out, int device_id)
{
  (void) device_id;
  *out = (pecall_dev *) calloc (1, sizeof (pecall_dev));
  return *out ? 0 : 1;
}

void
pecall_dev_destroy (pecall_dev * dev)
{
  if (!dev)
    return;
  if (dev->n_pins || dev->bad_unpins)
    fprintf (stderr, "pecall_dev_host_stub: %d ranges still pinned at destroy, %d unpins of ranges that were not pinned\n", dev->n_pins, dev->bad_unpins);
  free (dev->cols);
  free (dev->mark);
  free (dev);
}

const char *
pecall_dev_last_error (const pecall_dev * dev)
{
  return dev ? dev->err : "pecall_dev_host_stub: no object";
}

int
pecall_dev_pin_host (pecall_dev * dev, const void *host_ptr, uint64_t n_bytes)
{
  (void) n_bytes;
  if (dev->n_pins == MAX_PINS)
    return 1;
  dev->pin[dev->n_pins++] = host_ptr;
  return 0;
}

int
pecall_dev_unpin_host (pecall_dev * dev, const void *host_ptr)
{
  for (int k = 0; k < dev->n_pins; k++)
    if (dev->pin[k] == host_ptr)
      {
        dev->pin[k] = dev->pin[--dev->n_pins];
        return 0;
      }
  dev->bad_unpins++;
  return 1;
}

int
pecall_dev_set_pedigree (pecall_dev * dev, int indiv, const int *dad, const int *mom, const int *sex, const int *kid_off, const int *kid_list,
                         double denovo_rate)
{
  (void) dev, (void) indiv, (void) dad, (void) mom, (void) sex, (void) kid_off, (void) kid_list, (void) denovo_rate;
  return 0;
}

/* the "call" of n columns: the reference base, posterior 1 everywhere (an empty list), type 1 for A/C/G/T and -1 otherwise */
static void
call_columns (const uint8_t * ref_base, long n, int indiv, int8_t * call, uint64_t * n_post, int8_t * site_type, int32_t * allele_count,
              int8_t * n_pass, int32_t * denovo)
{
  for (long s = 0; s < n; s++)
    {
      memset (call + s * indiv, (int8_t) (ref_base[s] <= 3 ? ref_base[s] : 14), (size_t) indiv);
      site_type[s] = ref_base[s] <= 3 ? 1 : -1;
      if (n_pass)
        n_pass[s] = 0;
      denovo[s] = 0;
    }
  memset (allele_count, 0, (size_t) n * 6 * sizeof (int32_t));
  *n_post = 0;
}

int
pecall_dev_call_sites_sparse (pecall_dev * dev, const uint16_t * reads, const uint8_t * ref_base, const uint8_t * chrom_type, long n_sites, int indiv,
                              int haploid, double threshold, double theta, int8_t * call, uint32_t * post_site, double *post_rows, uint64_t post_cap,
                              uint64_t * n_post, int8_t * site_type, int32_t * allele_count, int8_t * n_pass, int32_t * denovo)
{
  (void) dev, (void) reads, (void) chrom_type, (void) haploid, (void) threshold, (void) theta, (void) post_site, (void) post_rows, (void) post_cap;
  call_columns (ref_base, n_sites, indiv, call, n_post, site_type, allele_count, n_pass, denovo);
  return 0;
}

int
pecall_dev_call_records (pecall_dev * dev, const void *const *recs, const uint64_t * n_recs, int indiv, uint32_t p0, uint32_t span,
                         const char *ref_letters, uint32_t ref_len, const uint8_t * chrom_by_slot, long *n_cols, uint32_t * col_slot, int haploid,
                         double threshold, double theta, int8_t * call, uint32_t * post_site, double *post_rows, uint64_t post_cap, uint64_t * n_post,
                         int8_t * site_type, int32_t * allele_count, int8_t * n_pass, int32_t * denovo)
{
  (void) chrom_by_slot, (void) haploid, (void) threshold, (void) theta, (void) post_site, (void) post_rows, (void) post_cap;
  dev->mark = (uint8_t *) realloc (dev->mark, span);
  memset (dev->mark, 0, span);
  for (int i = 0; i < indiv; i++)
    {
      uint64_t next_min = p0;
      for (uint64_t r = 0; r < n_recs[i]; r++)
        {
          uint32_t pos;
          memcpy (&pos, (const char *) recs[i] + r * 16, 4);
          if (pos < next_min || (uint64_t) pos >= (uint64_t) p0 + span)
            {
              snprintf (dev->err, sizeof dev->err, "pecall_dev_host_stub: sample %d, record %llu out of order", i, (unsigned long long) r);
              return PECALL_RC_UNORDERED;
            }
          dev->mark[pos - p0] = 1;
          next_min = (uint64_t) pos + 1;
        }
    }
  /* the union of the positions, ascending: slot -> column through col_of */
  uint32_t *col_of = (uint32_t *) malloc ((size_t) span * sizeof (uint32_t));
  long n = 0;
  for (uint32_t slot = 0; slot < span; slot++)
    if (dev->mark[slot])
      {
        col_of[slot] = (uint32_t) n;
        if (col_slot)
          col_slot[n] = slot;
        n++;
      }
  dev->n_cols = *n_cols = n;
  dev->indiv = indiv;
  dev->cols = (uint16_t *) realloc (dev->cols, (size_t) (n ? n : 1) * indiv * 6 * sizeof (uint16_t));
  memset (dev->cols, 0, (size_t) n * indiv * 6 * sizeof (uint16_t));
  for (int i = 0; i < indiv; i++)
    for (uint64_t r = 0; r < n_recs[i]; r++)
      {
        const char *rec = (const char *) recs[i] + r * 16;
        uint32_t pos;
        memcpy (&pos, rec, 4);
        memcpy (dev->cols + ((size_t) col_of[pos - p0] * indiv + i) * 6, rec + 4, 12);
      }
  uint8_t *ref_base = (uint8_t *) malloc ((size_t) (n ? n : 1));
  for (uint32_t slot = 0; slot < span; slot++)
    if (dev->mark[slot])
      {
        const char *p = slot < ref_len && ref_letters[slot] ? strchr ("ACGT", ref_letters[slot]) : NULL;
        ref_base[col_of[slot]] = p ? (uint8_t) (p - "ACGT") : 255;
      }
  call_columns (ref_base, n, indiv, call, n_post, site_type, allele_count, n_pass, denovo);
  free (ref_base);
  free (col_of);
  return 0;
}

int
pecall_dev_sites_gather (pecall_dev * dev, const uint32_t * cols, uint64_t n, uint16_t * reads_out, uint8_t * ref_base_out, uint8_t * chrom_out)
{
  (void) ref_base_out, (void) chrom_out;
  const size_t row = (size_t) dev->indiv * 6 * sizeof (uint16_t);
  for (uint64_t k = 0; k < n && reads_out; k++)
    {
      const uint64_t c = cols ? cols[k] : k;
      if ((long) c >= dev->n_cols)
        {
          snprintf (dev->err, sizeof dev->err, "pecall_dev_host_stub: column %llu of %ld asked for", (unsigned long long) c, dev->n_cols);
          return 1;
        }
      memcpy ((char *) reads_out + k * row, (const char *) dev->cols + c * row, row);
    }
  return 0;
}
