/* seed_entry_check.c -- pm_seed_entry_at (pecaller_amd/csrc/pemap_seed_entry.h), the per-lane address arithmetic of
   pm_seed4_kernel's entry requests, for a list of k-mers and all 64 lanes: out[64 i + lane] = the index of the lane's entry in the
   replicas taken as one array (replica << 32 | index inside it), or -1 for a lane that takes no part.  Built as a small shared
   object by tests/test_seed4_entry_index_cpu.py, which holds the table against the neighbour order and the replicas' permutation. */
#include <stdint.h>
#include "../../pecaller_amd/csrc/pemap_seed_entry.h"

void
seed_entry_table (const uint32_t * kmers, long n, int64_t * out)
{
  for (long i = 0; i < n; i++)
    for (int lane = 0; lane < 64; lane++)
      out[64 * i + lane] = pm_seed_entry_at (kmers[i], lane);
}

/* the same through the two steps the kernel takes: what a lane knows beforehand, then the k-mer */
void
seed_entry_table_two_step (const uint32_t * kmers, long n, int64_t * out)
{
  PmSeedEntryLane L[64];
  for (int lane = 0; lane < 64; lane++)
    L[lane] = pm_seed_entry_lane (lane);
  for (long i = 0; i < n; i++)
    for (int lane = 0; lane < 64; lane++)
      out[64 * i + lane] = L[lane].on ? (int64_t) (((uint64_t) pm_seed_entry_replica (L[lane]) << 32) + pm_seed_entry_index (kmers[i], L[lane])) : -1;
}
