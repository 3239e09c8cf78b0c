/*
 * pemap_seed_entry.h -- where lane j of a seed wave finds its table entry.  Lane j looks at neighbour j of a segment's k-mer in
 * fill_mers' order (pemapper.c:1969-2003: 0 = the k-mer itself, then the 48 single-substitution neighbours, 2-bit fields from the
 * low end, alternatives ascending), and reads its entry from the look-up replica p (j) in which the k-mer and its neighbours at
 * that pair of bases share a 64-byte line: replica p holds the entry of k-mer k at k with its 4-bit fields 0 and p swapped
 * (pm_swap_fields, pemap_kernels.hip.h; replica p starts 2^32 entries behind replica p - 1).  Lanes 49..63 look at nothing.
 * The 49 indices of one k-mer lie in 8 lines, one per replica: lanes 0..6 in replica 0, 7..12 in replica 1, ... 43..48 in replica 7.
 * Plain C, no HIP types: pm_seed4_kernel (pemap_seed4.hip.h) calls it on the device, tests/csrc/seed_entry_check.c on the host.
 */
#ifndef PEMAP_SEED_ENTRY_H
#define PEMAP_SEED_ENTRY_H
#include <stdint.h>

#ifdef __HIPCC__
#define PM_SEED_ENTRY_FN __host__ __device__
#else
#define PM_SEED_ENTRY_FN
#endif

#define PM_SEED_ENTRY_LANES 49          /* the k-mer and its 48 neighbours */

/* what a lane knows before it sees a k-mer */
typedef struct
{
  uint32_t sh;                  /* the 2-bit field the lane replaces starts at this bit */
  uint32_t mask;                /* 3 << sh; lane 0 (the k-mer itself) replaces nothing: 0 */
  uint32_t rank;                /* rank of the lane's alternative among the three bases that differ from the k-mer's */
  uint32_t p4;                  /* 4 x the replica = the bit at which the 4-bit field around the replaced base starts */
  int on;                       /* the lane takes part */
} PmSeedEntryLane;

static inline PM_SEED_ENTRY_FN PmSeedEntryLane
pm_seed_entry_lane (int lane)
{
  PmSeedEntryLane L;
  const int f = lane > 0 ? ((lane - 1) / 3) & 15 : 0;
  L.sh = 2u * (uint32_t) f;
  L.mask = lane > 0 ? 3u << L.sh : 0u;
  L.rank = lane > 0 ? (uint32_t) ((lane - 1) % 3) : 0u;
  L.p4 = 4u * (uint32_t) (f >> 1);
  L.on = lane >= 0 && lane < PM_SEED_ENTRY_LANES;
  return L;
}

/* the lane's replica */
static inline PM_SEED_ENTRY_FN int
pm_seed_entry_replica (PmSeedEntryLane L)
{
  return (int) (L.p4 >> 2);
}

/* index of the lane's entry inside its replica, for the k-mer k of a segment: the neighbour (pm_neighbour), then fields 0 and
   p swapped by the difference of the two (p = 0: the difference of a field with itself, nothing moves) */
static inline PM_SEED_ENTRY_FN uint32_t
pm_seed_entry_index (uint32_t k, PmSeedEntryLane L)
{
  const uint32_t cur = (k >> L.sh) & 3u;
  const uint32_t alt = L.rank + (L.rank >= cur ? 1u : 0u);
  const uint32_t nb = (k & ~L.mask) | ((alt << L.sh) & L.mask);
  const uint32_t t = ((nb >> L.p4) ^ nb) & 15u;
  return nb ^ t ^ (t << L.p4);
}

/* the same as an index into the replicas as one array: -1 for a lane that takes no part */
static inline PM_SEED_ENTRY_FN int64_t
pm_seed_entry_at (uint32_t k, int lane)
{
  const PmSeedEntryLane L = pm_seed_entry_lane (lane);
  if (!L.on)
    return -1;
  return (int64_t) (((uint64_t) pm_seed_entry_replica (L) << 32) + (uint64_t) pm_seed_entry_index (k, L));
}

#endif
