/* pemap_fastq_rule.h -- which lines of a fastq text are reads, and how long the reads are: the rule of fill_rows and map_one_file
 * (pemapper_main.c), which follow the reference's read loop (pemapper.c:649-748, the trims of pemapper_tsw.c:693-704), as arithmetic
 * on lines.  Plain C, shared by the host (tests/csrc/fastq_rule_check.c walks a text with it) and the kernels of pemap_fastq.hip.h,
 * so that there is one statement of the rule.
 *
 * A line is a maximal run of bytes ended by '\n'; the '\n' is not part of it, a '\r' is; bytes behind a text's last '\n' are no line.
 * Every line has a role, given by a walk over the lines of one mate's text:
 *   START  skipped (the first line of a stream)                 -> SEQ
 *   SEQ    a record's sequence line                             -> SKIP1
 *   SKIP1  skipped (normally "+")                               -> SKIP2
 *   SKIP2  skipped whatever it begins with (the qualities)      -> SEEK
 *   SEEK   skipped; begins with '@': -> SEQ, else -> SEEK
 * The walk of a stream begins in START (state_in = 0); a piece that continues behind a sequence line begins in SKIP1 (state_in = 1). */
#ifndef PEMAP_FASTQ_RULE_H
#define PEMAP_FASTQ_RULE_H

#ifdef __HIPCC__
#define PFQ_FN static __host__ __device__ __forceinline__
#else
#define PFQ_FN static inline
#endif

enum { PFQ_START = 0, PFQ_SEQ = 1, PFQ_SKIP1 = 2, PFQ_SKIP2 = 3, PFQ_SEEK = 4, PFQ_STATES = 5 };

/* a length's class */
enum { PFQ_COUNTS = 0, PFQ_END_FULL = 0, PFQ_END_TEXT = 1, PFQ_END_SHORT_FIRST = 2, PFQ_END_BAD_LEN = 3 };

#define PFQ_MAX_TEXT (1u << 30) /* bytes of one mate's text per call: offsets are 32-bit */

/* the walk's state for state_in (0 or 1; anything else is refused before it gets here) */
PFQ_FN int pfq_state_in (int state_in)
{
  return state_in ? PFQ_SKIP1 : PFQ_START;
}

/* the state of the line behind a line that was met in `state`; at = the line's first byte is '@' (an empty line: 0) */
PFQ_FN int pfq_next (int state, int at)
{
  switch (state)
    {
    case PFQ_START: return PFQ_SEQ;
    case PFQ_SEQ: return PFQ_SKIP1;
    case PFQ_SKIP1: return PFQ_SKIP2;
    case PFQ_SKIP2: return PFQ_SEEK;
    default: return at ? PFQ_SEQ : PFQ_SEEK;
    }
}

/* A line's effect on the walk as a map of the five states onto the five states, three bits a state (15 bits): map >> 3 s & 7 is the
 * state behind the line when it was met in state s.  There are two such maps, and composition is associative: a scan gives every line
 * its state. */
PFQ_FN unsigned pfq_map_of_line (int at)
{
  unsigned m = 0;
  for (int s = 0; s < PFQ_STATES; s++)
    m |= (unsigned) pfq_next (s, at) << (3 * s);
  return m;
}

#define PFQ_MAP_IDENTITY (0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12)

PFQ_FN int pfq_map_apply (unsigned map, int state)
{
  return (int) ((map >> (3 * state)) & 7u);
}

/* first `a`, then `b` */
PFQ_FN unsigned pfq_map_then (unsigned a, unsigned b)
{
  unsigned m = 0;
  for (int s = 0; s < PFQ_STATES; s++)
    m |= (unsigned) pfq_map_apply (b, pfq_map_apply (a, s)) << (3 * s);
  return m;
}

/* The read of a sequence line of `full` bytes: *skip = bytes into the line at which the read's row begins, the return value its
 * length (sl of fill_rows: full - trim_start; the row begins at the line's end when that is negative; less trim_end; never below 0). */
PFQ_FN long pfq_read_len (long full, int trim_start, int trim_end, long *skip)
{
  long sl = full - trim_start;
  *skip = sl >= 0 ? trim_start : full;
  sl -= trim_end;
  return sl < 0 ? 0 : sl;
}

/* what a read of length sl does to its mate's count: PFQ_COUNTS, or the `end` that stops the mate there.  The rule of the short read
 * looks at the first mate only and comes first (pemapper.c:663). */
PFQ_FN int pfq_classify (long sl, int first_mate, int min_read, int max_read)
{
  if (first_mate && sl <= 12)
    return PFQ_END_SHORT_FIRST;
  if (sl < min_read || sl > max_read)
    return PFQ_END_BAD_LEN;
  return PFQ_COUNTS;
}

/* `end` of a mate that was not stopped by a length: the batch is full, or the text ran out of complete records */
PFQ_FN int pfq_end_unstopped (int got, int max_records)
{
  return got == max_records ? PFQ_END_FULL : PFQ_END_TEXT;
}

/* pairs in the batch: the shorter of the two counts (the reference's loop ends with the first file that runs out) */
PFQ_FN int pfq_pairs (int got1, int got2, int paired)
{
  return paired ? (got1 < got2 ? got1 : got2) : got1;
}

#endif
