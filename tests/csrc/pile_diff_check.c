/*
 * pile_diff_check.c -- the difference form of a pileup counter plane (pecaller_amd/csrc/pemap_pile_diff.h) against plain
 * uint16_t arithmetic, on 4,099 positions: an odd count, so the last used word is half used and the padding is part of the array.
 *   (a) fold (unfold (x)) == x for every word;
 *   (b) 100,000 ranges a..b applied as uint16_t increments on a copy, and as the header's two word adds with take-back on the
 *       unfolded array, then folded, agree on every half;
 *   (c) the fold done in tiles of 1, 2, 64 and 4,096 words with carried sums equals the serial fold.
 * Built with -fsanitize=address,undefined by tests/test_pile_diff_cpu.py; prints one summary line and exits non-zero on any
 * disagreement.
 */
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "../../pecaller_amd/csrc/pemap_pile_diff.h"

#define N_POS 4099
/* the plane as index_alloc sizes it: (positions + 2) / 2 words rounded up to a multiple of 64, so position N_POS has a half too */
#define N_WORDS ((((N_POS + 2) / 2) + 63) & ~63)
#define N_HALVES (2 * N_WORDS)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t
rnd (void)
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t) (rng_state >> 16);
}

static uint16_t
half_of (const uint32_t * w, int p)
{
  return (uint16_t) (w[p >> 1] >> (16 * (p & 1)));
}

static void
set_half (uint32_t * w, int p, uint16_t v)
{
  const int sh = 16 * (p & 1);
  w[p >> 1] = (w[p >> 1] & ~(0xFFFFu << sh)) | ((uint32_t) v << sh);
}

static void
unfold (uint32_t * w, int n_words)
{
  /* from the top down, so that a word's predecessor is still a count word when it is read */
  for (int i = n_words - 1; i >= 0; i--)
    w[i] = pm_diff_unfold_word (w[i], i ? w[i - 1] >> 16 : 0u);
}

static void
fold_serial (uint32_t * w, int n_words)
{
  uint32_t carry = 0;
  for (int i = 0; i < n_words; i++)
    {
      w[i] = pm_diff_fold_word (w[i], carry);
      carry = w[i] >> 16;
    }
}

/* the device's way: every tile's sum, an exclusive scan of the sums with pm_diff_combine, every tile folded from its carried sum */
static void
fold_tiled (uint32_t * w, int n_words, int tile)
{
  static uint32_t sums[N_WORDS];
  const int n_tiles = (n_words + tile - 1) / tile;
  for (int t = 0; t < n_tiles; t++)
    {
      uint32_t s = 0;
      for (int i = t * tile; i < (t + 1) * tile && i < n_words; i++)
        s = pm_diff_combine (s, pm_diff_word_sum (w[i]));
      sums[t] = s;
    }
  uint32_t acc = 0;
  for (int t = 0; t < n_tiles; t++)
    {
      const uint32_t s = sums[t];
      sums[t] = acc;
      acc = pm_diff_combine (acc, s);
    }
  for (int t = n_tiles - 1; t >= 0; t--)        /* any order: a tile needs only its carried sum */
    {
      uint32_t carry = sums[t];
      for (int i = t * tile; i < (t + 1) * tile && i < n_words; i++)
        {
          const uint32_t d = w[i];
          w[i] = pm_diff_fold_word (d, carry);
          carry = pm_diff_combine (carry, pm_diff_word_sum (d));
        }
    }
}

/* one half of the difference array changed by +1 or -1 the way the kernels do it: a 32-bit add, the old word, the take-back */
static void
diff_add (uint32_t * w, int p, int sign)
{
  const uint32_t addend = pm_diff_addend (p & 1, sign);
  const uint32_t old = w[p >> 1];
  w[p >> 1] = old + addend;
  w[p >> 1] += pm_diff_takeback (old, addend);
}

int
main (void)
{
  static uint32_t start[N_WORDS], x[N_WORDS], y[N_WORDS];
  static uint16_t plain[N_HALVES];
  long bad = 0;
  for (int i = 0; i < N_WORDS; i++)
    start[i] = rnd ();
  static const uint16_t edge[6] = { 0, 1, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF };
  for (int k = 0; k < 6 * 6 * 4; k++)
    {
      /* every ordered pair of edge values on neighbouring positions, on both parities, scattered over the plane (the last used
         half, the padding and position 0 among them) */
      const int p = (k * 53) % (N_HALVES - 1);
      set_half (start, p, edge[k % 6]);
      set_half (start, p + 1, edge[(k / 6) % 6]);
    }
  set_half (start, 0, 0xFFFF);
  set_half (start, N_POS - 1, 0xFFFF);
  set_half (start, N_POS, 0x8000);
  set_half (start, N_HALVES - 1, 0xFFFE);

  /* (a) */
  memcpy (x, start, sizeof x);
  unfold (x, N_WORDS);
  memcpy (y, x, sizeof y);
  fold_serial (y, N_WORDS);
  for (int i = 0; i < N_WORDS; i++)
    bad += y[i] != start[i];
  const long bad_a = bad;

  /* (c) on the unfolded starting counts */
  long bad_c = 0;
  static const int tiles[4] = { 1, 2, 64, 4096 };
  for (int t = 0; t < 4; t++)
    {
      memcpy (y, x, sizeof y);
      fold_tiled (y, N_WORDS, tiles[t]);
      for (int i = 0; i < N_WORDS; i++)
        bad_c += y[i] != start[i];
    }

  /* (b) */
  for (int p = 0; p < N_HALVES; p++)
    plain[p] = half_of (start, p);
  long n_ranges = 0;
  for (int r = 0; r < 100000; r++)
    {
      int a, b;
      if (r < 70000)
        a = b = 778;            /* 70,000 over one position: its counter passes 65,535, D[778] (a low half) carries */
      else if (r == 70000) { a = 0; b = N_POS - 1; }
      else if (r == 70001) { a = 0; b = 0; }
      else if (r == 70002) { a = N_POS - 1; b = N_POS - 1; }
      else if (r == 70003) { a = 100; b = 199; }        /* ranges that abut */
      else if (r == 70004) { a = 200; b = 301; }
      else if (r == 70005) { a = 302; b = 302; }
      else if (r == 70006) { a = 303; b = 400; }
      else
        {
          a = (int) (rnd () % N_POS);
          b = a + (int) (rnd () % 300);
          if (b >= N_POS)
            b = N_POS - 1;
        }
      for (int p = a; p <= b; p++)
        plain[p]++;
      diff_add (x, a, +1);
      diff_add (x, b + 1, -1);
      n_ranges++;
    }
  memcpy (y, x, sizeof y);
  fold_serial (y, N_WORDS);
  long bad_b = 0;
  for (int p = 0; p < N_HALVES; p++)
    bad_b += half_of (y, p) != plain[p];
  /* the tiled fold of the same array */
  for (int t = 0; t < 4; t++)
    {
      static uint32_t z[N_WORDS];
      memcpy (z, x, sizeof z);
      fold_tiled (z, N_WORDS, tiles[t]);
      for (int i = 0; i < N_WORDS; i++)
        bad_c += z[i] != y[i];
    }
  printf ("%d positions in %d words: round trip %ld words differ; %ld ranges, %ld halves differ; tiled folds %ld words differ\n", N_POS,
          N_WORDS, bad_a, n_ranges, bad_b, bad_c);
  return (bad_a || bad_b || bad_c) ? 1 : 0;
}
