/*
 * pemap_gz_rule.h -- how the pileup records of <out>.pileup.gz become gzip members on the device (pemap_dev_fetch_records_gz), stated
 * once.  Plain C, no HIP types: the kernels of pemap_gz.hip.h call these on the device, pemapper_main.c and
 * tests/csrc/pemap_gz_rule_check.c on the host.  pmz_encode_piece is the serial statement the kernels are held to, byte for byte.
 * The bit reversal, the length and distance code arithmetic of the fixed form and the CRC-32 are pecall_gz_rule.h's, called as they are.
 *
 * Pieces.  The records a call returns -- 16 bytes each, {u32 pos; u16 A, C, G, T, Del, Ins}, little-endian, positions ascending -- are
 * cut into pieces of PMZ_PIECE_RECORDS = 512 records (8,192 bytes); the last piece of a call may be shorter, a call without records
 * has no piece.  512 and not 1,024: the deflate kernel keeps the piece, the member and its tables in 23 KB of LDS, so six
 * workgroups fit a CU's 160 KB where 1,024 records (about 41 KB) would leave three; a preset code's header is about 3 % of a member
 * of 512 records, which is what the longer piece could save at most.
 *
 * Member.  A piece becomes one complete gzip member (RFC 1952) in the BGZF layout: the 18 bytes 1f 8b 08 04, 00 00 00 00 (mtime),
 * 00 ff, 06 00 (one extra field of six bytes), 42 43 02 00 ('B' 'C', two bytes), the member's total length minus 1 as a little-endian
 * u16; one final deflate block; the CRC-32 of the piece and its length, little-endian.  A member is at most PMZ_MEMBER_MAX = 8,223
 * bytes, far under 65,536, so a reader finds every member boundary from the heads alone.  A file of members ends with the 28-byte
 * empty member pmz_eof_byte spells.
 *
 * Parse.  With t[0 .. n) the piece, position i has ONE candidate: distance 16 (the same byte of the previous record), if i >= 16.
 * Its match is the longest m <= min (258, n - i) with t[i + k] == t[i + k - 16] for all k < m; fewer than 3 bytes gives a literal.
 * Greedy: after a match of m the parse goes on at i + m, after a literal at i + 1; nothing is deferred.
 *   Consequence.  Let e[i] = (i >= 16 && t[i] == t[i - 16]).  The match at i is the run of set flags from i on, cut at 258, and a
 * greedy parse that enters a maximal run of r set flags at its first byte (it always does: the byte in front has e = 0 and is a
 * literal, or is the piece's start) leaves it only at its end.  So the tokens follow from the maximal runs of e alone, with no
 * walk from token to token (which pcg_deflate_kernel needs, having two candidates):
 *   - a byte with e = 0 is a literal;
 *   - a run of r >= 3 goes as r / 258 matches of 258 and then the remainder r % 258: one match if it is >= 3, literals otherwise;
 *   - a run of 1 or 2 is literals.
 * pmz_token_at is that, per byte, from the byte's offset in its run and the run's length.  Positions ascend strictly, so of the four
 * position bytes of a record at least one differs from the previous record's: a run of set flags holds at most the position bytes
 * behind that one (3), the twelve counter bytes and the next record's position bytes in front of its own differing one (3), and no
 * run of real records exceeds 18 bytes.  The cap at
 * 258 stays in the rule and in the kernel; it is reachable only by the arbitrary bytes of the check program.  NO GPU TEST REACHES IT.
 *
 * Codes.  PMZ_CODES preset codes are committed below as data: for each a length for every one of the 286 literal/length symbols
 * (none 0, none above 15), lengths for the 30 distance symbols (symbol 7, the only one used -- distance 16 is symbol 7 with the two
 * extra bits 1 1 -- and symbol 0, one bit each, so that the distance code is complete and not RFC 1951's one-code special case), the
 * canonical codes of those lengths bit-reversed, ready for the stream, and the block's ready-made header bits: BFINAL = 1,
 * BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code and the lengths coded with it.  Both codes of every table are complete
 * (Kraft sum exactly 1).  A token is at most 15 + 5 + 1 + 2 = 23 bits under a preset code and 31 under the fixed one.
 *   Per piece the smallest of these goes out: the stored form (5 + n bytes), the fixed-code form (pecall_gz_rule.h's), each preset
 * form with its header bits counted; ties go to the earlier in that order.  So no member is larger than its fixed-code form.
 * The tables come from tools/pileup_gz_tables.py, which prints the section between the two marks below: synthetic records (reads of
 * 150 at random over a random genome, 0.4 % errors) at the depths named there, symbol counts under this parse, Huffman codes limited
 * to 15 bits.
 */
#ifndef PEMAP_GZ_RULE_H
#define PEMAP_GZ_RULE_H
#include <stdint.h>
#include "pecall_gz_rule.h"

#ifdef __HIPCC__
#define PMZ_FN __device__       /* (the tables below are device data under hipcc: the host side of the library does not encode) */
#define PMZ_DATA static __device__
#else
#define PMZ_FN
#define PMZ_DATA static
#endif

#define PMZ_PIECE_RECORDS 512u
#define PMZ_RECORD 16u
#define PMZ_PIECE (PMZ_RECORD * PMZ_PIECE_RECORDS)
#define PMZ_DIST 16u
#define PMZ_DIST_SYM 7u         /* distance 16: symbol 7, two extra bits of value 3 */
#define PMZ_HEAD 18u
#define PMZ_TAIL 8u
#define PMZ_MEMBER_MAX (PMZ_HEAD + 5u + PMZ_PIECE + PMZ_TAIL)
#define PMZ_EOF_BYTES 28u
#define PMZ_FORM_STORED 0u
#define PMZ_FORM_FIXED 1u       /* form 2 + k: preset code k */

/* ---- generated by tools/pileup_gz_tables.py: begin (do not edit by hand) */
#define PMZ_CODES 3u
#define PMZ_HDR_BYTES 72u      /* of the longest ready-made block header */
/* table 0: made from synthetic records at depth 1x and 5x */
/* table 1: made from synthetic records at depth 30x */
/* table 2: made from synthetic records at depth 100x and 300x */
PMZ_DATA const uint8_t pmz_ll_len[PMZ_CODES][286] = {
  {
    2, 4, 5, 6, 6, 6, 7, 7, 7, 8, 9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
    10, 10, 10, 11, 10, 10, 10, 10, 10, 10, 11, 10, 11, 10, 10, 10, 10, 10, 10, 11, 10, 11, 11, 11,
    11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11,
    11, 11, 11, 11, 11, 11, 10, 11, 10, 10, 10, 11, 10, 11, 11, 10, 10, 10, 11, 11, 10, 11, 10, 11,
    11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11,
    11, 10, 10, 10, 11, 11, 10, 10, 10, 11, 10, 11, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
    10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
    10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
    10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
    10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
    10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 12, 3, 12, 3, 13, 4, 15, 5,
    15, 11, 12, 5, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15
  },
  {
    2, 6, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 9, 9, 8, 8, 8, 7,
    7, 7, 7, 7, 7, 6, 6, 7, 7, 7, 7, 7, 7, 7, 8, 8, 9, 9, 9, 9, 10, 10, 10, 10,
    10, 10, 10, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10,
    11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10,
    11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10,
    11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10,
    11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 10, 11, 11, 11, 11, 11, 11, 11, 11,
    11, 11, 11, 11, 11, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
    10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
    10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
    10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 12, 3, 12, 3, 13, 4, 15, 5,
    15, 8, 12, 5, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15
  },
  {
    2, 3, 6, 9, 10, 10, 11, 11, 11, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
    10, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9,
    9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10,
    10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 9, 9, 9, 9, 9, 9, 9, 9, 9, 8, 8, 8, 8,
    8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10,
    10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11,
    11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11,
    11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11,
    11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11,
    11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11,
    11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 11, 12, 3, 6, 3, 7, 5, 9, 6,
    15, 9, 13, 8, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 14
  }
};
PMZ_DATA const uint16_t pmz_ll_code[PMZ_CODES][286] = {
  {
    0, 1, 5, 29, 61, 3, 35, 99, 19, 83, 211, 467, 979, 51, 563, 307,
    819, 179, 691, 435, 947, 115, 627, 371, 883, 243, 755, 623, 499, 1011, 11, 523,
    267, 779, 1647, 139, 367, 651, 395, 907, 75, 587, 331, 1391, 843, 879, 1903, 239,
    1263, 751, 1775, 495, 1519, 1007, 2031, 31, 1055, 543, 1567, 287, 1311, 799, 1823, 159,
    1183, 671, 1695, 415, 1439, 927, 1951, 95, 1119, 607, 1631, 351, 1375, 863, 203, 1887,
    715, 459, 971, 223, 43, 1247, 735, 555, 299, 811, 1759, 479, 171, 1503, 683, 991,
    2015, 63, 1087, 575, 1599, 319, 1343, 831, 1855, 191, 1215, 703, 1727, 447, 1471, 959,
    1983, 127, 1151, 639, 1663, 383, 1407, 895, 1919, 427, 939, 107, 255, 1279, 619, 363,
    875, 767, 235, 1791, 747, 491, 1003, 27, 539, 283, 795, 155, 667, 411, 923, 91,
    603, 347, 859, 219, 731, 475, 987, 59, 571, 315, 827, 187, 699, 443, 955, 123,
    635, 379, 891, 251, 763, 507, 1019, 7, 519, 263, 775, 135, 647, 391, 903, 71,
    583, 327, 839, 199, 711, 455, 967, 39, 551, 295, 807, 167, 679, 423, 935, 103,
    615, 359, 871, 231, 743, 487, 999, 23, 535, 279, 791, 151, 663, 407, 919, 87,
    599, 343, 855, 215, 727, 471, 983, 55, 567, 311, 823, 183, 695, 439, 951, 119,
    631, 375, 887, 247, 759, 503, 1015, 15, 527, 271, 783, 143, 655, 399, 911, 79,
    591, 335, 847, 207, 719, 463, 975, 47, 559, 303, 815, 175, 687, 431, 943, 111,
    1535, 2, 3583, 6, 3071, 9, 7167, 21, 23551, 511, 1023, 13, 15359, 31743, 2047, 18431,
    10239, 26623, 6143, 22527, 14335, 30719, 4095, 20479, 12287, 28671, 8191, 24575, 16383, 32767
  },
  {
    0, 5, 243, 755, 499, 1011, 11, 523, 267, 779, 139, 651, 395, 907, 75, 587,
    331, 843, 51, 307, 99, 227, 19, 53, 117, 13, 77, 45, 109, 37, 21, 29,
    93, 61, 125, 3, 67, 35, 147, 83, 179, 435, 115, 371, 203, 715, 459, 971,
    43, 555, 299, 811, 751, 171, 1775, 683, 495, 427, 1519, 939, 1007, 107, 2031, 619,
    31, 363, 1055, 875, 543, 235, 1567, 747, 287, 491, 1311, 1003, 799, 27, 1823, 539,
    159, 283, 1183, 795, 671, 155, 1695, 667, 415, 411, 1439, 923, 927, 91, 1951, 603,
    95, 347, 1119, 859, 607, 219, 1631, 731, 351, 475, 1375, 987, 863, 59, 1887, 571,
    223, 315, 1247, 827, 735, 187, 1759, 699, 479, 443, 1503, 955, 991, 123, 2015, 635,
    63, 379, 1087, 891, 575, 251, 1599, 763, 319, 507, 1343, 1019, 831, 7, 1855, 519,
    191, 263, 1215, 775, 703, 135, 1727, 647, 447, 391, 1471, 903, 959, 71, 1983, 583,
    127, 1151, 639, 1663, 383, 1407, 895, 1919, 255, 1279, 767, 1791, 511, 327, 839, 199,
    711, 455, 967, 39, 551, 295, 807, 167, 679, 423, 935, 103, 615, 359, 871, 231,
    743, 487, 999, 23, 535, 279, 791, 151, 663, 407, 919, 87, 599, 343, 855, 215,
    727, 471, 983, 55, 567, 311, 823, 183, 695, 439, 951, 119, 631, 375, 887, 247,
    759, 503, 1015, 15, 527, 271, 783, 143, 655, 399, 911, 79, 591, 335, 847, 207,
    719, 463, 975, 47, 559, 303, 815, 175, 687, 431, 943, 111, 623, 367, 879, 239,
    1535, 2, 3583, 6, 3071, 1, 7167, 9, 23551, 211, 1023, 25, 15359, 31743, 2047, 18431,
    10239, 26623, 6143, 22527, 14335, 30719, 4095, 20479, 12287, 28671, 8191, 24575, 16383, 32767
  },
  {
    0, 2, 21, 227, 71, 583, 759, 1783, 503, 327, 839, 199, 711, 455, 967, 39,
    551, 295, 807, 167, 679, 423, 935, 103, 615, 483, 19, 275, 147, 403, 83, 339,
    211, 467, 51, 307, 179, 435, 115, 371, 243, 499, 11, 267, 139, 395, 75, 331,
    203, 459, 43, 299, 171, 427, 107, 363, 235, 491, 27, 359, 871, 231, 743, 487,
    999, 23, 535, 279, 791, 151, 663, 407, 919, 87, 599, 343, 855, 215, 727, 471,
    983, 55, 567, 283, 155, 411, 91, 347, 219, 475, 59, 315, 109, 237, 29, 157,
    93, 221, 61, 189, 125, 253, 3, 131, 67, 195, 35, 163, 187, 443, 123, 379,
    251, 507, 7, 263, 311, 823, 183, 695, 439, 951, 119, 631, 375, 887, 247, 1527,
    1015, 2039, 15, 1039, 527, 1551, 271, 1295, 783, 1807, 143, 1167, 655, 1679, 399, 1423,
    911, 1935, 79, 1103, 591, 1615, 335, 1359, 847, 1871, 207, 1231, 719, 1743, 463, 1487,
    975, 1999, 47, 1071, 559, 1583, 303, 1327, 815, 1839, 175, 1199, 687, 1711, 431, 1455,
    943, 1967, 111, 1135, 623, 1647, 367, 1391, 879, 1903, 239, 1263, 751, 1775, 495, 1519,
    1007, 2031, 31, 1055, 543, 1567, 287, 1311, 799, 1823, 159, 1183, 671, 1695, 415, 1439,
    927, 1951, 95, 1119, 607, 1631, 351, 1375, 863, 1887, 223, 1247, 735, 1759, 479, 1503,
    991, 2015, 63, 1087, 575, 1599, 319, 1343, 831, 1855, 191, 1215, 703, 1727, 447, 1471,
    959, 1983, 127, 1151, 639, 1663, 383, 1407, 895, 1919, 255, 1279, 767, 1791, 511, 1535,
    1023, 6, 53, 1, 45, 5, 135, 13, 15359, 391, 3071, 99, 31743, 2047, 18431, 10239,
    26623, 6143, 22527, 14335, 30719, 4095, 20479, 12287, 28671, 8191, 24575, 16383, 32767, 7167
  }
};
PMZ_DATA const uint8_t pmz_d_len[PMZ_CODES][30] = {
  {
    1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0
  },
  {
    1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0
  },
  {
    1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0
  }
};
PMZ_DATA const uint16_t pmz_d_code[PMZ_CODES][30] = {
  {
    0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0
  },
  {
    0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0
  },
  {
    0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0
  }
};
PMZ_DATA const uint16_t pmz_hdr_bits[PMZ_CODES] = { 462, 575, 384 };
PMZ_DATA const uint8_t pmz_hdr[PMZ_CODES][PMZ_HDR_BYTES] = {
  {
    237, 231, 101, 224, 125, 85, 185, 254, 225, 126, 158, 49, 231, 92, 107, 125, 127, 116, 135, 164, 72, 138, 221, 221,
    173, 8, 136, 2, 138, 216, 221, 45, 160, 128, 72, 119, 119, 119, 119, 119, 119, 119, 119, 119, 119, 236, 123, 223,
    255, 231, 140, 227, 30, 167, 59, 175, 119, 23, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0
  },
  {
    237, 231, 101, 160, 182, 101, 185, 182, 225, 238, 55, 221, 241, 190, 99, 140, 39, 239, 251, 233, 49, 222, 160, 17,
    17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17, 17,
    17, 17, 177, 155, 238, 238, 238, 238, 238, 238, 174, 121, 204, 227, 59, 215, 181, 198, 188, 86, 119, 110, 255, 54
  },
  {
    237, 231, 99, 160, 94, 105, 194, 181, 237, 158, 99, 166, 170, 187, 203, 70, 108, 219, 40, 219, 140, 147, 101, 35,
    78, 89, 109, 219, 182, 109, 219, 182, 109, 219, 238, 126, 198, 28, 247, 149, 185, 243, 174, 109, 235, 59, 254, 29,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0
  }
};
/* ---- generated by tools/pileup_gz_tables.py: end */
#define PMZ_FORMS (2u + PMZ_CODES)

/* the pieces of n records */
static inline PCG_FN uint64_t
pmz_pieces (uint64_t n_records)
{
  return (n_records + PMZ_PIECE_RECORDS - 1u) / PMZ_PIECE_RECORDS;
}

/* byte k < PMZ_HEAD of a member of member_len bytes in all */
static inline PCG_FN uint8_t
pmz_head_byte (uint32_t k, uint32_t member_len)
{
  switch (k)
    {
    case 0: return 0x1fu;
    case 1: return 0x8bu;
    case 2: return 0x08u;
    case 3: return 0x04u;
    case 9: return 0xffu;
    case 10: return 0x06u;
    case 12: return 0x42u;
    case 13: return 0x43u;
    case 14: return 0x02u;
    case 16: return (uint8_t) (member_len - 1u);
    case 17: return (uint8_t) ((member_len - 1u) >> 8);
    default: return 0u;
    }
}

/* byte k < PMZ_EOF_BYTES of the empty member that ends a file: the head, the empty fixed-code block 03 00, CRC 0, length 0 */
static inline PCG_FN uint8_t
pmz_eof_byte (uint32_t k)
{
  return k < PMZ_HEAD ? pmz_head_byte (k, PMZ_EOF_BYTES) : k == PMZ_HEAD ? 0x03u : 0u;
}

/* The token that begins at a byte whose flag is set, o bytes into a maximal run of r set flags (o < r):
   0 none (the byte lies inside a match), 1 a literal, else a match of that length. */
static inline PCG_FN uint32_t
pmz_token_at (uint32_t o, uint32_t r)
{
  const uint32_t full = r / PCG_MAX_MATCH * PCG_MAX_MATCH, rem = r - full;
  if (o < full)
    return o % PCG_MAX_MATCH == 0u ? PCG_MAX_MATCH : 0u;
  if (rem < PCG_MIN_MATCH)
    return 1u;
  return o == full ? rem : 0u;
}

/* The flags by words, as the kernel holds them: bit j of flag_w[k] is e[32 k + j], zero from the piece's end on.  The set bits of w
   from bit 0 up, and from bit 31 down */
static inline PCG_FN uint32_t
pmz_ones_up (uint32_t w)
{
  return ~w ? (uint32_t) __builtin_ctz (~w) : 32u;
}

static inline PCG_FN uint32_t
pmz_ones_down (uint32_t w)
{
  return ~w ? (uint32_t) __builtin_clz (~w) : 32u;
}

/* the set flags that end directly in front of word k, and that begin directly behind it */
static inline PCG_FN uint32_t
pmz_reach_left (const uint32_t * flag_w, uint32_t k)
{
  uint32_t n = 0u;
  while (k-- > 0u)
    {
      const uint32_t ones = pmz_ones_down (flag_w[k]);
      n += ones;
      if (ones < 32u)
        break;
    }
  return n;
}

static inline PCG_FN uint32_t
pmz_reach_right (const uint32_t * flag_w, uint32_t k, uint32_t n_words)
{
  uint32_t n = 0u;
  for (k++; k < n_words; k++)
    {
      const uint32_t ones = pmz_ones_up (flag_w[k]);
      n += ones;
      if (ones < 32u)
        break;
    }
  return n;
}

/* The token that begins at bit j of the flag word m: 0 none, 1 a literal, else a match of that length.  left / right: pmz_reach_left /
   pmz_reach_right of the word (used only where the run leaves the word). */
static inline PCG_FN uint32_t
pmz_word_token (uint32_t m, uint32_t j, uint32_t left, uint32_t right)
{
  if (!((m >> j) & 1u))
    return 1u;
  uint32_t l = pmz_ones_down (m << (31u - j));  /* set flags that end at j, j included: at most j + 1, zeros were shifted in */
  if (l == j + 1u)
    l += left;
  uint32_t r = pmz_ones_up (m >> j);    /* set flags from j on: at most 32 - j */
  if (r == 32u - j)
    r += right;
  return pmz_token_at (l - 1u, l + r - 1u);
}

/* a token under the fixed code, as its bits in stream order */
static inline PCG_FN uint32_t
pmz_token_fixed (uint32_t len, uint32_t byte, int *bits)
{
  return pcg_token (len, PMZ_DIST, byte, bits);
}

/* the length symbol of a match of len 3 .. 258, its extra bits and their value (pcg_token's arithmetic) */
static inline PCG_FN uint32_t
pmz_len_sym (uint32_t len, uint32_t *eb, uint32_t *ev)
{
  const uint32_t l = len - 3u;
  *eb = *ev = 0u;
  if (len == PCG_MAX_MATCH)
    return 285u;
  if (l < 8u)
    return 257u + l;
  *eb = (uint32_t) pcg_log2 (l) - 2u;
  *ev = l & ((1u << *eb) - 1u);
  return 257u + 4u * *eb + (l >> *eb);
}

/* a token under a code given as the literal/length symbols' lengths and reversed codes and the distance symbol's: at most 23 bits */
static inline PCG_FN uint32_t
pmz_token_coded (const uint8_t * ll_len, const uint16_t * ll_code, uint32_t d_len, uint32_t d_code, uint32_t len, uint32_t byte, int *bits)
{
  if (len < PCG_MIN_MATCH)
    {
      *bits = ll_len[byte];
      return ll_code[byte];
    }
  uint32_t eb, ev;
  const uint32_t sym = pmz_len_sym (len, &eb, &ev);
  uint32_t v = ll_code[sym], n = ll_len[sym];
  v |= ev << n;
  n += eb;
  v |= d_code << n;
  n += d_len;
  v |= 3u << n;                 /* the two extra bits of distance symbol 7: 16 - 13 */
  n += 2u;
  *bits = (int) n;
  return v;
}

/* a token under preset code c */
static inline PMZ_FN uint32_t
pmz_token_preset (uint32_t c, uint32_t len, uint32_t byte, int *bits)
{
  return pmz_token_coded (pmz_ll_len[c], pmz_ll_code[c], pmz_d_len[c][PMZ_DIST_SYM], pmz_d_code[c][PMZ_DIST_SYM], len, byte, bits);
}

/* bytes of the deflate block of a piece of n bytes in a form, from the sum of its tokens' bits in that form, the form's header bits
   and the bits of its end-of-block code (stored: 5 + n) */
static inline PCG_FN uint32_t
pmz_form_bytes (uint32_t form, uint32_t n, uint32_t token_bits, uint32_t hdr_bits, uint32_t eob_bits)
{
  return form == PMZ_FORM_STORED ? 5u + n : (hdr_bits + token_bits + eob_bits + 7u) >> 3;
}

/* the form that goes out: the smallest of bytes[0 .. PMZ_FORMS), ties to the earlier */
static inline PCG_FN uint32_t
pmz_choose (const uint32_t * bytes)
{
  uint32_t best = 0u;
  for (uint32_t f = 1u; f < PMZ_FORMS; f++)
    if (bytes[f] < bytes[best])
      best = f;
  return best;
}

/* ---- the serial statement (host) */
#ifndef __HIPCC__

/* the tokens of t[0 .. n), n <= PMZ_PIECE, from the runs of the equality flag: tok_pos / tok_len [n at most]; a literal has length 1 */
static inline uint32_t
pmz_parse (const uint8_t * t, uint32_t n, uint16_t * tok_pos, uint16_t * tok_len)
{
  uint32_t k = 0;
  for (uint32_t i = 0; i < n;)
    {
      uint32_t r = 0;
      while (i + r < n && i + r >= PMZ_DIST && t[i + r] == t[i + r - PMZ_DIST])
        r++;
      if (r == 0u)
        {
          tok_pos[k] = (uint16_t) i;
          tok_len[k++] = 1u;
          i++;
          continue;
        }
      for (uint32_t o = 0; o < r; o++)
        {
          const uint32_t len = pmz_token_at (o, r);
          if (len)
            {
              tok_pos[k] = (uint16_t) (i + o);
              tok_len[k++] = (uint16_t) len;
            }
        }
      i += r;
    }
  return k;
}

/* the bytes t[0 .. n), 0 < n <= PMZ_PIECE, as a member at out[0 .. PMZ_MEMBER_MAX) -> the member's length; *form_out (may be NULL): the form */
static inline uint32_t
pmz_encode_bytes (const uint8_t * t, uint32_t n, uint8_t * out, uint32_t * form_out)
{
  uint16_t tp[PMZ_PIECE], tl[PMZ_PIECE];
  uint32_t table[256], bits[PMZ_FORMS], bytes[PMZ_FORMS];
  const uint32_t nt = pmz_parse (t, n, tp, tl);
  int b;
  for (uint32_t f = 0; f < PMZ_FORMS; f++)
    bits[f] = 0u;
  for (uint32_t k = 0; k < nt; k++)
    {
      pmz_token_fixed (tl[k], t[tp[k]], &b);
      bits[PMZ_FORM_FIXED] += (uint32_t) b;
      for (uint32_t c = 0; c < PMZ_CODES; c++)
        {
          pmz_token_preset (c, tl[k], t[tp[k]], &b);
          bits[2u + c] += (uint32_t) b;
        }
    }
  bytes[PMZ_FORM_STORED] = pmz_form_bytes (PMZ_FORM_STORED, n, 0u, 0u, 0u);
  bytes[PMZ_FORM_FIXED] = pmz_form_bytes (PMZ_FORM_FIXED, n, bits[PMZ_FORM_FIXED], 3u, 7u);
  for (uint32_t c = 0; c < PMZ_CODES; c++)
    bytes[2u + c] = pmz_form_bytes (2u + c, n, bits[2u + c], pmz_hdr_bits[c], pmz_ll_len[c][256]);
  const uint32_t form = pmz_choose (bytes);
  const uint32_t m = PMZ_HEAD + bytes[form] + PMZ_TAIL;
  if (form_out)
    *form_out = form;
  for (uint32_t k = 0; k < PMZ_HEAD; k++)
    out[k] = pmz_head_byte (k, m);
  uint32_t at = PMZ_HEAD;
  if (form == PMZ_FORM_STORED)
    {
      out[at++] = 1u;
      out[at++] = (uint8_t) n;
      out[at++] = (uint8_t) (n >> 8);
      out[at++] = (uint8_t) ~n;
      out[at++] = (uint8_t) (~n >> 8);
      for (uint32_t k = 0; k < n; k++)
        out[at++] = t[k];
    }
  else
    {
      uint64_t acc = 3u;        /* final block, fixed codes */
      int have = 3;
      if (form != PMZ_FORM_FIXED)
        {
          const uint32_t c = form - 2u;
          acc = 0u;
          have = 0;
          for (uint32_t k = 0; k < pmz_hdr_bits[c] / 8u; k++)
            out[at++] = pmz_hdr[c][k];
          if (pmz_hdr_bits[c] % 8u)
            {
              acc = pmz_hdr[c][pmz_hdr_bits[c] / 8u];
              have = (int) (pmz_hdr_bits[c] % 8u);
            }
        }
      for (uint32_t k = 0; k <= nt; k++)
        {
          uint32_t v;
          if (form == PMZ_FORM_FIXED)
            v = k < nt ? pmz_token_fixed (tl[k], t[tp[k]], &b) : pcg_sym (256u, &b);
          else
            v = k < nt ? pmz_token_preset (form - 2u, tl[k], t[tp[k]], &b) : pmz_token_preset (form - 2u, 1u, 256u, &b);
          acc |= (uint64_t) v << have;
          have += b;
          for (; have >= 8; have -= 8, acc >>= 8)
            out[at++] = (uint8_t) acc;
        }
      if (have)
        out[at++] = (uint8_t) acc;
    }
  for (uint32_t k = 0; k < 256u; k++)
    table[k] = pcg_crc_table_entry (k);
  const uint32_t crc = pcg_crc_slice (table, t, n);
  for (int k = 0; k < 4; k++)
    out[at++] = (uint8_t) (crc >> (8 * k));
  for (int k = 0; k < 4; k++)
    out[at++] = (uint8_t) (n >> (8 * k));
  return at;
}

/* n records, 0 < n <= PMZ_PIECE_RECORDS, as a member at out[0 .. PMZ_MEMBER_MAX) -> the member's length */
static inline uint32_t
pmz_encode_piece (const void *records, uint32_t n, uint8_t * out)
{
  return pmz_encode_bytes ((const uint8_t *) records, PMZ_RECORD * n, out, (uint32_t *) 0);
}

#endif
#endif
