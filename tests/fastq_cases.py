"""A pure-Python model of the rule by which pemapper_hip takes reads out of fastq text (fill_rows and map_one_file of
pecaller_amd/csrc/pemapper_main.c; pecaller_amd/csrc/pemap_fastq_rule.h states it for the host and the kernels), and the list of
cases that the CPU suite (test_fastq_rule_cpu.py) and the GPU suite (test_gpu_fastq_parse.py) both run.

A line is a run of bytes ended by b"\\n" (a b"\\r" is part of it); bytes behind the last b"\\n" are no line.  The walk over the lines:
START skipped -> SEQ; SEQ a record's sequence -> SKIP1; SKIP1 skipped -> SKIP2; SKIP2 skipped -> SEEK; SEEK skipped, -> SEQ if the
line begins with b"@" else SEEK.  state 0 begins in START, state 1 in SKIP1."""
import random

MIN_READ = 16
MAX_READ = 278
START, SEQ, SKIP1, SKIP2, SEEK = range(5)


def lines_of(text):
    """[(start, full)] of the complete lines"""
    out, pos = [], 0
    while True:
        e = text.find(b"\n", pos)
        if e < 0:
            return out
        out.append((pos, e - pos))
        pos = e + 1


def parse_mate(text, state=0, trim_start=0, trim_end=0, first_mate=True, max_records=1 << 20):
    """-> dict(records=[bytes], nexts=[offset behind the record's line], got, end, bad_len)"""
    st = SKIP1 if state else START
    records, nexts, k, end, bad_len = [], [], 0, None, 0
    for start, full in lines_of(text):
        if st == SEQ:
            if k < max_records and end is None:
                sl = full - trim_start
                off = start + (trim_start if sl >= 0 else full)
                sl = max(sl - trim_end, 0)
                if first_mate and sl <= 12:
                    end = 2
                elif sl < MIN_READ or sl > MAX_READ:
                    end, bad_len = 3, sl
                else:
                    records.append(text[off:off + sl])
                    nexts.append(start + full + 1)
            k += 1
            st = SKIP1
        elif st == START:
            st = SEQ
        elif st == SKIP1:
            st = SKIP2
        elif st == SKIP2:
            st = SEEK
        else:
            st = SEQ if text[start:start + 1] == b"@" else SEEK
    got = len(records)
    if end is None:
        end = 0 if got == max_records else 1
    return dict(records=records, nexts=nexts, got=got, end=end, bad_len=bad_len)


def parse_pair(text1, text2=None, state1=0, state2=0, trim_start=0, trim_end=0, max_records=1 << 20):
    """-> dict(n, got, end, bad_len, consumed, records=[per mate the first n])  (text2 None: single-end)"""
    ms = [parse_mate(text1, state1, trim_start, trim_end, True, max_records)]
    if text2 is not None:
        ms.append(parse_mate(text2, state2, trim_start, trim_end, False, max_records))
    n = min(m["got"] for m in ms)
    pad = [0] * (2 - len(ms))
    return dict(n=n, got=[m["got"] for m in ms] + pad, end=[m["end"] for m in ms] + pad, bad_len=[m["bad_len"] for m in ms] + pad,
                consumed=[m["nexts"][n - 1] if n else 0 for m in ms] + pad, records=[m["records"][:n] for m in ms])


# ---- the cases
_rng = random.Random(20240611)


def seq(n):
    return bytes(_rng.choice(b"ACGT") for _ in range(n))


def rec(name, s, qual=None, plus=b"+", nl=b"\n"):
    q = b"I" * len(s) if qual is None else qual
    return b"@" + name + nl + s + nl + plus + nl + q + nl


def plain(n, length=50, tag=b"r"):
    return b"".join(rec(tag + str(i).encode(), seq(length)) for i in range(n))


def with_lengths(lengths, **kw):
    return b"".join(rec(b"r%d" % i, seq(L), **kw) for i, L in enumerate(lengths))


def quirky(n, rng, lo=30, hi=150):
    """n records with what real files and broken files hold between them"""
    out = []
    for i in range(n):
        s = seq(rng.randint(lo, hi))
        q = rng.random()
        qual = (b"@" + b"J" * (len(s) - 1)) if q < 0.3 else None
        out.append(rec(b"q%d" % i, s, qual=qual, plus=b"+x" if rng.random() < 0.2 else b"+"))
        r = rng.random()
        if r < 0.1:
            out.append(b"junk line\n")
        elif r < 0.15:
            out.append(b"\n" * rng.randint(1, 20))
        elif r < 0.2:
            out.append(b"+x\nmore junk\n\n")
    return b"".join(out)


def _cases():
    C = []

    def add(name, text1, text2="same", **kw):
        if isinstance(text2, str):
            text2 = plain(len(parse_mate(text1, kw.get("state1", 0), first_mate=False)["records"]) or 3, 60, b"m") if text2 == "same" else None
        C.append(dict(name=name, text1=text1, text2=text2, state1=kw.pop("state1", 0), state2=kw.pop("state2", 0), trim_start=kw.pop("trim_start", 0),
                      trim_end=kw.pop("trim_end", 0), max_records=kw.pop("max_records", 1000)))
        assert not kw, kw

    add("wellformed", plain(5, 100), plain(5, 100))
    add("wellformed_single", plain(5, 100), "none")
    add("qual_begins_with_at", with_lengths([40, 41, 42, 43], qual=b"@" * 40))
    add("qual_at_both", with_lengths([40, 41, 42], qual=b"@@@@"), with_lengths([50, 51, 52], qual=b"@"))
    add("junk_and_plus_x", rec(b"a", seq(30)) + b"junk\n+x\n" + rec(b"b", seq(31), plus=b"+x") + b"more\njunk\n+x\n" + rec(b"c", seq(32)))
    long_at = b"@" + seq(40)
    add("two_at_lines_long", rec(b"a", seq(30)) + b"@x\n" + long_at + b"\n+\nIIII\n" + rec(b"b", seq(33)))
    add("three_at_lines_long", rec(b"a", seq(30)) + b"@x\n" + long_at + b"\n" + long_at + b"\nII\n" + rec(b"b", seq(33)))
    add("two_at_lines_short_first_mate", rec(b"a", seq(30)) + b"@x\n@y\n" + seq(30) + b"\n+\nII\n")
    add("two_at_lines_short_second_mate", plain(3), rec(b"a", seq(30)) + b"@x\n@y\n" + seq(30) + b"\n+\nII\n")
    add("three_at_lines_short", rec(b"a", seq(30)) + b"@x\n@y\n@z\n" + seq(30) + b"\n+\nII\n", "none")
    add("empty_lines", rec(b"a", seq(30)) + b"\n\n" + rec(b"b", seq(30)) + b"\n" * 20 + rec(b"c", seq(30)) + b"\n")
    add("empty_lines_first", b"\n" * 20 + plain(3))
    add("only_newlines", b"\n" * 20)
    add("only_newlines_state1", b"\n" * 37, b"\n" * 3, state1=1, state2=1)
    add("crlf", with_lengths([30, 31, 32], nl=b"\r\n"), with_lengths([40, 41, 42], nl=b"\r\n"))
    add("crlf_277_278", with_lengths([277], nl=b"\r\n"), with_lengths([100, 100], nl=b"\r\n"))
    add("no_newline_at_all", b"@r0" + seq(40))
    add("empty_text", b"", b"")
    add("ends_without_newline_in_quality", plain(3)[:-1], plain(3))
    add("ends_without_newline_in_sequence", plain(2) + b"@r2\n" + seq(50), plain(3))
    add("long_header_and_quality", rec(b"h" * 9999, seq(100)) + rec(b"b", seq(100), qual=b"I" * 10000) + rec(b"c", seq(100)),
        rec(b"a", seq(100), qual=b"@" * 10000) + rec(b"h" * 9999, seq(100)) + rec(b"c", seq(100)))
    add("long_sequence_line", rec(b"a", seq(50)) + rec(b"b", seq(10000)) + rec(b"c", seq(50)))
    add("state0_single_line", b"@r0\n")
    add("state0_two_lines", b"@r0\n" + seq(50) + b"\n", b"@r0\n" + seq(50) + b"\n")
    add("state1", b"+\nIIII\n" + plain(3), b"+\nIIII\njunk\n" + plain(3), state1=1, state2=1)
    add("state1_seek_at", b"+\n@III\n" + plain(2), "none", state1=1)
    add("state1_and_state0", b"+\nIIII\n" + plain(3), plain(3), state1=1, state2=0)
    add("trim_3_2", plain(4, 100), plain(4, 100), trim_start=3, trim_end=2)
    add("trim_3_2_edge_lengths", with_lengths([21, 283, 20]), with_lengths([283, 21, 21]), trim_start=3, trim_end=2)
    add("trim_3_2_too_long", with_lengths([100, 284]), trim_start=3, trim_end=2)
    add("trim_start_beyond_line_first", with_lengths([100, 10, 100]), trim_start=30)
    add("trim_start_beyond_line_second", plain(3, 100), with_lengths([100, 10, 100]), trim_start=30)
    add("trims_eat_the_line", plain(3, 100), with_lengths([100, 40, 100]), trim_start=20, trim_end=20)
    add("trims_eat_more_than_the_line", plain(3, 100), with_lengths([100, 35, 100]), trim_start=20, trim_end=20)
    for L in (12, 13, 15, 16, 278, 279):
        add("length_%d_first" % L, with_lengths([50, 60, L, 70]), plain(4))
        add("length_%d_second" % L, plain(4), with_lengths([50, 60, L, 70]))
    add("length_12_single", with_lengths([50, 12, 50]), "none")
    add("length_13_single", with_lengths([50, 13, 50]), "none")
    add("empty_sequence_line", with_lengths([50, 0, 50]))
    # the stopping record against max_records
    add("stop_at_0", with_lengths([5, 50, 50]))
    add("stop_at_0_second", plain(3), with_lengths([300, 50, 50]))
    add("stop_at_max_minus_1", with_lengths([50, 50, 300, 50]), plain(4), max_records=3)
    add("stop_at_max", with_lengths([50, 50, 50, 300]), plain(4), max_records=3)
    add("stop_behind_max", with_lengths([50, 50, 50, 50, 5]), plain(5), max_records=3)
    for d in (-1, 0, 1):
        add("max_records_count%+d" % d, plain(6), plain(6), max_records=6 + d)
        add("max_records_count%+d_single" % d, plain(6), "none", max_records=6 + d)
    add("max_records_1", plain(6), plain(6), max_records=1)
    add("mates_differ_first_longer", plain(7), plain(4))
    add("mates_differ_second_longer", plain(2), plain(9))
    add("mates_differ_second_empty", plain(2), b"@only a header\n")
    add("both_stop_at_2_short_and_long", with_lengths([50, 50, 5, 50]), with_lengths([50, 50, 300, 50]))
    add("both_stop_at_2_bad_lengths", with_lengths([50, 50, 14, 50]), with_lengths([50, 50, 300, 50]))
    add("second_stops_before_first", with_lengths([50, 50, 5, 50]), with_lengths([50, 300, 50, 50]))
    add("quirky_60", quirky(60, random.Random(1)), quirky(55, random.Random(2)))
    return C


CASES = _cases()
assert len({c["name"] for c in CASES}) == len(CASES)


def model_of(case):
    return parse_pair(case["text1"], case["text2"], case["state1"], case["state2"], case["trim_start"], case["trim_end"], case["max_records"])
