"""pemap_dev_stage_fastq / pemap_dev_submit_fastq: read rows made on the device from fastq text (pecaller_amd/csrc/pemap_fastq.hip.h)
against the Python model of tests/fastq_cases.py -- every case of the shared list, the edges of the kernels' scans (sized from the
constants pecaller_amd.pemap mirrors), pieces chained by `consumed`, the argument checks -- and, on the g1 fixture index, against the
reference's golden coordinates and against pemap_dev_stage_reads of the same rows."""
import random

import numpy as np
import pytest

import fastq_cases as fc
import fixtures

pytestmark = pytest.mark.gpu

STRIDE = 288


@pytest.fixture(scope="module")
def pdev():
    """an object without an index: staging needs none"""
    from pecaller_amd import PemapDev
    d = PemapDev(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev():
    from pecaller_amd import PemapDev
    d = PemapDev(0)
    ix = fixtures.index()
    d.build_index(ix["genome"], ix["contig_len"])
    yield d
    d.close()


def _check(d, text1, text2, state1=0, state2=0, trim_start=0, trim_end=0, max_records=1000, model=None):
    """stage and read back: the result and the rows are the model's"""
    d.set_params(paired=text2 is not None)
    want = model or fc.parse_pair(text1, text2, state1, state2, trim_start, trim_end, max_records)
    res = d.stage_fastq(text1, text2, state1, state2, trim_start, trim_end, max_records, STRIDE)
    assert res == {k: want[k] for k in ("n", "got", "end", "bad_len", "consumed")}
    if not want["n"]:
        return res
    n, stride, paired = d.staged_info()
    assert (n, stride, paired) == (want["n"], STRIDE, text2 is not None)
    r1, l1, r2, l2 = d.staged_reads()
    for rows, lens, recs in ((r1, l1, want["records"][0]),) + (((r2, l2, want["records"][1]),) if paired else ()):
        assert lens.tolist() == [len(r) for r in recs]
        flat = rows.tobytes()
        for i, r in enumerate(recs):
            assert flat[i * STRIDE:i * STRIDE + len(r)] == r, i
    return res


@pytest.mark.parametrize("case", fc.CASES, ids=[c["name"] for c in fc.CASES])
def test_every_case_of_the_shared_list(pdev, case):
    _check(pdev, case["text1"], case["text2"], case["state1"], case["state2"], case["trim_start"], case["trim_end"], case["max_records"])


# ---- the edges of the scans
def _seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def _rec(rng, i, length):
    s = _seq(rng, length)
    return b"@e%d\n" % i + s + b"\n+\n" + b"I" * length + b"\n"


def _fill_to(rng, size, tail=b""):
    """records, then one junk line, of `size` bytes together with `tail` (which follows them)"""
    out, used, i = [], len(tail), 0
    while size - used > 400:
        r = _rec(rng, i, int(rng.integers(16, 151)))
        out.append(r)
        used += len(r)
        i += 1
    assert size - used >= 1
    out.append(b"j" * (size - used - 1) + b"\n")
    return b"".join(out) + tail


def _edge_texts():
    from pecaller_amd import pemap
    T, LT, TOP = pemap.FASTQ_TILE, pemap.FASTQ_LINE_TILE, pemap.FASTQ_TOP
    rng = np.random.default_rng(7)
    E = {}
    for d in (-1, 0, 1):
        E["tile%+d_bytes" % d] = _fill_to(rng, T + d)
        E["two_tiles%+d_bytes" % d] = _fill_to(rng, 2 * T + d)
    E["tile_minus_1_no_final_newline"] = _fill_to(rng, T)[:-1]
    # '\n' as the last byte of a tile and as the first byte of the next (an empty line), then records
    E["newline_on_both_sides_of_a_tile_edge"] = _fill_to(rng, T) + b"\n" + _rec(rng, 900, 100) + _rec(rng, 901, 100)
    # a sequence line that straddles the edge: the record's header ends 50 bytes in front of it
    E["sequence_straddles_a_tile_edge"] = _fill_to(rng, T - 50 - 6, b"@e800\n") + _seq(rng, 120) + b"\n+\n" + b"I" * 120 + b"\n" + _rec(rng, 801, 60)
    E["header_newline_is_the_tile's_last_byte"] = _fill_to(rng, T, b"@e800\n") + _seq(rng, 120) + b"\n+\n" + b"I" * 120 + b"\n"
    # a lane whose 16 bytes are all '\n'
    E["a_lane_of_newlines"] = _fill_to(rng, 1600) + b"\n" * 48 + _rec(rng, 700, 80) + b"\n" * 16 + _rec(rng, 701, 80)
    # one tile more than the top-level block takes at a time, and a '\n' count per tile that varies
    E["top_plus_one_tiles"] = _fill_to(rng, TOP * T + 1000)
    assert (len(E["top_plus_one_tiles"]) + T - 1) // T == TOP + 1
    # line counts around the role scan's tile, with records on both sides of its edge (four lines a record)
    for d in (-1, 0, 1, 2, 5):
        E["line_tile%+d_lines" % d] = b"".join(_rec(rng, i, 40) for i in range(LT // 4 - 1)) + b"x\n" * (4 + d) + b"".join(_rec(rng, i, 41) for i in range(5))
    # more line tiles than the top-level block takes at a time: mostly empty lines, records in front, between and behind
    E["top_plus_one_line_tiles"] = (b"".join(_rec(rng, i, 50) for i in range(300)) + b"\n" * (TOP * LT // 2) + b"".join(_rec(rng, i, 51) for i in range(300))
                                    + b"\n" * (TOP * LT // 2) + b"".join(_rec(rng, i, 52) for i in range(300)))
    return E


EDGES = None


def _edges():
    global EDGES
    if EDGES is None:
        EDGES = _edge_texts()
    return EDGES


EDGE_NAMES = ["tile-1_bytes", "tile+0_bytes", "tile+1_bytes", "two_tiles-1_bytes", "two_tiles+0_bytes", "two_tiles+1_bytes", "tile_minus_1_no_final_newline",
              "newline_on_both_sides_of_a_tile_edge", "sequence_straddles_a_tile_edge", "header_newline_is_the_tile's_last_byte", "a_lane_of_newlines",
              "top_plus_one_tiles", "line_tile-1_lines", "line_tile+0_lines", "line_tile+1_lines", "line_tile+2_lines", "line_tile+5_lines",
              "top_plus_one_line_tiles"]


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edges_of_the_scans(pdev, name):
    E = _edges()
    assert sorted(E) == sorted(EDGE_NAMES)
    text = E[name]
    other = E["two_tiles+1_bytes"]
    res = _check(pdev, text, other, max_records=1 << 20)
    assert res["got"][0] > 0
    # the same text as the second mate, in state 1 behind a sequence line, and alone
    _check(pdev, other, b"+\nII\n" + text, state2=1, max_records=1 << 20)
    _check(pdev, text, None, max_records=1 << 20)


def test_record_limit_inside_and_at_the_edge_of_a_line_tile(pdev):
    """max_records in the middle of a tile of lines, at its last record and at the first of the next"""
    from pecaller_amd import pemap
    per = pemap.FASTQ_LINE_TILE // 4
    rng = np.random.default_rng(9)
    text = b"".join(_rec(rng, i, 30 + i % 50) for i in range(3 * per))
    for mr in (per - 1, per, per + 1, 2 * per, 2 * per + 1, 3 * per, 3 * per + 1):
        res = _check(pdev, text, text, max_records=mr)
        assert res["n"] == min(mr, 3 * per) and res["end"][0] == (0 if mr <= 3 * per else 1)
    # a stopping record as the last record of a tile, as the first of the next, and the lower of two that stop
    lines = text.split(b"\n")
    for k in (per - 1, per, 2 * per):
        bad = lines[:]
        bad[4 * k + 1] = b"ACGT"
        bad[4 * (2 * per + 7) + 1] = b"A" * 300
        res = _check(pdev, b"\n".join(bad), text, max_records=1 << 20)
        assert res["got"][0] == k and res["end"][0] == 2


# ---- pieces chained by `consumed`
def _chain(d, texts, piece, max_records, trims=(0, 0)):
    """feed the texts in pieces of `piece` bytes, carrying tail and state as a caller does -> per mate the records"""
    mates = len(texts)
    d.set_params(paired=mates == 2)
    pos, tail, state, out = [0] * mates, [b""] * mates, [0] * mates, [[] for _ in texts]
    for _ in range(100000):
        buf = []
        for m in range(mates):
            buf.append(tail[m] + texts[m][pos[m]:pos[m] + piece])
            pos[m] = min(pos[m] + piece, len(texts[m]))
        res = d.stage_fastq(buf[0], buf[1] if mates == 2 else None, state[0], state[1] if mates == 2 else 0, trims[0], trims[1], max_records, STRIDE)
        if res["n"]:
            r1, l1, r2, l2 = d.staged_reads()
            for m, (rows, lens) in enumerate(((r1, l1), (r2, l2))[:mates]):
                flat = rows.tobytes()
                out[m] += [flat[i * STRIDE:i * STRIDE + int(lens[i])] for i in range(res["n"])]
                tail[m] = buf[m][res["consumed"][m]:]
                state[m] = 1
        else:
            tail = buf
        if any(e in (2, 3) for e in res["end"][:mates]) and res["n"] < max_records:
            break
        if all(pos[m] == len(texts[m]) for m in range(mates)) and res["n"] < max_records:
            break
    return out


@pytest.mark.parametrize("piece", [4099, 7777, 65537])
def test_pieces_chained_by_consumed_give_the_one_shot_records(pdev, piece):
    t1 = fc.quirky(3000, random.Random(11))
    t2 = fc.quirky(2900, random.Random(12))
    one = fc.parse_pair(t1, None)
    assert one["n"] == 3000
    assert _chain(pdev, [t1], piece, 700)[0] == one["records"][0]
    two = fc.parse_pair(t1, t2)
    assert two["n"] == 2900 and two["got"] == [3000, 2900]
    got = _chain(pdev, [t1, t2], piece, 512)
    assert got[0] == two["records"][0] and got[1] == two["records"][1]


def test_chained_pieces_with_trims_and_crlf(pdev):
    t1 = fc.quirky(500, random.Random(13), 60, 150).replace(b"\n", b"\r\n")
    t2 = fc.quirky(500, random.Random(14), 60, 150)
    want = fc.parse_pair(t1, t2, trim_start=3, trim_end=2)
    assert want["n"] == 500
    got = _chain(pdev, [t1, t2], 1001, 64, trims=(3, 2))
    assert got[0] == want["records"][0] and got[1] == want["records"][1]


# ---- argument checks: values refused on the host, before any kernel
def test_bad_arguments_are_refused_with_a_message(pdev):
    from pecaller_amd import PemapError
    good = fc.plain(3)
    pdev.set_params(paired=True)
    bad = [dict(stride=15), dict(stride=277), dict(max_records=0), dict(max_records=-1), dict(state1=2), dict(state2=-1), dict(trim_start=-1),
           dict(trim_end=-1)]
    for kw in bad:
        args = dict(text1=good, text2=good, state1=0, state2=0, trim_start=0, trim_end=0, max_records=10, stride=STRIDE)
        args.update(kw)
        with pytest.raises(PemapError) as e:
            pdev.stage_fastq(**args)
        assert "stage_fastq" in str(e.value), kw
    with pytest.raises(PemapError) as e:
        pdev.stage_fastq(good, None)
    assert "second text" in str(e.value)
    # a length beyond 2^30 is refused by its value: the text itself is never touched
    import ctypes as C
    from pecaller_amd import pemap
    res = pemap.FastqResult()
    rc = pdev.L.pemap_dev_stage_fastq(pdev.h, good, pemap.FASTQ_MAX_TEXT + 1, 0, good, len(good), 0, 0, 0, 10, STRIDE, C.byref(res))
    assert rc != 0 and b"bytes" in pdev.L.pemap_dev_last_error(pdev.h)
    rc = pdev.L.pemap_dev_stage_fastq(pdev.h, None, 0, 0, good, len(good), 0, 0, 0, 10, STRIDE, C.byref(res))
    assert rc != 0 and b"NULL" in pdev.L.pemap_dev_last_error(pdev.h)
    rc = pdev.L.pemap_dev_stage_fastq(pdev.h, good, len(good), 0, good, len(good), 0, 0, 0, 10, STRIDE, None)
    assert rc != 0
    # submit_fastq needs an index, and the object still works
    with pytest.raises(PemapError):
        pdev.submit_fastq(good, good)
    _check(pdev, good, good)


# ---- on the g1 fixture index
def _text_of(rows, lens, first=0):
    flat = rows.tobytes()
    stride = rows.shape[1]
    return b"".join(b"@g%d\n%s\n+\n%s\n" % (first + i, flat[i * stride:i * stride + int(n)], b"I" * int(n)) for i, n in enumerate(lens))


def test_r150_staged_as_text_maps_like_the_rows(dev):
    r1, l1, r2, l2 = fixtures.reads("r150")
    dev.set_lookup_replicas(8)
    dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
    dev.stage_reads(r1, l1, r2, l2)
    dev.run()
    a1, a2, at = dev.collect()
    res = dev.stage_fastq(_text_of(r1, l1), _text_of(r2, l2), max_records=1 << 20, stride=r1.shape[1])
    assert res["n"] == len(l1) and res["end"] == [1, 1]
    s1, sl1, s2, sl2 = dev.staged_reads()
    assert np.array_equal(sl1, l1) and np.array_equal(sl2, l2)
    dev.run()
    m1, m2, mt = dev.collect()
    assert np.array_equal(m1, fixtures.golden_m("r150", 1)) and np.array_equal(m2, fixtures.golden_m("r150", 2))
    assert np.array_equal(m1, a1) and np.array_equal(m2, a2) and np.array_equal(mt, at)


def test_r150_submitted_as_text_in_pieces_three_batches_in_flight(dev):
    r1, l1, r2, l2 = fixtures.reads("r150")
    dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
    dev.stage_reads(r1, l1, r2, l2)
    dev.run()
    _, _, at = dev.collect()
    dev.reset_pileup()
    texts = [_text_of(r1, l1), _text_of(r2, l2)]
    piece, max_records = 777777, 3000
    pos, tail, state, tickets = [0, 0], [b"", b""], [0, 0], []
    for _ in range(1000):
        buf = []
        for m in range(2):
            buf.append(tail[m] + texts[m][pos[m]:pos[m] + piece])
            pos[m] = min(pos[m] + piece, len(texts[m]))
        res, t = dev.submit_fastq(buf[0], buf[1], state[0], state[1], 0, 0, max_records, r1.shape[1])
        if res["n"]:
            tickets.append((res["n"], t))
            tail = [buf[m][res["consumed"][m]:] for m in range(2)]
            state = [1, 1]
        else:
            assert t is None
            tail = buf
        if pos[0] == len(texts[0]) and pos[1] == len(texts[1]) and res["n"] < max_records:
            break
    assert len(tickets) >= 7 and any(n < max_records for n, _ in tickets[:-1])       # (pieces that held fewer records than a batch takes)
    out = [dev.wait_batch(t) for _, t in tickets]
    m1, m2, mt = (np.concatenate([o[k] for o in out]) for k in range(3))
    assert np.array_equal(m1, fixtures.golden_m("r150", 1)) and np.array_equal(m2, fixtures.golden_m("r150", 2))
    assert np.array_equal(mt, at)
    counts, _ = dev.fetch_pileup()
    fixtures.check_pileup_against_golden("r150", counts)


def test_r100_single_end_as_text(dev):
    r1, l1, _, _ = fixtures.reads("r100")
    dev.set_params(paired=False, min_dist=0, max_dist=500, min_align=0.85)
    try:
        res = dev.stage_fastq(_text_of(r1, l1), None, max_records=1 << 20, stride=r1.shape[1])
        assert res["n"] == len(l1) and res["got"] == [len(l1), 0]
        dev.run()
        m1, _, mt = dev.collect()
        assert np.array_equal(m1, fixtures.golden_m("r100", 1))
        res, t = dev.submit_fastq(_text_of(r1, l1), None, max_records=1 << 20, stride=r1.shape[1])
        x1, _, xt = dev.wait_batch(t)
        assert np.array_equal(x1, m1) and np.array_equal(xt, mt)
    finally:
        dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
