"""PECALLER_DEVICE_GUIDE=1 of pecaller_amd/csrc/pecaller_main.c on the CPU: the host program linked against the host-only stand-in
with pecall_dev_call_records_guided (tests/csrc/pecall_dev_host_stub_guided.c).  What is checked is the host's half of a guided run,
before any GPU is involved: the ranges of BED lines, the walk of the streams over a range (records in gaps passed over, records
behind the range left pending), the cut at the column where the last stream ends, the positions every sample has seen
(<out>.dist), the columns' heads, the fall-back of lines that go backwards, and that every page-locked range is released again.
Fixtures: the reference's runs of tests/golden/make_golden_pecall_guide.py, _guide_end.py and _guide_many.py."""
import gzip
import os
import re
import struct
import subprocess
import numpy as np
import pytest
import pecall_sites_fixture as fx
import refio
import test_pecaller_host_cpu as h

ROOT = h.ROOT
SWITCH = {"PECALLER_DEVICE_GUIDE": "1"}
LINE = re.compile(r"^ pecaller_hip: device guide merge: (\d+) columns of (\d+) intervals in (\d+) ranges$", re.M)
COLUMNS = re.compile(r"pecaller_hip: (\d+) columns x ")
# fixture -> records, BED, goldens' stem, the last position the streams hold (None: the 40 records far behind the intervals are written)
FIXTURES = {
    "guide": ("pecall_guide.npz", "pecall_guide.bed", "pecall_guide", False),
    "guide_end": ("pecall_guide.npz", "pecall_guide.bed", "pecall_guide_end", True),
    "guide_many": ("pecall_guide_many.npz", "pecall_guide_many.bed", "pecall_guide_many", False),
    "guide_many_back": ("pecall_guide_many.npz", "pecall_guide_many_back.bed", "pecall_guide_many_back", False),
}


def _build(tmp_path_factory, stub):
    out = str(tmp_path_factory.mktemp("host_exe") / "pecaller_host")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Wno-unused-result", "-o", out, os.path.join(h.CSRC, "pecaller_main.c"),
                           os.path.join(ROOT, "tests", "csrc", stub), "-lz", "-lm", "-lpthread"])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "pecall_dev_host_stub_guided.c")


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """a working directory per set of pileup files: all records (and the 40 behind), or the records up to the guide_end fixture's cut"""
    out = {}
    for npz, limit in (("pecall_guide.npz", None), ("pecall_guide.npz", h._guide_end_limit()), ("pecall_guide_many.npz", None)):
        z = np.load(os.path.join(fx.GOLD, npz))
        d = h._workdir(tmp_path_factory, "guided", "pecall_guide.sdx")
        for s, nm in enumerate(str(x) for x in z["names"]):
            if limit is None:
                h._write(d, nm, h._records(z, s) + [struct.pack("<I6H", int(z["tail"][0]) + k, *h.PAD_RECORD) for k in range(40)])
            else:
                h._write(d, nm, h._records(z, s, lambda p: p <= limit))
        out[(npz, limit is not None)] = d
    return out


def read_bed(name):
    return [(x.split("\t")[0], int(x.split("\t")[1]), int(x.split("\t")[2])) for x in open(os.path.join(fx.GOLD, name)).read().split("\n") if x]


def check_guided(out, z, bed, golden, limit):
    """.dist and the rows' keys against the reference's; the rows of <out>.piles.gz (the stand-in makes every A/C/G/T column one): the
    fixture's records at a guided position the first time it is called, zeros where nobody has a record, and zeros at a position
    that a line going backwards calls when the streams are past it"""
    stdout, cols, base, piles, dist = out
    names = [str(x) for x in z["names"]]
    assert sorted(cols) == sorted(names)
    perm = [names.index(c) for c in cols]
    h.check_keys(base, piles, golden + ".base.txt.gz")
    h.check_dist(dist, golden + ".dist.txt")
    lens, cn, _ = refio.read_sdx(os.path.join(fx.GOLD, "pecall_guide.sdx"))
    starts = np.concatenate([[0], np.cumsum(np.array(lens) + 15)])
    rec = {int(p): z["reads"][i][perm].astype(np.int64) for i, p in enumerate(z["pos"]) if limit is None or int(p) <= limit}
    zeros = np.zeros((len(cols), 6), np.int64)
    # rows are written range by range in the BED's order: the global positions in the order they are called
    order, top = [], 0
    for c, lo, hi in bed:
        for p1 in range(lo, max(hi, lo) + 1):
            g = int(starts[cn.index(c)]) + p1 - 1
            order.append((c, p1, g, g < top))
        top = max(top, int(starts[cn.index(c)]) + max(hi, lo))
    past = {}
    for c, p1, g, behind in order:
        past.setdefault((c, p1), []).append(behind)
    n_covered = n_zero = 0
    seen = {}
    for r in piles:
        key = (r[0], int(r[1]))
        k = seen.get(key, 0)
        seen[key] = k + 1
        g = int(starts[cn.index(r[0])]) + int(r[1]) - 1
        exp = zeros if past[key][k] else rec.get(g, zeros)
        n_covered += exp.any()
        n_zero += not exp.any()
        assert np.array_equal(h.counts_of(r, len(cols)), exp), r[:3]
    assert n_covered > 100 and n_zero > 10
    return stdout, len(base)


def expected_ranges(bed, tile):
    """the range rule, restated: consecutive lines that ascend, are disjoint and fit from the range's first position into `tile`
    positions; a longer line is cut there and goes on in the next range; a line that goes backwards or overlaps begins a new one"""
    lens, cn, _ = refio.read_sdx(os.path.join(fx.GOLD, "pecall_guide.sdx"))
    starts = np.concatenate([[0], np.cumsum(np.array(lens) + 15)])
    n, p0, end = 0, None, None
    for c, lo, hi in bed:
        a, b = int(starts[cn.index(c)]) + lo - 1, int(starts[cn.index(c)]) + hi       # [a, b)
        while a < b:
            if p0 is None or a < end or a >= p0 + tile:
                n, p0 = n + 1, a
            end = min(b, p0 + tile)
            a = end
            if end == p0 + tile:
                p0 = None
    return n


CASES = [pytest.param(f, env, threads, id="%s-%s-%s_threads" % (f, "tile10" if env else "default_tile", threads))
         for f in FIXTURES for env, threads in (({}, "2"), ({"PECALLER_TILE_LOG2": "10"}, "2"), ({"PECALLER_TILE_LOG2": "10"}, "8"), ({}, "8"))]


@pytest.mark.parametrize("fixture,env,threads", CASES)
def test_guided_run_on_the_cpu(exe, dirs, fixture, env, threads):
    npz, bed_name, golden, cut = FIXTURES[fixture]
    z = np.load(os.path.join(fx.GOLD, npz))
    bed = read_bed(bed_name)
    limit = h._guide_end_limit() if cut else None
    d = dirs[(npz, cut)]
    on = h.run_host(exe, d, threads, dict(env, **SWITCH), os.path.join(fx.GOLD, bed_name))
    stdout, n_rows = check_guided(on, z, bed, golden, limit)
    m = LINE.search(stdout)
    assert m, stdout[-600:]
    n_cols, n_iv, n_ranges = (int(x) for x in m.groups())
    total = int(COLUMNS.search(stdout).group(1))
    assert 1 <= n_cols <= total and (n_cols == total or n_iv < len(bed))
    tile = 1 << 10 if env else 1 << 20
    if fixture == "guide_many_back":
        # the two lines that go backwards begin ranges of their own (or are left to the per-position path)
        assert n_iv < len(bed) or n_ranges == expected_ranges(bed, tile) >= 3
    elif fixture == "guide_end":
        # the run ends with the column at which the last stream ends, chrMT:300: the ranges up to that line
        assert n_rows == 902 and n_cols == total and n_ranges == expected_ranges(bed[:3], tile)
    else:
        assert n_iv == len(bed) and n_cols == total and n_ranges == expected_ranges(bed, tile)
    if env and fixture.startswith("guide_many"):
        assert n_ranges >= 10                    # (ranges of 1,024 positions: intervals and gaps straddle them)
    # the same files without the switch: the per-position path
    off = h.run_host(exe, d, threads, env, os.path.join(fx.GOLD, bed_name))
    assert "device guide merge" not in off[0]
    assert sorted(map(tuple, off[2])) == sorted(map(tuple, on[2])) and sorted(map(tuple, off[3])) == sorted(map(tuple, on[3])) and off[4] == on[4]


def test_switch_is_ignored_under_the_serial_merge(exe, dirs):
    """PECALLER_SERIAL_MERGE=1: the switch is ignored, the reference's per-position loop takes every line"""
    npz, bed_name, golden, _ = FIXTURES["guide_many_back"]
    z = np.load(os.path.join(fx.GOLD, npz))
    out = h.run_host(exe, dirs[(npz, False)], "2", dict(SWITCH, PECALLER_SERIAL_MERGE="1"), os.path.join(fx.GOLD, bed_name))
    check_guided(out, z, read_bed(bed_name), golden, None)
    assert "device guide merge" not in out[0]


def test_a_library_without_the_entry_refuses_the_switch(tmp_path_factory, dirs):
    """the entry is weak: the program links against the stand-in that lacks it, runs as before, and ends a run that asks for it"""
    old = _build(tmp_path_factory, "pecall_dev_host_stub.c")
    npz, bed_name, golden, _ = FIXTURES["guide_many"]
    bed = os.path.join(fx.GOLD, bed_name)
    d = dirs[(npz, False)]
    out = h.run_host(old, d, "2", {}, bed)
    check_guided(out, np.load(os.path.join(fx.GOLD, npz)), read_bed(bed_name), golden, None)
    e = {k: v for k, v in os.environ.items() if not k.startswith(("PECALLER_", "PEMAP_"))}
    r = subprocess.run([old, "pileup", str(d / "g1.sdx"), "20", "out", "0.95", "0.001", "n", "2", "n", bed], cwd=d / "run", stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=dict(e, **SWITCH))
    assert r.returncode != 0
    assert b"PECALLER_DEVICE_GUIDE=1 needs pecall_dev_call_records_guided" in r.stdout


def test_lines_the_range_builder_leaves_to_the_per_position_path(exe, dirs, tmp_path):
    """a line whose end lies in front of its start (the reference still calls the start position) between lines the device takes: the
    same rows and .dist with and without the switch, and the line is not among the intervals counted"""
    npz = "pecall_guide_many.npz"
    bed = read_bed("pecall_guide_many.bed")
    bed.insert(5, ("chr1", 1300, 1290))
    path = tmp_path / "odd.bed"
    path.write_text("".join("%s\t%d\t%d\n" % b for b in bed))
    d = dirs[(npz, False)]
    on = h.run_host(exe, d, "2", dict(SWITCH, PECALLER_TILE_LOG2="10"), str(path))
    off = h.run_host(exe, d, "2", {"PECALLER_TILE_LOG2": "10"}, str(path))
    assert on[2] == off[2] and on[3] == off[3] and on[4] == off[4]
    # one row for the odd line, its start position; every other row is the many-interval fixture's
    exp = [x.split("\t")[:2] for x in gzip.open(os.path.join(fx.GOLD, "pecall_guide_many.base.txt.gz"), "rt").read().split("\n")[1:] if x]
    assert sorted((r[0], int(r[1])) for r in on[2]) == sorted([(c, int(p)) for c, p in exp] + [("chr1", 1300)])
    m = LINE.search(on[0])
    assert m and int(m.group(2)) == len(bed) - 1
