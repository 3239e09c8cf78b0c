"""The whole host program pecaller_amd/csrc/pecaller_main.c on the CPU, linked against a host-only stand-in for the library
(tests/csrc/pecall_dev_host_stub.c: every A/C/G/T column is "called" as its reference letter with type 1, so every such column is
written to <out>.piles.gz too).  What is checked is the host's own half of the run: the walk of the pileup streams (ranges, the
serial merge, guide stretches and guide positions, the records path of the device merge), <out>.dist, the tile pipeline, the row
text's keys, the repeat with the serial merge, and that every page-locked range is released again.  Same pileup files, made from the
same committed fixtures, as tests/test_gpu_pecaller_cli*.py."""
import gzip
import importlib.util
import json
import os
import shutil
import struct
import subprocess
import numpy as np
import pytest
import pecall_sites_fixture as fx
import refio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pecaller_amd", "csrc")
PAD_RECORD = [20, 0, 0, 0, 0, 0]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("host_exe") / "pecaller_host")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-Wno-unused-result", "-o", out, os.path.join(CSRC, "pecaller_main.c"),
                           os.path.join(ROOT, "tests", "csrc", "pecall_dev_host_stub.c"), "-lz", "-lm", "-lpthread"])
    return out


def _workdir(tmp_path_factory, tag, sdx):
    d = tmp_path_factory.mktemp(tag)
    _, seqs = refio.read_fasta(os.path.join(fx.GOLD, "g1.fa.gz"))
    shutil.copy(os.path.join(fx.GOLD, sdx), d / "g1.sdx")
    with gzip.open(d / "g1.seq", "wb", compresslevel=1) as f:
        f.write(np.concatenate(seqs).tobytes())
    (d / "run").mkdir()
    return d


def _write(d, name, recs):
    with gzip.open(d / "run" / ("%s.pileup.gz" % name), "wb", compresslevel=1) as f:
        f.write(b"".join(recs))


def _records(z, s, keep=lambda p: True):
    reads, pos = z["reads"], z["pos"]
    return [struct.pack("<I6H", int(pos[i]), *[int(x) for x in reads[i, s]]) for i in range(len(pos)) if reads[i, s].sum() > 0 and keep(int(pos[i]))]


@pytest.fixture(scope="module")
def sites_dir(tmp_path_factory):
    z = np.load(os.path.join(fx.GOLD, "pecall_sites.npz"))
    d = _workdir(tmp_path_factory, "sites", "g1.sdx")
    for s, nm in enumerate(str(x) for x in z["names"]):
        _write(d, nm, _records(z, s) + [struct.pack("<I6H", int(z["pos"][-1]) + 1 + k, *PAD_RECORD) for k in range(int(z["pad"][0]))])
    return d


@pytest.fixture(scope="module")
def unordered_dir(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("mk_unordered", os.path.join(fx.GOLD, "make_golden_pecall_unordered.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    z = np.load(os.path.join(fx.GOLD, "pecall_sites.npz"))
    dist_spec = json.load(open(os.path.join(fx.GOLD, "pecall_unordered.json")))
    d = _workdir(tmp_path_factory, "unordered", "g1.sdx")
    for s, nm in enumerate(str(x) for x in z["names"]):
        _write(d, nm, mk.stream_records(z, s, dist_spec))
    return d


@pytest.fixture(scope="module")
def guide_dir(tmp_path_factory):
    z = np.load(os.path.join(fx.GOLD, "pecall_guide.npz"))
    d = _workdir(tmp_path_factory, "guide", "pecall_guide.sdx")
    for s, nm in enumerate(str(x) for x in z["names"]):
        _write(d, nm, _records(z, s) + [struct.pack("<I6H", int(z["tail"][0]) + k, *PAD_RECORD) for k in range(40)])
    return d


def _guide_end_limit():
    cut = json.load(open(os.path.join(fx.GOLD, "pecall_guide_end.json")))["cut"]
    lens, cn, _ = refio.read_sdx(os.path.join(fx.GOLD, "pecall_guide.sdx"))
    starts = np.concatenate([[0], np.cumsum(np.array(lens) + 15)])
    return int(starts[cn.index("chrMT")]) + cut - 1


@pytest.fixture(scope="module")
def guide_end_dir(tmp_path_factory):
    z = np.load(os.path.join(fx.GOLD, "pecall_guide.npz"))
    limit = _guide_end_limit()
    d = _workdir(tmp_path_factory, "guide_end", "pecall_guide.sdx")
    for s, nm in enumerate(str(x) for x in z["names"]):
        _write(d, nm, _records(z, s, lambda p: p <= limit))
    return d


def run_host(exe, d, threads="8", env=None, guide=None):
    """-> (stdout, header names, base rows, piles rows, dist lines); the stand-in's complaint about page-locked ranges fails the run"""
    run = d / "run"
    for f in ("out.base.gz", "out.snp", "out.piles.gz", "out.dist"):
        if os.path.exists(run / f):
            os.remove(run / f)
    e = {k: v for k, v in os.environ.items() if not k.startswith(("PECALLER_", "PEMAP_"))}
    e.update(env or {})
    r = subprocess.run([exe, "pileup", str(d / "g1.sdx"), "20", "out", "0.95", "0.001", "n", threads, "n"] + ([guide] if guide else []),
                       cwd=run, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    assert b"pecall_dev_host_stub" not in r.stderr, r.stderr
    base = gzip.open(run / "out.base.gz", "rt").read().split("\n")
    piles = gzip.open(run / "out.piles.gz", "rt").read().split("\n")
    cols = [c for c in base[0].split("\t")[3:] if c]
    assert [c for c in piles[0].split("\t")[3:] if c] == cols
    split = lambda rows: [x.split("\t") for x in rows if x]
    return r.stdout.decode(), cols, split(base[1:]), split(piles[1:]), open(run / "out.dist").read().split("\n")


def check_dist(dist, golden):
    """field for field, columns matched by sample name"""
    got = [x.split("\t") for x in dist]
    exp = [x.split("\t") for x in open(os.path.join(fx.GOLD, golden)).read().split("\n")]
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g[0] == e[0] and len(g) == len(e)
        if len(g) > 1:
            assert dict(zip(got[0][1:], g[1:])) == dict(zip(exp[0][1:], e[1:])), g[0]


def check_keys(base, piles, golden, upto=None):
    """contig, position and reference letter of every row of <out>.base.gz (up to position `upto`: the padding columns behind it are
    not in the golden text) are the reference's; <out>.piles.gz has the rows of <out>.base.gz -> the number of rows written"""
    exp = [x.split("\t")[:3] for x in gzip.open(os.path.join(fx.GOLD, golden), "rt").read().split("\n")[1:] if x]
    key = lambda rows: sorted((r[0], int(r[1]), r[2]) for r in rows)
    assert key(r for r in base if upto is None or int(r[1]) <= upto) == key(exp)
    assert key(piles) == key(base)
    return len(base)


def counts_of(row, n):
    return np.array([int(v) for v in row[3:]], np.int64).reshape(n, 6)


def check_sites(out, z, unordered_spec=None):
    stdout, cols, base, piles, dist = out
    names = [str(x) for x in z["names"]]
    assert sorted(cols) == sorted(names)
    perm = [names.index(c) for c in cols]
    reads, pos = z["reads"][:, perm, :].astype(np.int64), z["pos"]
    last = int(pos[-1]) + 1
    n_exp = check_keys(base, piles, "pecall_unordered.base.txt.gz" if unordered_spec else "pecall_sites.base.txt.gz", last)
    check_dist(dist, "pecall_unordered.dist.txt" if unordered_spec else "pecall_sites.dist.txt")
    col_of = {int(q) + 1: i for i, q in enumerate(pos)}
    exp = {}
    for p1, i in col_of.items():
        exp[p1] = reads[i].copy()
    if unordered_spec:
        # a position that a stream holds twice is two columns (the second record's counts are the first's halved), a record behind
        # its successor a column of its own: the rows of one position add up to the fixture's column
        s, i = unordered_spec["twice"]
        exp[int(pos[i]) + 1][cols.index(names[s])] += reads[i][cols.index(names[s])] // 2
    got = {}
    for r in piles:
        p1 = int(r[1])
        if p1 > last:
            assert p1 <= last + int(z["pad"][0]) and np.array_equal(counts_of(r, len(cols)), np.array([PAD_RECORD] * len(cols)))
            continue
        c = counts_of(r, len(cols))
        if unordered_spec:
            got[p1] = got.get(p1, 0) + c
        else:
            assert p1 not in got
            got[p1] = c
    assert len(got) > 5000
    for p1, c in got.items():
        assert np.array_equal(c, exp[p1]), p1
    return n_exp, stdout


@pytest.mark.parametrize("env,threads", [({}, "8"), ({"PECALLER_TILE_LOG2": "10"}, "2"), ({"PECALLER_TILE_LOG2": "10"}, "8"),
                                         ({"PECALLER_SERIAL_MERGE": "1"}, "8"), ({"PECALLER_DEVICE_MERGE": "1", "PECALLER_TILE_LOG2": "10"}, "8")],
                         ids=["default_tile", "tile10_2threads", "tile10_8threads", "serial_merge", "device_merge_tile10"])
def test_host_program_on_the_sites_fixture(exe, sites_dir, env, threads):
    z = np.load(os.path.join(fx.GOLD, "pecall_sites.npz"))
    n_rows, stdout = check_sites(run_host(exe, sites_dir, threads, env), z)
    assert n_rows == 5947                        # (5,907 of the fixture's columns and its 40 padding columns)
    assert "starting over with the serial merge" not in stdout
    if "PECALLER_DEVICE_MERGE" in env:
        assert " pecaller_hip: device merge: 5947 columns in 6 ranges\n" in stdout
    else:
        assert "device merge:" not in stdout


@pytest.mark.parametrize("env,starts_over", [({}, True), ({"PECALLER_SERIAL_MERGE": "1"}, False), ({"PECALLER_DEVICE_MERGE": "1"}, True)],
                         ids=["host_walk", "serial_from_start", "device_merge"])
def test_host_program_on_streams_that_are_not_ascending(exe, unordered_dir, env, starts_over):
    """(the repeat with the serial merge runs teardown, a second pass and teardown again in one process)"""
    z = np.load(os.path.join(fx.GOLD, "pecall_sites.npz"))
    spec = json.load(open(os.path.join(fx.GOLD, "pecall_unordered.json")))
    n_rows, stdout = check_sites(run_host(exe, unordered_dir, "8", dict(env, PECALLER_TILE_LOG2="10")), z, spec)
    assert n_rows == 5950                        # (three positions twice)
    assert ("starting over with the serial merge" in stdout) == starts_over
    assert stdout.count("Found a total of %d individuals" % len(z["names"])) == (2 if starts_over else 1)
    assert "device merge:" not in stdout


def check_guide(out, z, golden, limit=None):
    stdout, cols, base, piles, dist = out
    names = [str(x) for x in z["names"]]
    assert sorted(cols) == sorted(names)
    perm = [names.index(c) for c in cols]
    n_exp = check_keys(base, piles, golden + ".base.txt.gz")
    check_dist(dist, golden + ".dist.txt")
    lens, cn, _ = refio.read_sdx(os.path.join(fx.GOLD, "pecall_guide.sdx"))
    starts = np.concatenate([[0], np.cumsum(np.array(lens) + 15)])
    rec = {int(p): z["reads"][i][perm].astype(np.int64) for i, p in enumerate(z["pos"]) if limit is None or int(p) <= limit}
    if limit is None:
        for k in range(40):
            rec[int(z["tail"][0]) + k] = np.array([PAD_RECORD] * len(cols))
    zeros = np.zeros((len(cols), 6), np.int64)
    n_covered = 0
    for r in piles:                              # every position of the intervals is a row: the fixture's counts, or zeros
        g = int(starts[cn.index(r[0])]) + int(r[1]) - 1
        n_covered += g in rec
        assert np.array_equal(counts_of(r, len(cols)), rec.get(g, zeros)), r[:3]
    assert n_covered > 100
    return n_exp


@pytest.mark.parametrize("env", [{}, {"PECALLER_GUIDE_RANGE_MIN": "64", "PECALLER_TILE_LOG2": "10"}], ids=["per_position", "stretches"])
def test_host_program_with_a_guide_file(exe, guide_dir, env):
    z = np.load(os.path.join(fx.GOLD, "pecall_guide.npz"))
    check_guide(run_host(exe, guide_dir, "2", env, os.path.join(fx.GOLD, "pecall_guide.bed")), z, "pecall_guide")


@pytest.mark.parametrize("env", [{}, {"PECALLER_GUIDE_RANGE_MIN": "64", "PECALLER_TILE_LOG2": "10"}], ids=["per_position", "stretches"])
def test_host_program_guide_ends_with_the_last_stream(exe, guide_end_dir, env):
    z = np.load(os.path.join(fx.GOLD, "pecall_guide.npz"))
    n = check_guide(run_host(exe, guide_end_dir, "2", env, os.path.join(fx.GOLD, "pecall_guide.bed")), z, "pecall_guide_end", _guide_end_limit())
    assert n == 902
