"""pecaller_hip with PECALLER_DEVICE_MERGE=1: the pileup columns are made on the device from the streams' records
(pecall_dev_call_records).  Its files against the same program's files without the switch (same directory, same order of the
samples), against the oracle and the reference's text; the runs the switch must leave to the host path."""
import gzip
import os
import re
import shutil
import struct
import subprocess
import numpy as np
import pytest
import oracle_py
import pecall_sites_fixture as fx
import refio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pecaller_amd", "pecaller_hip")
FILES = ("out.base.gz", "out.snp", "out.piles.gz", "out.dist")


def write_genome(tmp_path, sdx="g1.sdx"):
    _, seqs = refio.read_fasta(os.path.join(fx.GOLD, "g1.fa.gz"))
    shutil.copy(os.path.join(fx.GOLD, sdx), tmp_path / "g1.sdx")
    with gzip.open(tmp_path / "g1.seq", "wb", compresslevel=1) as f:
        f.write(np.concatenate(seqs).tobytes())


def run_both(run, args, env_extra=None):
    """the program without and with the switch in one directory -> (stdout, files) of each; files inflated where gzip"""
    out = []
    for switch in (None, "1"):
        env = dict(os.environ)
        env.pop("PECALLER_DEVICE_MERGE", None)
        env.update(env_extra or {})
        if switch:
            env["PECALLER_DEVICE_MERGE"] = switch
        for f in FILES:
            if os.path.exists(run / f):
                os.remove(run / f)
        stdout = subprocess.run([EXE] + args, cwd=run, stdout=subprocess.PIPE, check=True, env=env).stdout.decode()
        files = {f: (gzip.open(run / f, "rb").read() if f.endswith(".gz") else open(run / f, "rb").read()) for f in FILES}
        out.append((stdout, files))
    return out


def merge_line(stdout):
    m = re.search(r"^ pecaller_hip: device merge: (\d+) columns in (\d+) ranges$", stdout, re.M)
    return (int(m.group(1)), int(m.group(2))) if m else None


def columns_reported(stdout):
    return int(re.search(r"pecaller_hip: (\d+) columns x", stdout).group(1))


def check_rows(files, z, f, names, min_snp):
    """the rows against the oracle in the order this directory gave and, where the order is the fixture's, the reference's text
    (as test_gpu_pecaller_cli.py checks them)"""
    reads, pos = z["reads"], z["pos"]
    base = files["out.base.gz"].decode().split("\n")
    cols = [c for c in base[0].split("\t")[3:] if c]
    assert sorted(cols) == sorted(names)
    perm = [names.index(c) for c in cols]
    r = reads[:, perm, :]
    call, p, typ, ac, _ = oracle_py.call_sites(r, f["dom"])
    rows = {int(x.split("\t")[1]): x for x in base[1:] if x}
    srows = {int(x.split("\t")[1]): x for x in files["out.snp"].decode().split("\n")[1:] if x}
    n_base = n_snp = 0
    for i, q in enumerate(pos):
        pos1 = int(q) + 1
        if f["dom"][i] > 3 or r[i].sum() == 0:
            assert pos1 not in rows
            continue
        n_base += 1
        assert rows[pos1] == fx.base_row("chr1", pos1, chr(f["ref"][i]), call[i], p[i]), pos1
        if typ[i] > 0:
            n_snp += 1
            assert srows[pos1] == fx.snp_row("chr1", pos1, chr(f["ref"][i]), call[i], p[i], typ[i], ac[i]), pos1
        else:
            assert pos1 not in srows
    assert n_base == len(f["base_rows"]) and n_snp > min_snp
    prow = {int(x.split("\t")[1]): x for x in files["out.piles.gz"].decode().split("\n")[1:] if x}
    assert set(prow) == set(srows)
    col_of = {int(q) + 1: i for i, q in enumerate(pos)}
    padding = "".join("\t%d" % v for v in [20, 0, 0, 0, 0, 0] * len(names))
    for k in sorted(prow):                      # every row: the fixture's columns, then the padding columns write_streams appends
        if k in col_of:
            i = col_of[k]
            assert prow[k] == "chr1\t%d\t%s" % (k, chr(f["ref"][i])) + "".join("\t%d" % v for v in r[i].ravel()), k
        else:
            assert int(pos[-1]) + 1 < k <= int(pos[-1]) + 1 + int(z["pad"][0]), k
            assert prow[k] == "chr1\t%d\t%s" % (k, srows[k].split("\t")[2]) + padding, k
    if cols == [str(x) for x in z["columns"]]:
        for pos1, row in f["base_rows"].items():
            assert rows[pos1] == row
        for pos1, row in f["snp_rows"].items():
            assert srows[pos1] == row


def write_streams(run, z, names):
    reads, pos, pad = z["reads"], z["pos"], int(z["pad"][0])
    for s, nm in enumerate(names):
        recs = [struct.pack("<I6H", int(pos[i]), *[int(x) for x in reads[i, s]]) for i in range(len(pos)) if reads[i, s].sum() > 0]
        recs += [struct.pack("<I6H", int(pos[-1]) + 1 + k, 20, 0, 0, 0, 0, 0) for k in range(pad)]
        with gzip.open(run / ("%s.pileup.gz" % nm), "wb", compresslevel=1) as f:
            f.write(b"".join(recs))
    return int((reads.sum(2) > 0).any(1).sum()) + pad


@pytest.mark.parametrize("tile_log2", [None, "10"])
@pytest.mark.parametrize("threads", ["2", "8"])
def test_device_merge_writes_the_host_path_s_files(tmp_path, tile_log2, threads):
    """(tile_log2 = 10: six ranges of 1,024 positions -- records of a stream on both sides of a boundary, the last range partly empty)"""
    assert os.path.exists(EXE), "build with make -C pecaller_amd/csrc"
    z = np.load(os.path.join(fx.GOLD, "pecall_sites.npz"))
    names = [str(x) for x in z["names"]]
    write_genome(tmp_path)
    run = tmp_path / "run"
    run.mkdir()
    n_columns = write_streams(run, z, names)
    (off_out, off_files), (on_out, on_files) = run_both(run, ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", threads, "n"],
                                                        {"PECALLER_TILE_LOG2": tile_log2} if tile_log2 else None)
    assert merge_line(off_out) is None
    got = merge_line(on_out)
    assert got is not None, on_out
    assert got[0] == columns_reported(on_out) == columns_reported(off_out) == n_columns
    if tile_log2:
        assert got[1] >= 6
    for f in FILES:
        assert on_files[f] == off_files[f], f
    check_rows(on_files, z, fx.load(), names, 100)


def test_device_merge_100_samples(tmp_path):
    assert os.path.exists(EXE), "build with make -C pecaller_amd/csrc"
    z = np.load(os.path.join(fx.GOLD, "pecall_wide.npz"))
    names = [str(x) for x in z["names"]]
    write_genome(tmp_path)
    run = tmp_path / "run"
    run.mkdir()
    n_columns = write_streams(run, z, names)
    (off_out, off_files), (on_out, on_files) = run_both(run, ["pileup", str(tmp_path / "g1.sdx"), "105", "out", "0.95", "0.001", "n", "8", "n"])
    assert merge_line(off_out) is None
    got = merge_line(on_out)
    assert got is not None and got[0] == columns_reported(on_out) == n_columns
    for f in FILES:
        assert on_files[f] == off_files[f], f
    check_rows(on_files, z, fx.load("pecall_wide"), names, 30)


def test_device_merge_leaves_unordered_streams_to_the_serial_merge(tmp_path):
    """the streams of test_pecaller_cli_takes_streams_that_are_not_ascending: the walk notices the record out of order before anything
    of it reaches the device, the program says so and starts over with the serial merge -- the files of a run without the switch"""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("mk_unordered", os.path.join(fx.GOLD, "make_golden_pecall_unordered.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    z = np.load(os.path.join(fx.GOLD, "pecall_sites.npz"))
    names = [str(x) for x in z["names"]]
    dist_spec = json.load(open(os.path.join(fx.GOLD, "pecall_unordered.json")))
    write_genome(tmp_path)
    run = tmp_path / "run"
    run.mkdir()
    for s, nm in enumerate(names):
        with gzip.open(run / ("%s.pileup.gz" % nm), "wb", compresslevel=1) as f:
            f.write(b"".join(mk.stream_records(z, s, dist_spec)))
    (off_out, off_files), (on_out, on_files) = run_both(run, ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", "8", "n"],
                                                        {"PECALLER_TILE_LOG2": "10"})
    assert "starting over with the serial merge" in off_out and "starting over with the serial merge" in on_out
    assert merge_line(on_out) is None
    for f in FILES:
        assert on_files[f] == off_files[f], f
    exp = gzip.open(os.path.join(fx.GOLD, "pecall_unordered.base.txt.gz"), "rt").read().split("\n")
    last = int(z["pos"][-1]) + 1
    rows = sorted(x for x in on_files["out.base.gz"].decode().split("\n")[1:] if x and int(x.split("\t")[1]) <= last)
    assert [x.split("\t")[:2] for x in rows] == [x.split("\t")[:2] for x in exp[1:] if x]


def test_device_merge_keeps_the_host_path_with_a_guide_file(tmp_path):
    f = fx.load_guide()
    z = f["z"]
    write_genome(tmp_path, "pecall_guide.sdx")
    run = tmp_path / "run"
    run.mkdir()
    tail = int(z["tail"][0])
    for s, nm in enumerate(f["names"]):
        recs = [struct.pack("<I6H", int(z["pos"][i]), *[int(x) for x in z["reads"][i, s]]) for i in range(len(z["pos"])) if z["reads"][i, s].sum() > 0]
        recs += [struct.pack("<I6H", tail + k, 20, 0, 0, 0, 0, 0) for k in range(40)]
        with gzip.open(run / ("%s.pileup.gz" % nm), "wb", compresslevel=1) as fh:
            fh.write(b"".join(recs))
    (off_out, off_files), (on_out, on_files) = run_both(run, ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", "2", "n",
                                                              os.path.join(fx.GOLD, "pecall_guide.bed")],
                                                        {"PECALLER_GUIDE_RANGE_MIN": "64", "PECALLER_TILE_LOG2": "10"})
    assert merge_line(off_out) is None and merge_line(on_out) is None
    for k in FILES:
        assert on_files[k] == off_files[k], k
    rows = {(x.split("\t")[0], int(x.split("\t")[1])) for x in on_files["out.base.gz"].decode().split("\n")[1:] if x}
    assert len(rows) == len(f["base_rows"])
