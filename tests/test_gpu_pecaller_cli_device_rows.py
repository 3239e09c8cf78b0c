"""pecaller_hip with PECALLER_DEVICE_ROWS=1: the rows of <outfile>.base.gz whose posteriors are all 1 are made on the device
(pecall_dev_sites_base_text), the host formats the others and splices them in.  Its files against the same program's files without
the switch (same directory, same order of the samples), with the host merge and with PECALLER_DEVICE_MERGE=1, in guide mode and after
a restart into the serial merge; against the oracle and the reference's text."""
import gzip
import os
import re
import struct
import subprocess
import numpy as np
import pytest
import pecall_sites_fixture as fx
from test_gpu_pecaller_cli_device_merge import EXE, FILES, check_rows, columns_reported, write_genome, write_streams

pytestmark = pytest.mark.gpu


def run_both(run, args, env_extra=None):
    """the program without and with the switch in one directory -> (stdout, files) of each; files inflated where gzip"""
    out = []
    for switch in (None, "1"):
        env = dict(os.environ)
        for k in ("PECALLER_DEVICE_ROWS", "PECALLER_DEVICE_MERGE"):
            env.pop(k, None)
        env.update(env_extra or {})
        if switch:
            env["PECALLER_DEVICE_ROWS"] = switch
        for f in FILES:
            if os.path.exists(run / f):
                os.remove(run / f)
        stdout = subprocess.run([EXE] + args, cwd=run, stdout=subprocess.PIPE, check=True, env=env).stdout.decode()
        files = {f: (gzip.open(run / f, "rb").read() if f.endswith(".gz") else open(run / f, "rb").read()) for f in FILES}
        out.append((stdout, files))
    return out


def rows_line(stdout):
    m = re.findall(r"^ pecaller_hip: device rows: (\d+) rows from the device, (\d+) holes formatted by the host$", stdout, re.M)
    return (int(m[-1][0]), int(m[-1][1])) if m else None


def check_switch(off, on, min_holes=1):
    (off_out, off_files), (on_out, on_files) = off, on
    assert rows_line(off_out) is None
    got = rows_line(on_out)
    assert got is not None, on_out
    for f in FILES:
        assert on_files[f] == off_files[f], f
    n_rows = len([x for x in on_files["out.base.gz"].decode().split("\n")[1:] if x])
    assert got[0] + got[1] == n_rows and got[0] > 0 and got[1] >= min_holes, (got, n_rows)
    return got


@pytest.mark.parametrize("device_merge", [False, True])
@pytest.mark.parametrize("tile_log2", [None, "10"])
@pytest.mark.parametrize("threads", ["2", "8"])
def test_device_rows_write_the_host_path_s_files(tmp_path, tile_log2, threads, device_merge):
    """(tile_log2 = 10: six tiles of 1,024 positions, each with a text and a hole list of its own)"""
    assert os.path.exists(EXE), "build with make -C pecaller_amd/csrc"
    z = np.load(os.path.join(fx.GOLD, "pecall_sites.npz"))
    names = [str(x) for x in z["names"]]
    write_genome(tmp_path)
    run = tmp_path / "run"
    run.mkdir()
    n_columns = write_streams(run, z, names)
    env = {"PECALLER_TILE_LOG2": tile_log2} if tile_log2 else {}
    if device_merge:
        env["PECALLER_DEVICE_MERGE"] = "1"
    off, on = run_both(run, ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", threads, "n"], env)
    check_switch(off, on, 30)
    assert columns_reported(on[0]) == columns_reported(off[0]) == n_columns
    assert ("device merge:" in on[0]) == device_merge
    check_rows(on[1], z, fx.load(), names, 100)


def test_device_rows_with_a_hole_list_that_is_too_short(tmp_path):
    """PECALLER_POST_CAP=3: the list of posteriors and the hole list begin with three entries; both calls are made again with the
    size the library asked for"""
    z = np.load(os.path.join(fx.GOLD, "pecall_sites.npz"))
    names = [str(x) for x in z["names"]]
    write_genome(tmp_path)
    run = tmp_path / "run"
    run.mkdir()
    write_streams(run, z, names)
    off, on = run_both(run, ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", "4", "n"], {"PECALLER_TILE_LOG2": "11", "PECALLER_POST_CAP": "3"})
    check_switch(off, on, 30)
    check_rows(on[1], z, fx.load(), names, 100)


def test_device_rows_100_samples(tmp_path):
    z = np.load(os.path.join(fx.GOLD, "pecall_wide.npz"))
    names = [str(x) for x in z["names"]]
    write_genome(tmp_path)
    run = tmp_path / "run"
    run.mkdir()
    n_columns = write_streams(run, z, names)
    off, on = run_both(run, ["pileup", str(tmp_path / "g1.sdx"), "105", "out", "0.95", "0.001", "n", "8", "n"])
    check_switch(off, on, 10)
    assert columns_reported(on[0]) == n_columns
    check_rows(on[1], z, fx.load("pecall_wide"), names, 30)


def test_device_rows_with_a_guide_file(tmp_path):
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
    off, on = run_both(run, ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", "2", "n", os.path.join(fx.GOLD, "pecall_guide.bed")],
                       {"PECALLER_GUIDE_RANGE_MIN": "64", "PECALLER_TILE_LOG2": "10"})
    check_switch(off, on)
    rows = {(x.split("\t")[0], int(x.split("\t")[1])): x for x in on[1]["out.base.gz"].decode().split("\n")[1:] if x}
    assert len(rows) == len(f["base_rows"])
    assert len(set(k[0] for k in rows)) > 1          # (several contig names in the device's text)
    if [c for c in on[1]["out.base.gz"].decode().split("\n")[0].split("\t")[3:] if c] == f["columns"]:
        for k, row in f["base_rows"].items():
            assert rows[k] == row, k


def test_device_rows_after_a_restart_into_the_serial_merge(tmp_path):
    """the streams of test_pecaller_cli_takes_streams_that_are_not_ascending: the run is abandoned and starts over with the serial
    merge, whose tiles get their text from the device all the same"""
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
    off, on = run_both(run, ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", "8", "n"], {"PECALLER_TILE_LOG2": "10"})
    assert "starting over with the serial merge" in off[0] and "starting over with the serial merge" in on[0]
    check_switch(off, on, 30)
    exp = gzip.open(os.path.join(fx.GOLD, "pecall_unordered.base.txt.gz"), "rt").read().split("\n")
    last = int(z["pos"][-1]) + 1
    rows = sorted(x for x in on[1]["out.base.gz"].decode().split("\n")[1:] if x and int(x.split("\t")[1]) <= last)
    assert [x.split("\t")[:2] for x in rows] == [x.split("\t")[:2] for x in exp[1:] if x]
