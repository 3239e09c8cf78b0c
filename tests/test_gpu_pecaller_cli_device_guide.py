"""pecaller_hip with a BED guide file and PECALLER_DEVICE_GUIDE=1: runs of BED lines go to the device as ranges of intervals
(pecall_dev_call_records_guided).  Its files against the same program's files without the switch (same directory, same order of the
samples) and against what the unmodified reference wrote (tests/golden/make_golden_pecall_guide*.py)."""
import gzip
import json
import os
import re
import shutil
import struct
import subprocess
import numpy as np
import pytest
import pecall_sites_fixture as fx
import refio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pecaller_amd", "pecaller_hip")
FILES = ("out.base.gz", "out.snp", "out.piles.gz", "out.dist")
# fixture -> records, BED, the goldens' stem, whether the streams end at the guide_end fixture's cut
FIXTURES = {
    "pecall_guide": ("pecall_guide.npz", "pecall_guide.bed", "pecall_guide", False),
    "pecall_guide_end": ("pecall_guide.npz", "pecall_guide.bed", "pecall_guide_end", True),
    "pecall_guide_many": ("pecall_guide_many.npz", "pecall_guide_many.bed", "pecall_guide_many", False),
    "pecall_guide_many_back": ("pecall_guide_many.npz", "pecall_guide_many_back.bed", "pecall_guide_many_back", False),
}


def write_inputs(tmp_path, npz, cut):
    z = np.load(os.path.join(fx.GOLD, npz))
    _, seqs = refio.read_fasta(os.path.join(fx.GOLD, "g1.fa.gz"))
    shutil.copy(os.path.join(fx.GOLD, "pecall_guide.sdx"), tmp_path / "g1.sdx")
    with gzip.open(tmp_path / "g1.seq", "wb", compresslevel=1) as f:
        f.write(np.concatenate(seqs).tobytes())
    run = tmp_path / "run"
    run.mkdir()
    limit = None
    if cut:
        lens, cn, _ = refio.read_sdx(os.path.join(fx.GOLD, "pecall_guide.sdx"))
        starts = np.concatenate([[0], np.cumsum(np.array(lens) + 15)])
        limit = int(starts[cn.index("chrMT")]) + json.load(open(os.path.join(fx.GOLD, "pecall_guide_end.json")))["cut"] - 1
    reads, pos, tail = z["reads"], z["pos"], int(z["tail"][0])       # (an .npz inflates an array every time it is asked for)
    for s, nm in enumerate(str(x) for x in z["names"]):
        recs = [struct.pack("<I6H", int(pos[i]), *[int(x) for x in reads[i, s]]) for i in range(len(pos))
                if reads[i, s].sum() > 0 and (limit is None or int(pos[i]) <= limit)]
        if limit is None:
            recs += [struct.pack("<I6H", tail + k, 20, 0, 0, 0, 0, 0) for k in range(40)]
        with gzip.open(run / ("%s.pileup.gz" % nm), "wb", compresslevel=1) as f:
            f.write(b"".join(recs))
    return run, z


def run_one(run, args, env_extra):
    """-> (stdout, files); files inflated where gzip"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PECALLER_")}
    env.update(env_extra)
    for f in FILES:
        if os.path.exists(run / f):
            os.remove(run / f)
    stdout = subprocess.run([EXE] + args, cwd=run, stdout=subprocess.PIPE, check=True, env=env).stdout.decode()
    return stdout, {f: (gzip.open(run / f, "rb").read() if f.endswith(".gz") else open(run / f, "rb").read()) for f in FILES}


def run_both(run, args, env_extra=None):
    """the program without and with the switch in one directory"""
    return [run_one(run, args, dict(env_extra or {}, **sw)) for sw in ({}, {"PECALLER_DEVICE_GUIDE": "1"})]


def guide_line(stdout):
    m = re.search(r"^ pecaller_hip: device guide merge: (\d+) columns of (\d+) intervals in (\d+) ranges$", stdout, re.M)
    return tuple(int(x) for x in m.groups()) if m else None


def columns_reported(stdout):
    return int(re.search(r"pecaller_hip: (\d+) columns x", stdout).group(1))


def key_of(row):
    x = row.split("\t")
    return x[0], int(x[1])


def check_against_the_reference(files, golden, columns):
    """the rows' contigs and positions and <out>.dist, field for field by sample name, are the reference's; where this directory's
    order of the samples is the fixture's, the rows' whole text too (as test_gpu_pecaller_cli.py::test_pecaller_cli_guide_mode)"""
    base = files["out.base.gz"].decode().split("\n")
    snp = files["out.snp"].decode().split("\n")
    exp_base = gzip.open(os.path.join(fx.GOLD, golden + ".base.txt.gz"), "rt").read().split("\n")
    cols = [c for c in base[0].split("\t")[3:] if c]
    assert sorted(cols) == sorted(columns)
    rows, exp_rows = sorted(x for x in base[1:] if x), [x for x in exp_base[1:] if x]
    assert sorted(key_of(x) for x in rows) == sorted(key_of(x) for x in exp_rows)
    got_d = [x.split("\t") for x in files["out.dist"].decode().split("\n")]
    exp_d = [x.split("\t") for x in open(os.path.join(fx.GOLD, golden + ".dist.txt")).read().split("\n")]
    assert len(got_d) == len(exp_d)
    for g, e in zip(got_d, exp_d):
        assert g[0] == e[0]
        if len(g) > 1:
            assert dict(zip(got_d[0][1:], g[1:])) == dict(zip(exp_d[0][1:], e[1:])), g[0]
    snp_golden = os.path.join(fx.GOLD, golden + ".snp.txt")
    if os.path.exists(snp_golden):
        exp_snp = [x for x in open(snp_golden).read().split("\n")[1:] if x]
        assert sorted(key_of(x) for x in snp[1:] if x) == sorted(key_of(x) for x in exp_snp)
        if cols == columns:
            assert sorted(x for x in snp[1:] if x) == exp_snp
    if cols == columns:
        assert rows == exp_rows
    return len(rows)


@pytest.mark.parametrize("tile_log2", [None, "10"])
@pytest.mark.parametrize("fixture", list(FIXTURES))
def test_device_guide_writes_the_host_path_s_files(tmp_path, fixture, tile_log2):
    """(tile_log2 = 10: ranges of 1,024 positions, so that intervals and gaps straddle ranges)"""
    assert os.path.exists(EXE), "build with make -C pecaller_amd/csrc"
    npz, bed_name, golden, cut = FIXTURES[fixture]
    run, z = write_inputs(tmp_path, npz, cut)
    bed = os.path.join(fx.GOLD, bed_name)
    n_lines = len([x for x in open(bed).read().split("\n") if x])
    (off_out, off_files), (on_out, on_files) = run_both(run, ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", "2", "n", bed],
                                                        {"PECALLER_TILE_LOG2": tile_log2} if tile_log2 else None)
    assert guide_line(off_out) is None and "device guide merge" not in off_out
    got = guide_line(on_out)
    assert got is not None, on_out
    n_cols, n_iv, n_ranges = got
    assert n_cols == columns_reported(on_out) == columns_reported(off_out)
    for f in FILES:
        assert on_files[f] == off_files[f], f
    n_rows = check_against_the_reference(on_files, golden, [str(x) for x in z["columns"]])
    assert n_rows <= n_cols
    if fixture == "pecall_guide_many_back":
        assert n_iv < n_lines or n_ranges > 1        # the lines that go backwards: left to the host, or ranges of their own
    if fixture == "pecall_guide_end":
        assert n_rows == 902                         # (the last row is the column at which the last stream ends)
    if tile_log2 and fixture.startswith("pecall_guide_many"):
        assert n_ranges >= 10


def test_device_guide_with_device_rows(tmp_path):
    assert os.path.exists(EXE), "build with make -C pecaller_amd/csrc"
    npz, bed_name, golden, cut = FIXTURES["pecall_guide_many_back"]
    run, z = write_inputs(tmp_path, npz, cut)
    args = ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", "8", "n", os.path.join(fx.GOLD, bed_name)]
    (off_out, off_files), (on_out, on_files) = run_both(run, args, {"PECALLER_TILE_LOG2": "10", "PECALLER_DEVICE_ROWS": "1"})
    plain_out, plain_files = run_one(run, args, {"PECALLER_TILE_LOG2": "10"})
    got = guide_line(on_out)
    assert got is not None and got[0] == columns_reported(on_out)
    m = re.search(r"device rows: (\d+) rows from the device", on_out)
    assert m and int(m.group(1)) > 1000
    for f in FILES:
        assert on_files[f] == off_files[f] == plain_files[f], f
    check_against_the_reference(on_files, golden, [str(x) for x in z["columns"]])
