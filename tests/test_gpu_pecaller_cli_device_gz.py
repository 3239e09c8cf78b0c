"""pecaller_hip with PECALLER_DEVICE_ROWS=1 PECALLER_DEVICE_GZ=1: the rows of <outfile>.base.gz whose posteriors are all 1 are made and
deflated on the device (pecall_dev_sites_base_gz) and go to the file as they come back; the host's rows of the others go in between as
gzip members of its own.  Its files against the same program's files without a switch (same directory, same order of the samples)."""
import gzip
import os
import re
import subprocess
import numpy as np
import pytest
import pecall_sites_fixture as fx
from test_gpu_pecaller_cli_device_merge import EXE, FILES, check_rows, columns_reported, write_genome, write_streams
from test_gpu_pecaller_cli_device_rows import rows_line

pytestmark = pytest.mark.gpu
SWITCHES = ("PECALLER_DEVICE_ROWS", "PECALLER_DEVICE_GZ", "PECALLER_DEVICE_MERGE", "PECALLER_DEVICE_GUIDE")


def run_once(run, args, env_extra, check=True, raw=False):
    """-> (stdout, files); files inflated with the gzip module where gzip (raw: as they lie on the disk)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PECALLER_DEVICE_")}
    env.update(env_extra)
    for f in FILES:
        if os.path.exists(run / f):
            os.remove(run / f)
    p = subprocess.run([EXE] + args, cwd=run, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
    if check:
        assert p.returncode == 0, p.stdout[-2000:].decode(errors="replace")
    files = {f: (gzip.open(run / f, "rb").read() if f.endswith(".gz") and not raw else open(run / f, "rb").read()) for f in FILES if os.path.exists(run / f)}
    return p.stdout.decode(errors="replace"), files, p.returncode


def gz_line(stdout):
    m = re.findall(r"^ pecaller_hip: device gz: (\d+) bytes of text deflated on the device into (\d+) bytes of gz$", stdout, re.M)
    return (int(m[-1][0]), int(m[-1][1])) if m else None


def prepare(tmp_path, tag="pecall_sites"):
    z = np.load(os.path.join(fx.GOLD, tag + ".npz"))
    names = [str(x) for x in z["names"]]
    write_genome(tmp_path)
    run = tmp_path / "run"
    run.mkdir()
    n_columns = write_streams(run, z, names)
    return z, names, run, n_columns


@pytest.mark.parametrize("device_merge", [False, True])
def test_device_gz_writes_the_host_path_s_files(tmp_path, device_merge):
    """PECALLER_TILE_LOG2=10: six tiles of 1,024 positions, each with members and a hole list of its own.  .base.gz inflates to the
    same bytes; .snp, the inflated .piles.gz and .dist are equal"""
    assert os.path.exists(EXE), "build with make -C pecaller_amd/csrc"
    z, names, run, n_columns = prepare(tmp_path)
    args = ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", "8", "n"]
    env = {"PECALLER_TILE_LOG2": "10"}
    if device_merge:
        env["PECALLER_DEVICE_MERGE"] = "1"
    off_out, off_files, _ = run_once(run, args, env)
    on_out, on_files, _ = run_once(run, args, dict(env, PECALLER_DEVICE_ROWS="1", PECALLER_DEVICE_GZ="1"))
    assert gz_line(off_out) is None and rows_line(off_out) is None
    assert sorted(on_files) == sorted(off_files) == sorted(FILES)
    for f in FILES:
        assert on_files[f] == off_files[f], f
    rows, text = rows_line(on_out), gz_line(on_out)
    assert rows is not None and text is not None, on_out
    base = on_files["out.base.gz"]
    n_rows = len([x for x in base.decode().split("\n")[1:] if x])
    assert rows[0] + rows[1] == n_rows and rows[0] > 0 and rows[1] >= 30
    # the device's text is the file less the header line and the holes' rows; it shrank
    assert 0 < text[1] < text[0] < len(base)
    assert columns_reported(on_out) == columns_reported(off_out) == n_columns
    assert ("device merge:" in on_out) == device_merge
    check_rows(on_files, z, fx.load(), names, 100)


def test_device_gz_100_samples(tmp_path):
    """rows of ~420 bytes, tiles of 4,096 positions: runs of several pieces between the holes"""
    z, names, run, n_columns = prepare(tmp_path, "pecall_wide")
    args = ["pileup", str(tmp_path / "g1.sdx"), "105", "out", "0.95", "0.001", "n", "8", "n"]
    off_out, off_files, _ = run_once(run, args, {"PECALLER_TILE_LOG2": "12"})
    on_out, on_files, _ = run_once(run, args, {"PECALLER_TILE_LOG2": "12", "PECALLER_DEVICE_ROWS": "1", "PECALLER_DEVICE_GZ": "1"})
    for f in FILES:
        assert on_files[f] == off_files[f], f
    assert gz_line(on_out) is not None and columns_reported(on_out) == n_columns
    check_rows(on_files, z, fx.load("pecall_wide"), names, 30)


def test_device_gz_alone_is_refused(tmp_path):
    z, names, run, _ = prepare(tmp_path)
    out, _, rc = run_once(run, ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", "2", "n"], {"PECALLER_DEVICE_GZ": "1"}, check=False)
    assert rc != 0
    assert "PECALLER_DEVICE_GZ=1 needs PECALLER_DEVICE_ROWS=1" in out


def test_no_switch_writes_what_a_clean_environment_writes(tmp_path):
    """the switches set to 0 against an environment without any PECALLER_DEVICE_* variable: the four files byte for byte"""
    z, names, run, _ = prepare(tmp_path)
    args = ["pileup", str(tmp_path / "g1.sdx"), "20", "out", "0.95", "0.001", "n", "4", "n"]
    _, clean, _ = run_once(run, args, {"PECALLER_TILE_LOG2": "10"}, raw=True)
    _, zeros, _ = run_once(run, args, dict({k: "0" for k in SWITCHES}, PECALLER_TILE_LOG2="10"), raw=True)
    assert sorted(clean) == sorted(zeros) == sorted(FILES)
    for f in FILES:
        assert clean[f] == zeros[f], f
