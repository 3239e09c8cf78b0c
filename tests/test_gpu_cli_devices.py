"""pemapper_hip under PEMAP_DEVICES: several device objects in one process, the index handed on, batches dealt round robin, the
pileups summed before an output set is written.  Rehearsed with a repeated id on the one GPU of the box (look-up replicas off):
output FILES compared with the reference's, and with the single-object run's where no golden exists."""
import gzip
import os
import shutil
import subprocess
import numpy as np
import pytest
import fixtures
import refio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pecaller_amd", "pemapper_hip")


def _prep(tmp_path):
    """index files next to each other as the reference expects: <base>.sdx and <base>.seq (gz of the letters)"""
    ix = fixtures.index()
    shutil.copy(os.path.join(fixtures.GOLD, "g1.sdx"), tmp_path / "g1.sdx")
    with gzip.open(tmp_path / "g1.seq", "wb", compresslevel=1) as f:
        f.write(ix["genome"].tobytes())
    return str(tmp_path / "g1.sdx")


def _compare(name, out, f1, f2):
    m = fixtures.meta()[name]
    assert np.array_equal(np.fromfile(f1 + ".mfile", dtype="<u4"), fixtures.golden_m(name, 1))
    if f2:
        assert np.array_equal(np.fromfile(f2 + ".mfile", dtype="<u4"), fixtures.golden_m(name, 2))
    pile = refio.read_pileup(out + ".pileup.gz")
    assert len(pile) == m["pileup_records"] and refio.md5(pile) == m["pileup_md5"]
    assert refio.read_indel(out + ".indel.txt.gz") == refio.read_indel(os.path.join(fixtures.GOLD, name + ".indel.txt.gz"))
    assert open(out + ".summary.txt").read() == open(os.path.join(fixtures.GOLD, name + ".summary.txt")).read()


def _env(devices):
    env = dict(os.environ, PEMAP_REPLICAS="0")
    env.pop("PEMAP_DEVICES", None)
    if devices is not None:
        env["PEMAP_DEVICES"] = devices
    return env


def _run(cmd, devices):
    r = subprocess.run(cmd, env=_env(devices), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout[-3000:].decode(errors="replace")
    return r.stdout


def _split_reads(tmp_path, cuts):
    """the golden r150 pairs cut into file pairs at `cuts` (the third one plain text, the others gz) -> the two name lists"""
    g1, g2 = (gzip.open(os.path.join(fixtures.GOLD, "g1_%d_.fastq.gz" % k)).read().split(b"\n") for k in (1, 2))
    n1, n2 = [], []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        fa, fb = str(tmp_path / ("part%d_1_.fastq" % k)), str(tmp_path / ("part%d_2_.fastq" % k))
        if k != 2:
            fa, fb = fa + ".gz", fb + ".gz"
        for fn, lines in ((fa, g1), (fb, g2)):
            data = b"\n".join(lines[4 * a:4 * b]) + b"\n"
            with (gzip.open(fn, "wb", compresslevel=1) if fn.endswith(".gz") else open(fn, "wb")) as f:
                f.write(data)
        n1.append(fa)
        n2.append(fb)
    return n1, n2


@pytest.mark.parametrize("name", ["r150", "r250"])
def test_two_objects_single_file_pair(tmp_path, name):
    assert os.path.exists(EXE), "build with make -C pecaller_amd/csrc"
    sdx = _prep(tmp_path)
    s = fixtures.SETS[name]
    f1 = str(tmp_path / ("%s_1_.fastq.gz" % s["prefix"]))
    f2 = str(tmp_path / ("%s_2_.fastq.gz" % s["prefix"]))
    shutil.copy(os.path.join(fixtures.GOLD, os.path.basename(f1)), f1)
    shutil.copy(os.path.join(fixtures.GOLD, os.path.basename(f2)), f2)
    out = str(tmp_path / "out")
    extra = [str(x) for x in fixtures.meta()[name]["extra_args"]]
    log = _run([EXE, out, sdx, "p", f1, f2, "500", "0", "N", "0.85", "8", "200000000"] + extra, "0,0")
    assert b"pemapper_hip: 2 devices (ids 0,0): index shared in" in log
    assert b"pemapper_hip: pileups of 2 devices merged in" in log
    _compare(name, out, f1, f2)


@pytest.mark.parametrize("workers,batch", [("1", None), ("4", None), ("1", "1000")])
def test_three_objects_array_mode(tmp_path, workers, batch, monkeypatch):
    """five uneven file pairs into one output set, by one worker (which then owns four buffer sets) and by four; and by one worker in
    batches of 1000 pairs, so that a file pair spans up to six batches: the sets go round, a set waits for its own batch on the
    object that batch went to, and one file pair keeps all three objects busy"""
    monkeypatch.setenv("PEMAPPER_FILE_WORKERS", workers)
    if batch:
        monkeypatch.setenv("PEMAPPER_BATCH_PAIRS", batch)
    else:
        monkeypatch.delenv("PEMAPPER_BATCH_PAIRS", raising=False)
    sdx = _prep(tmp_path)
    cuts = [0, 3000, 3001, 9000, 14500, 20000]
    n1, n2 = _split_reads(tmp_path, cuts)
    (tmp_path / "a1.txt").write_text("\n".join(n1) + "\n")
    (tmp_path / "a2.txt").write_text("\n".join(n2) + "\n")
    out = str(tmp_path / "outm")
    log = _run([EXE, out, sdx, "pa", str(tmp_path / "a1.txt"), str(tmp_path / "a2.txt"), "500", "0", "N", "0.85", "16", "200000000"], "0,0,0")
    assert b"pemapper_hip: 3 devices (ids 0,0,0): index shared in" in log and b"pileups of 3 devices merged in" in log
    m = fixtures.meta()["r150"]
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        assert np.array_equal(np.fromfile(n1[k] + ".mfile", dtype="<u4"), fixtures.golden_m("r150", 1)[a:b]), k
        assert np.array_equal(np.fromfile(n2[k] + ".mfile", dtype="<u4"), fixtures.golden_m("r150", 2)[a:b]), k
    pile = refio.read_pileup(out + ".pileup.gz")
    assert len(pile) == m["pileup_records"] and refio.md5(pile) == m["pileup_md5"]
    assert refio.read_indel(out + ".indel.txt.gz") == refio.read_indel(os.path.join(fixtures.GOLD, "r150.indel.txt.gz"))
    assert open(out + ".summary.txt").read() == open(os.path.join(fixtures.GOLD, "r150.summary.txt")).read()


def test_two_output_sets_equal_the_single_object_run(tmp_path):
    """a `pa` list with output names in its second column: setA for pairs [0, 9000), setB for [9000, 20000).  The objects' pileups
    are summed before each set is written and all objects start the next set empty.  No golden exists for half sets: the single-object
    path (checked against the reference by tests/test_gpu_cli.py) is the yardstick."""
    sdx = _prep(tmp_path)
    got = {}
    for tag, devices in (("multi", "0,0"), ("single", None)):
        d = tmp_path / tag
        d.mkdir()
        n1, n2 = _split_reads(d, [0, 9000, 20000])
        outs = [str(d / "setA"), str(d / "setB")]
        (d / "a1.txt").write_text("".join("%s\t%s\n" % (f, o) for f, o in zip(n1, outs)))
        (d / "a2.txt").write_text("".join("%s\t%s\n" % (f, o) for f, o in zip(n2, outs)))
        log = _run([EXE, str(d / "unused"), sdx, "pa", str(d / "a1.txt"), str(d / "a2.txt"), "500", "0", "N", "0.85", "8", "200000000"], devices)
        assert log.count(b"pileups of 2 devices merged in") == (2 if devices else 0)
        files = {}
        for o in outs:
            base = os.path.basename(o)
            files[base + ".pileup"] = gzip.open(o + ".pileup.gz", "rb").read()
            assert len(files[base + ".pileup"]) > 16 * 100000
            # (the strings of one site are printed in the order of the device's insertion log, which is free in either run)
            files[base + ".indel"] = refio.read_indel(o + ".indel.txt.gz")
            files[base + ".indel.header"] = gzip.open(o + ".indel.txt.gz", "rb").readline()
            files[base + ".summary"] = open(o + ".summary.txt").read()
        for k, f in enumerate(n1 + n2):
            files["mfile%d" % k] = open(f + ".mfile", "rb").read()
        assert not os.path.exists(str(d / "unused") + ".summary.txt")
        got[tag] = files
    assert sorted(got["multi"]) == sorted(got["single"])
    for k in got["single"]:
        assert got["multi"][k] == got["single"][k], k
    assert "\nAll\t9000\t1" in got["multi"]["setA.summary"] and "\nAll\t11000\t1" in got["multi"]["setB.summary"]


@pytest.mark.parametrize("devices", ["0,x", ",".join(["0"] * 17)])
def test_bad_device_lists_are_refused(tmp_path, devices):
    sdx = _prep(tmp_path)
    f1 = str(tmp_path / "g1_1_.fastq.gz")
    f2 = str(tmp_path / "g1_2_.fastq.gz")
    shutil.copy(os.path.join(fixtures.GOLD, "g1_1_.fastq.gz"), f1)
    shutil.copy(os.path.join(fixtures.GOLD, "g1_2_.fastq.gz"), f2)
    r = subprocess.run([EXE, str(tmp_path / "out"), sdx, "p", f1, f2, "500", "0", "N", "0.85", "8", "200000000"], env=_env(devices),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 1 and b"PEMAP_DEVICES=" + devices.encode() in r.stdout, r.stdout[-2000:]
    assert not os.path.exists(f1 + ".mfile")
