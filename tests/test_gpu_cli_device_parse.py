"""pemapper_hip with PEMAPPER_DEVICE_PARSE=1: the read files' text goes to the device as it is and the rows are made there
(pemap_dev_submit_fastq) instead of by fill_rows on the host.  Every run here has the switch; the comparisons are those of
test_gpu_cli.py, against the same reference-made goldens: every output file is what it is without the switch."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import fixtures
import refio
from test_gpu_cli import EXE, _compare, _prep

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switch(monkeypatch):
    monkeypatch.setenv("PEMAPPER_DEVICE_PARSE", "1")


def _golden_text():
    return tuple(gzip.open(os.path.join(fixtures.GOLD, "g1_%d_.fastq.gz" % k)).read() for k in (1, 2))


@pytest.mark.parametrize("name", ["r150", "r100", "r250"])
def test_outputs_equal_reference(tmp_path, name):
    assert os.path.exists(EXE), "build with make -C pecaller_amd/csrc"
    sdx = _prep(tmp_path)
    s = fixtures.SETS[name]
    f1 = str(tmp_path / ("%s_1_.fastq.gz" % s["prefix"]))
    shutil.copy(os.path.join(fixtures.GOLD, os.path.basename(f1)), f1)
    f2 = None
    out = str(tmp_path / "out")
    extra = [str(x) for x in fixtures.meta()[name]["extra_args"]]
    if s["paired"]:
        f2 = str(tmp_path / ("%s_2_.fastq.gz" % s["prefix"]))
        shutil.copy(os.path.join(fixtures.GOLD, os.path.basename(f2)), f2)
        cmd = [EXE, out, sdx, "p", f1, f2, "500", "0", "N", "0.85", "8", "200000000"] + extra
    else:
        cmd = [EXE, out, sdx, "s", f1, "N", "0.85", "8", "200000000"] + extra
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    _compare(name, out, f1, f2)


def test_plain_text_with_qualities_that_begin_with_at(tmp_path):
    """the plain-text run of test_cli_plain_text_input_and_uneven_mate_files with every fourth quality line's first byte set to '@':
    the mapper ignores qualities, and the line behind a sequence's '+' is skipped whatever it begins with"""
    sdx = _prep(tmp_path)
    files = []
    for k, g in enumerate(_golden_text()):
        lines = g.split(b"\n")
        for i in range(3, len(lines), 16):
            if lines[i]:
                lines[i] = b"@" + lines[i][1:]
        fn = str(tmp_path / ("p_%d_.fastq" % (k + 1)))
        open(fn, "wb").write(b"\n".join(lines))
        files.append(fn)
    out = str(tmp_path / "outp")
    log = subprocess.check_output([EXE, out, sdx, "p", files[0], files[1], "500", "0", "N", "0.85", "8", "200000000"])
    assert b"read and mapped in" in log
    _compare("r150", out, files[0], files[1])


def test_junk_lines_cut_mate_and_short_first_mate_read(tmp_path):
    sdx = _prep(tmp_path)
    g1, g2 = _golden_text()
    l1, l2 = g1.split(b"\n"), g2.split(b"\n")
    l1[4 * 100:4 * 100] = [b"junk line", b"+another"]
    cut = l1[:]
    cut[4 * 9000 + 1 + 2] = b"ACGTACGTACGT"
    for tag, a, b, n in (("e", l1, l2[:4 * 7000], 7000), ("s", cut, l2, 9000)):
        fa, fb = str(tmp_path / (tag + "_1_.fastq")), str(tmp_path / (tag + "_2_.fastq"))
        open(fa, "wb").write(b"\n".join(a))
        open(fb, "wb").write(b"\n".join(b) + (b"\n" if tag == "e" else b""))
        subprocess.check_call([EXE, str(tmp_path / ("out" + tag)), sdx, "p", fa, fb, "500", "0", "N", "0.85", "8", "200000000"],
                              stdout=subprocess.DEVNULL)
        m1, m2 = np.fromfile(fa + ".mfile", dtype="<u4"), np.fromfile(fb + ".mfile", dtype="<u4")
        assert len(m1) == n and len(m2) == n, (tag, len(m1), len(m2))
        assert np.array_equal(m1, fixtures.golden_m("r150", 1)[:n]) and np.array_equal(m2, fixtures.golden_m("r150", 2)[:n])


@pytest.mark.parametrize("mate", [1, 2])
def test_a_read_of_279_bases_is_the_length_message_and_exit_status_1(tmp_path, mate):
    sdx = _prep(tmp_path)
    texts = [g.split(b"\n") for g in _golden_text()]
    texts[mate - 1][4 * 1234 + 1] = b"ACGT" * 69 + b"ACG"
    files = []
    for k in (1, 2):
        fn = str(tmp_path / ("b_%d_.fastq" % k))
        open(fn, "wb").write(b"\n".join(texts[k - 1]))
        files.append(fn)
    r = subprocess.run([EXE, str(tmp_path / "outb"), sdx, "p", files[0], files[1], "500", "0", "N", "0.85", "8", "200000000"], stdout=subprocess.PIPE)
    assert r.returncode == 1
    assert (" Read 1234 of %s has length 279: supported range is 16..278 " % files[mate - 1]).encode() in r.stdout


def _five_pairs(tmp_path):
    g1, g2 = (g.split(b"\n") for g in _golden_text())
    cuts = [0, 3000, 3001, 9000, 14500, 20000]
    n1, n2 = [], []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        fa, fb = str(tmp_path / ("part%d_1_.fastq" % k)), str(tmp_path / ("part%d_2_.fastq" % k))
        if k != 2:
            fa, fb = fa + ".gz", fb + ".gz"
        for fn, lines in ((fa, g1), (fb, g2)):
            data = b"\n".join(lines[4 * a:4 * b]) + b"\n"
            (gzip.open(fn, "wb", compresslevel=1) if fn.endswith(".gz") else open(fn, "wb")).write(data)
        n1.append(fa)
        n2.append(fb)
    (tmp_path / "a1.txt").write_text("\n".join(n1) + "\n")
    (tmp_path / "a2.txt").write_text("\n".join(n2) + "\n")
    return cuts, n1, n2


def _compare_set(out, cuts, n1, n2):
    m = fixtures.meta()["r150"]
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        assert np.array_equal(np.fromfile(n1[k] + ".mfile", dtype="<u4"), fixtures.golden_m("r150", 1)[a:b]), k
        assert np.array_equal(np.fromfile(n2[k] + ".mfile", dtype="<u4"), fixtures.golden_m("r150", 2)[a:b]), k
    pile = refio.read_pileup(out + ".pileup.gz")
    assert len(pile) == m["pileup_records"] and refio.md5(pile) == m["pileup_md5"]
    assert refio.read_indel(out + ".indel.txt.gz") == refio.read_indel(os.path.join(fixtures.GOLD, "r150.indel.txt.gz"))
    assert open(out + ".summary.txt").read() == open(os.path.join(fixtures.GOLD, "r150.summary.txt")).read()


def test_array_mode_five_uneven_file_pairs_four_workers(tmp_path, monkeypatch):
    monkeypatch.setenv("PEMAPPER_FILE_WORKERS", "4")
    sdx = _prep(tmp_path)
    cuts, n1, n2 = _five_pairs(tmp_path)
    out = str(tmp_path / "outm")
    subprocess.check_call([EXE, out, sdx, "pa", str(tmp_path / "a1.txt"), str(tmp_path / "a2.txt"), "500", "0", "N", "0.85", "16", "200000000"],
                          stdout=subprocess.DEVNULL)
    _compare_set(out, cuts, n1, n2)


def _gz_pair(tmp_path):
    f1, f2 = str(tmp_path / "g1_1_.fastq.gz"), str(tmp_path / "g1_2_.fastq.gz")
    shutil.copy(os.path.join(fixtures.GOLD, "g1_1_.fastq.gz"), f1)
    shutil.copy(os.path.join(fixtures.GOLD, "g1_2_.fastq.gz"), f2)
    return f1, f2


def test_two_device_objects(tmp_path, monkeypatch):
    monkeypatch.setenv("PEMAP_DEVICES", "0,0")
    monkeypatch.setenv("PEMAPPER_BATCH_PAIRS", "3000")
    sdx = _prep(tmp_path)
    f1, f2 = _gz_pair(tmp_path)
    out = str(tmp_path / "outd")
    subprocess.check_call([EXE, out, sdx, "p", f1, f2, "500", "0", "N", "0.85", "8", "200000000"], stdout=subprocess.DEVNULL)
    _compare("r150", out, f1, f2)


@pytest.mark.parametrize("parse_bytes", ["100003", "700"])
def test_small_text_buffer_pieces_end_inside_records_and_batches_come_back_short(tmp_path, monkeypatch, parse_bytes):
    """3,000 pairs a batch take about 930 KB of text a mate: a buffer of 100,003 bytes holds some 320 records and ends in the middle of
    one; a buffer of 700 bytes holds a record or two, and every batch is short (600 pairs are mapped)"""
    monkeypatch.setenv("PEMAPPER_BATCH_PAIRS", "3000")
    monkeypatch.setenv("PEMAPPER_PARSE_BYTES", parse_bytes)
    sdx = _prep(tmp_path)
    f1, f2 = _gz_pair(tmp_path)
    out = str(tmp_path / "outs")
    if parse_bytes == "700":
        log = subprocess.check_output([EXE, out, sdx, "p", f1, f2, "500", "0", "N", "0.85", "8", "600"])
        assert log.count(b"We have read") >= 150
        m1 = np.fromfile(f1 + ".mfile", dtype="<u4")
        assert len(m1) == 600 and np.array_equal(m1, fixtures.golden_m("r150", 1)[:600])
        assert np.array_equal(np.fromfile(f2 + ".mfile", dtype="<u4"), fixtures.golden_m("r150", 2)[:600])
        return
    log = subprocess.check_output([EXE, out, sdx, "p", f1, f2, "500", "0", "N", "0.85", "8", "200000000"])
    assert log.count(b"We have read") > 20000 // 3000 + 1
    _compare("r150", out, f1, f2)


def test_a_line_longer_than_the_text_buffer_grows_it(tmp_path, monkeypatch):
    monkeypatch.setenv("PEMAPPER_PARSE_BYTES", "4096")
    sdx = _prep(tmp_path)
    files = []
    for k, g in enumerate(_golden_text()):
        lines = g.split(b"\n")
        lines[4 * 50] = b"@" + b"h" * 20000          # a header of five buffers
        lines[4 * 60 + 3] = b"I" * 9000             # a quality line of two
        fn = str(tmp_path / ("l_%d_.fastq" % (k + 1)))
        open(fn, "wb").write(b"\n".join(lines))
        files.append(fn)
    out = str(tmp_path / "outl")
    subprocess.check_call([EXE, out, sdx, "p", files[0], files[1], "500", "0", "N", "0.85", "8", "200000000"], stdout=subprocess.DEVNULL)
    _compare("r150", out, files[0], files[1])


def test_max_reads_5000(tmp_path):
    sdx = _prep(tmp_path)
    f1, f2 = _gz_pair(tmp_path)
    (tmp_path / "a1.txt").write_text(f1 + "\n")
    (tmp_path / "a2.txt").write_text(f2 + "\n")
    out = str(tmp_path / "outa")
    subprocess.check_call([EXE, out, sdx, "pa", str(tmp_path / "a1.txt"), str(tmp_path / "a2.txt"), "500", "0", "N", "0.85", "8", "5000"],
                          stdout=subprocess.DEVNULL)
    m1, m2 = np.fromfile(f1 + ".mfile", dtype="<u4"), np.fromfile(f2 + ".mfile", dtype="<u4")
    assert len(m1) == 5000 and np.array_equal(m1, fixtures.golden_m("r150", 1)[:5000])
    assert len(m2) == 5000 and np.array_equal(m2, fixtures.golden_m("r150", 2)[:5000])


def test_single_end_array_mode(tmp_path):
    """'sa' with the switch"""
    sdx = _prep(tmp_path)
    f1 = str(tmp_path / "g1s_1_.fastq.gz")
    shutil.copy(os.path.join(fixtures.GOLD, "g1s_1_.fastq.gz"), f1)
    (tmp_path / "a1.txt").write_text(f1 + "\n")
    out = str(tmp_path / "outsa")
    subprocess.check_call([EXE, out, sdx, "sa", str(tmp_path / "a1.txt"), "N", "0.85", "8", "200000000"], stdout=subprocess.DEVNULL)
    _compare("r100", out, f1, None)
