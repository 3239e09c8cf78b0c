"""pemapper_hip with PEMAPPER_DEVICE_GZ=1: the records of <out>.pileup.gz are deflated on the device (pemap_dev_fetch_records_gz) and
written as they come back.  The file is a chain of BGZF members that ends in the empty one; it inflates to the bytes the run without
the switch inflates to, and every other file is the same.  Both runs are this program's: the run without the switch is what
tests/test_gpu_cli.py holds against the reference's goldens.  (indel.txt.gz is compared row by row with the strings of a site sorted,
as everywhere: their order is the order of the device's insertion log, which is free from run to run.)"""
import gzip
import os
import shutil
import subprocess
import pytest
import fixtures
import refio
import pileup_gz_cases as pc
from test_gpu_cli import EXE, _prep

pytestmark = pytest.mark.gpu
SWITCHES = ("PEMAPPER_DEVICE_GZ", "PEMAPPER_DEVICE_PARSE", "PEMAPPER_OUTPUT_TIMES")


def run(cmd, env_extra, check=True):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES and k != "PEMAP_DEVICES"}
    env.update(env_extra)
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if check:
        assert r.returncode == 0, r.stdout[-3000:].decode(errors="replace")
    return r


def copy_reads(d, prefix, paired):
    names = []
    for k in ((1, 2) if paired else (1,)):
        f = str(d / ("%s_%d_.fastq.gz" % (prefix, k)))
        shutil.copy(os.path.join(fixtures.GOLD, os.path.basename(f)), f)
        names.append(f)
    return names


def outputs(outs, reads, raw=False):
    """the files of a run by name; raw: as they lie on the disk"""
    files = {}
    for o in outs:
        base = os.path.basename(o)
        files[base + ".pileup"] = open(o + ".pileup.gz", "rb").read() if raw else gzip.open(o + ".pileup.gz", "rb").read()
        if raw:
            files[base + ".indel"] = open(o + ".indel.txt.gz", "rb").read()
        else:
            files[base + ".indel"] = refio.read_indel(o + ".indel.txt.gz")
            files[base + ".indel.header"] = gzip.open(o + ".indel.txt.gz", "rb").readline()
        files[base + ".summary"] = open(o + ".summary.txt").read()
    for k, f in enumerate(reads):
        files["mfile%d" % k] = open(f + ".mfile", "rb").read()
    return files


def check_bgzf(path, inflated):
    """walked by the heads alone: members of at most 65,536 bytes and 512 records, the empty one last and only there"""
    gz = open(path, "rb").read()
    members = pc.walk(gz)
    assert members[-1] == (pc.EOF, b"") and gz.endswith(pc.EOF)
    assert all(0 < len(t) <= pc.PIECE and len(m) <= 65536 for m, t in members[:-1])
    assert all(len(t) == pc.PIECE for _, t in members[:-2])
    assert b"".join(t for _, t in members) == inflated
    return len(members)


def on_and_off(tmp_path, make_cmd, extra_env=None):
    """the same command line in two directories, without and with the switch -> (files off, files on, outs on, log on)"""
    got = {}
    for tag, env in (("off", {}), ("on", {"PEMAPPER_DEVICE_GZ": "1"})):
        d = tmp_path / tag
        d.mkdir()
        cmd, outs, reads = make_cmd(d)
        log = run(cmd, dict(extra_env or {}, **env)).stdout
        got[tag] = (outputs(outs, reads), outs, log)
    off, on = got["off"][0], got["on"][0]
    assert sorted(on) == sorted(off)
    for k in off:
        assert on[k] == off[k], k
    with pytest.raises(AssertionError):
        pc.walk(open(got["off"][1][0] + ".pileup.gz", "rb").read())      # (the host's members carry no lengths)
    return off, on, got["on"][1], got["on"][2]


def test_paired_golden(tmp_path):
    assert os.path.exists(EXE), "build with make -C pecaller_amd/csrc"
    sdx = _prep(tmp_path)

    def make(d):
        f1, f2 = copy_reads(d, "g1", True)
        return [EXE, str(d / "out"), sdx, "p", f1, f2, "500", "0", "N", "0.85", "8", "200000000"], [str(d / "out")], [f1, f2]
    off, on, outs, log = on_and_off(tmp_path, make)
    m = fixtures.meta()["r150"]
    pile = refio.read_pileup(outs[0] + ".pileup.gz")
    assert len(pile) == m["pileup_records"] and refio.md5(pile) == m["pileup_md5"]
    assert check_bgzf(outs[0] + ".pileup.gz", on["out.pileup"]) == (m["pileup_records"] + pc.PIECE_RECORDS - 1) // pc.PIECE_RECORDS + 1
    assert b"outputs of" not in log


def test_single_end_golden_and_output_times(tmp_path):
    sdx = _prep(tmp_path)

    def make(d):
        f1, = copy_reads(d, "g1s", False)
        return [EXE, str(d / "out"), sdx, "s", f1, "N", "0.85", "8", "200000000"], [str(d / "out")], [f1]
    off, on, outs, log = on_and_off(tmp_path, make, {"PEMAPPER_OUTPUT_TIMES": "1"})
    check_bgzf(outs[0] + ".pileup.gz", on["out.pileup"])
    import re
    assert len(re.findall(rb"\n pemapper_hip: outputs of \S+out written in \d+\.\d{3} s", log)) == 1


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_array_mode_with_two_output_names(tmp_path, devices):
    """setA for the pairs [0, 9000), setB for the rest: two files of members, each with its own empty member; under PEMAP_DEVICES the
    members are made after the objects' pileups were summed"""
    from test_gpu_cli_devices import _split_reads
    sdx = _prep(tmp_path)

    def make(d):
        n1, n2 = _split_reads(d, [0, 9000, 20000])
        outs = [str(d / "setA"), str(d / "setB")]
        (d / "a1.txt").write_text("".join("%s\t%s\n" % (f, o) for f, o in zip(n1, outs)))
        (d / "a2.txt").write_text("".join("%s\t%s\n" % (f, o) for f, o in zip(n2, outs)))
        return [EXE, str(d / "unused"), sdx, "pa", str(d / "a1.txt"), str(d / "a2.txt"), "500", "0", "N", "0.85", "8", "200000000"], outs, n1 + n2
    env = {"PEMAP_REPLICAS": "0"}
    if devices:
        env["PEMAP_DEVICES"] = devices
    off, on, outs, log = on_and_off(tmp_path, make, env)
    for o in outs:
        assert check_bgzf(o + ".pileup.gz", on[os.path.basename(o) + ".pileup"]) > 100
    assert log.count(b"pileups of 2 devices merged in") == (2 if devices else 0)


def test_nothing_mapped_is_the_empty_member(tmp_path):
    """reads that map nowhere: the 28-byte empty member is the whole file"""
    sdx = _prep(tmp_path)
    f1 = str(tmp_path / "junk_1_.fastq")
    import random
    rnd = random.Random(7)
    with open(f1, "w") as f:
        for k in range(50):
            f.write("@r%d\n%s\n+\n%s\n" % (k, "".join(rnd.choice("ACGT") for _ in range(80)), "I" * 80))
    run([EXE, str(tmp_path / "out"), sdx, "s", f1, "N", "0.85", "8", "200000000"], {"PEMAPPER_DEVICE_GZ": "1"})
    assert open(tmp_path / "out.pileup.gz", "rb").read() == pc.EOF


def test_switch_unset_or_0_writes_the_same_bytes(tmp_path):
    """a clean environment against every switch set to 0: all files byte for byte"""
    sdx = _prep(tmp_path)
    got = {}
    for tag, env in (("clean", {}), ("zeros", {k: "0" for k in SWITCHES})):
        d = tmp_path / tag
        d.mkdir()
        f1, f2 = copy_reads(d, "g1", True)
        log = run([EXE, str(d / "out"), sdx, "p", f1, f2, "500", "0", "N", "0.85", "8", "200000000"], env).stdout
        assert b"outputs of" not in log
        got[tag] = dict(outputs([str(d / "out")], [f1, f2], raw=True), rows=refio.read_indel(str(d / "out") + ".indel.txt.gz"))
    for k in got["clean"]:
        if not k.endswith(".indel"):        # (deflated rows whose strings come in the insertion log's order: compared as rows)
            assert got["clean"][k] == got["zeros"][k], k
    assert len(got["clean"]["rows"]) > 10


def test_a_library_without_the_entry_refuses_the_switch(tmp_path):
    """the program next to a stand-in library that exports every entry it needs but pemap_dev_fetch_records_gz (the symbol is weak)"""
    sdx = _prep(tmp_path)
    d = tmp_path / "standin"
    d.mkdir()
    exe = str(d / "pemapper_hip")
    shutil.copy(EXE, exe)
    syms = [l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--undefined-only", EXE]).decode().splitlines() if " pemap_dev_" in l]
    assert "pemap_dev_fetch_records_gz" in syms and "pemap_dev_create" in syms
    src = "".join('const char *%s (void) { return "stand-in"; }\n' % s if s == "pemap_dev_last_error" else "int %s (void) { return 1; }\n" % s
                  for s in syms if s != "pemap_dev_fetch_records_gz")
    (d / "standin.c").write_text(src)
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(d / "libpemap_hip.so"), str(d / "standin.c")])
    f1, = copy_reads(d, "g1s", False)
    cmd = [exe, str(d / "out"), sdx, "s", f1, "N", "0.85", "8", "200000000"]
    r = run(cmd, {"PEMAPPER_DEVICE_GZ": "1"}, check=False)
    assert r.returncode == 1 and b"PEMAPPER_DEVICE_GZ=1 needs pemap_dev_fetch_records_gz, which this library lacks" in r.stdout, r.stdout[-2000:]
    r = run(cmd, {}, check=False)
    assert r.returncode != 0 and b"PEMAPPER_DEVICE_GZ" not in r.stdout
