"""The gzip rule of the device-made <out>.pileup.gz (pecaller_amd/csrc/pemap_gz_rule.h: what the kernels of pemap_gz.hip.h,
pemapper_main.c and tests/csrc/pemap_gz_rule_check.c all call) on the CPU, through the stand-alone program, and the C-ABI entries
pemap_dev_fetch_records_gz / pemap_dev_fetch_gz_ms as names.  The program is built twice, plainly and with the address and
undefined-behaviour sanitizers; both run on the same cases and must write the same bytes.  Nothing of it is loaded into Python."""
import ctypes
import gzip
import os
import re
import subprocess
import zlib
import numpy as np
import pytest
import pileup_gz_cases as pc

ROOT = pc.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return pc.build_check(tmp_path_factory.mktemp("pemap_gz_rule"))


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return pc.build_check(tmp_path_factory.mktemp("pemap_gz_rule_san"), sanitize=True)


@pytest.fixture(scope="module")
def cases():
    return pc.cases()


@pytest.fixture(scope="module")
def fic(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fic") / "fast_inflate_check")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "csrc", "fast_inflate_check.c"), "-lz", "-lpthread"])
    return exe


def test_the_header_is_plain_c():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", pc.RULE])
    assert pc.PIECE_RECORDS in (512, 1024) and 1 <= pc.CODES <= 4
    assert pc.MEMBER_MAX < 65536


def test_the_cases_cover_what_they_should(cases):
    R = pc.PIECE_RECORDS
    assert [len(cases["records_%d" % n]) // 16 for n in (1, R - 1, R, R + 1, 2 * R + 1)] == [1, 511, 512, 513, 1025]
    assert [len(p) for p in pc.pieces(cases["records_1025"])] == [pc.PIECE, pc.PIECE, 16]
    assert pc.flag_runs(cases["runs"]) == list(pc.RUNS) and len(cases["runs"]) <= pc.PIECE
    two = pc.pieces(cases["repeat_across_pieces"])
    assert len(two) == 2 and two[1][:16] == two[0][-16:]
    hi = np.frombuffer(cases["high_bytes"], pc.PILE_DT)
    assert hi["c"].max() > 255 and hi["pos"].min() >= 1 << 31 and np.all(np.diff(hi["pos"].astype(np.int64)) > 0)
    for name, data in cases.items():
        if name.startswith(("records_", "depth_")) and len(data) > 16:
            assert 3 <= max(max(pc.flag_runs(p) or [0]) for p in pc.pieces(data)) <= 18, name


@pytest.mark.parametrize("name", sorted(pc.cases()))
def test_members_of_a_case(exe, exe_san, fic, cases, tmp_path, name):
    """every member is found from the heads' lengths, inflates on its own to its piece (the closed-form parse equalled the greedy
    one, or the program had failed); the gzip module and the repository's own inflater give the whole input; no member is longer
    than the stored form of its piece; the sanitizer build writes the same bytes"""
    data = cases[name]
    gz, forms = pc.encode(exe, tmp_path, data)
    gz_san, forms_san = pc.encode(exe_san, tmp_path, data, tag="san")
    assert gz_san == gz and forms_san == forms
    want = pc.pieces(data)
    got = pc.walk(gz)
    assert len(got) == len(want)
    for (member, inflated), piece in zip(got, want):
        assert inflated == piece
        assert len(member) <= pc.HEAD + 5 + len(piece) + 8
        assert zlib.decompress(member, 31) == piece
    assert gzip.decompress(gz) == data
    assert gzip.decompress(gz + pc.EOF) == data
    out = str(tmp_path / "inflated")
    subprocess.check_call([fic, "cat", str(tmp_path / "t.gz"), out])
    assert open(out, "rb").read() == data


def test_forms_and_sizes(exe, cases, tmp_path):
    """random bytes go stored, exactly; the short piece goes with the fixed code; records go with a preset code and shrink well
    below half; each depth's records choose a table made for it"""
    gz, forms = pc.encode(exe, tmp_path, cases["random"])
    assert forms[0] == 2 and sum(forms) == 2 and len(gz) == sum(pc.HEAD + 5 + len(p) + 8 for p in pc.pieces(cases["random"]))
    gz, forms = pc.encode(exe, tmp_path, cases["short_fixed"])
    assert forms[1] == 1 and sum(forms) == 1 and len(gz) < pc.HEAD + 5 + 48 + 8
    gz, forms = pc.encode(exe, tmp_path, cases["records_1025"])
    assert sum(forms[2:]) >= 2 and len(gz) * 2 < len(cases["records_1025"])
    for depth in (1, 5, 100, 300):
        data = cases["depth_%d" % depth]
        gz, forms = pc.encode(exe, tmp_path, data)
        assert forms[0] == 0 and sum(forms[2:]) >= 1 and len(gz) * 2 < len(data), depth


def test_runs_at_the_cap(exe, tmp_path):
    """a run of 258 set flags is one token and one of 259 is not; a remainder of 1 or 2 behind a full match goes as literals (the
    program compared every case with the byte-by-byte parse); every length from 255 to 264 inflates"""
    size = {}
    for r in list(range(255, 265)) + [516, 517, 518, 519]:
        data = pc.flags_with_runs([r])
        gz, _ = pc.encode(exe, tmp_path, data, tag="r%d" % r)
        assert gzip.decompress(gz) == data
        size[r] = len(gz)
    assert size[259] > size[258] and size[517] > size[516]


def test_no_match_reaches_in_front_of_its_piece(exe, cases, tmp_path):
    """a member made of a piece alone equals the member made of it inside a longer input, also where the piece begins with the 16
    bytes the piece in front ends with"""
    for name in ("repeat_across_pieces", "records_1025"):
        whole = pc.walk(pc.encode(exe, tmp_path, cases[name])[0])
        for k, piece in enumerate(pc.pieces(cases[name])):
            assert pc.encode(exe, tmp_path, piece, tag="p%d" % k)[0] == whole[k][0], (name, k)
    second = pc.pieces(cases["repeat_across_pieces"])[1]
    other = bytes(x ^ 0x55 for x in pc.pieces(cases["repeat_across_pieces"])[0]) + second
    assert pc.walk(pc.encode(exe, tmp_path, other, tag="o")[0])[1][0] == pc.walk(pc.encode(exe, tmp_path, cases["repeat_across_pieces"])[0])[1][0]


def test_tables_are_complete_and_within_15_bits(exe, exe_san):
    for e in (exe, exe_san):
        assert subprocess.run([e, "tables"], stdout=subprocess.PIPE, check=True).stdout == b"tables %d ok\n" % pc.CODES
        assert subprocess.run([e, "consts"], stdout=subprocess.PIPE, check=True).stdout.split() == [b"%d" % pc.PIECE_RECORDS, b"%d" % pc.CODES, b"%d" % pc.MEMBER_MAX]


def test_tables_in_python():
    """the same from the header's text: Kraft sums of exactly 1, no literal/length symbol without a code, two distance symbols"""
    txt = open(pc.RULE).read()
    for name, n in (("pmz_ll_len", 286), ("pmz_d_len", 30)):
        body = re.search(name + r"\[PMZ_CODES\]\[\d+\] = \{(.*?)\};", txt, re.S).group(1)
        rows = [[int(x) for x in re.findall(r"\d+", r)] for r in re.findall(r"\{(.*?)\}", body, re.S)]
        assert len(rows) == pc.CODES
        for r in rows:
            assert len(r) == n and max(r) <= 15
            assert sum(2 ** (15 - l) for l in r if l) == 2 ** 15
            assert (min(r) >= 1) if n == 286 else (r[7] >= 1 and sum(1 for l in r if l) >= 2)


def test_eof_block(exe, tmp_path):
    subprocess.check_call([exe, "eof", str(tmp_path / "eof")])
    blk = open(tmp_path / "eof", "rb").read()
    assert blk == pc.EOF and len(blk) == 28 and gzip.decompress(blk) == b""
    assert pc.walk(blk) == [(blk, b"")]


def test_the_generator_reproduces_the_committed_tables():
    txt = open(pc.RULE).read()
    sec = pc.generator_section()
    first, last = sec.split("\n")[0], sec.rstrip("\n").split("\n")[-1]
    assert "begin" in first and "end" in last
    assert txt[txt.index(first):txt.index(last) + len(last) + 1] == sec
    assert re.findall(r"table (\d+): made from synthetic records at depth", sec) == [str(k) for k in range(pc.CODES)]


def test_entries_are_declared_exported_listed_and_mirrored():
    from pecaller_amd import build, pemap
    txt = open(os.path.join(ROOT, "include", "pemap_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+pemap_dev_fetch_records_gz\s*\(([^;]*)\)\s*;", txt)
    assert m, "include/pemap_hip.h does not declare pemap_dev_fetch_records_gz"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["dev", "first", "count", "gz_out", "gz_capacity", "gz_bytes", "n_records", "ins_records",
                                                         "ins_capacity", "n_ins"]
    assert re.search(r"\bint\s+pemap_dev_fetch_gz_ms\s*\(\s*pemap_dev\s*\*\s*dev\s*,\s*float\s*\*\s*ms4\s*\)\s*;", txt)
    lib = ctypes.CDLL(build.build())
    for name in ("pemap_dev_fetch_records_gz", "pemap_dev_fetch_gz_ms"):
        assert hasattr(lib, name) and name in pemap.SYMBOLS, name
    assert callable(getattr(pemap.PemapDev, "fetch_records_gz", None)) and callable(getattr(pemap.PemapDev, "fetch_gz_ms", None))
    assert pemap.PILEUP_GZ_PIECE_RECORDS == pc.PIECE_RECORDS
    for dep in ("pemap_gz.hip.h", "pemap_gz_rule.h"):
        assert dep in build.DEPS and os.path.exists(os.path.join(build.CSRC, dep)), dep
