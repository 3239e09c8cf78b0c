"""The gzip rule of the device-made <outfile>.base.gz (pecaller_amd/csrc/pecall_gz_rule.h: what the kernels of pecall_gz.hip.h and
tests/csrc/gz_rule_check.c both call) on the CPU, through the stand-alone program, and the C-ABI entry pecall_dev_sites_base_gz as
a name."""
import ctypes
import gzip
import os
import re
import subprocess
import zlib
import numpy as np
import pytest
import gz_cases as gc

ROOT = gc.ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """built with the address and undefined-behaviour sanitizers: a program of its own, nothing of it is loaded into Python"""
    return gc.build_check(tmp_path_factory.mktemp("gz_rule"), sanitize=True)


@pytest.fixture(scope="module")
def cases():
    return gc.texts()


def test_the_header_is_plain_c():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", gc.RULE])
    assert 0 < gc.PCG_PIECE <= 32768


def test_the_cases_cover_what_they_should(cases):
    P = gc.PCG_PIECE
    assert [len(cases["run_" + k][0]) for k in ("piece_minus_1", "piece", "piece_plus_1", "two_pieces_plus_1")] == [P - 1, P, P + 1, 2 * P + 1]
    assert [len(gc.pieces(cases["run_two_pieces_plus_1"][0])[k]) for k in range(3)] == [P, P, 1]
    assert any(b >= 144 for b in cases["high_name"][0])
    cuts = cases["adjacent_cuts"][1]
    assert any(a == b for a, b in zip(cuts[:-1], cuts[1:])) and cuts[0] == 0 and cuts[-1] == len(cases["adjacent_cuts"][0])


@pytest.mark.parametrize("name", sorted(gc.texts()))
def test_members_of_a_text(exe, cases, tmp_path, name):
    """every member inflates on its own to its piece; the gzip module accepts the whole (CRC-32 and ISIZE); the whole inflates to
    the text; no member is longer than the stored form of its piece"""
    text, cuts = cases[name]
    gz = gc.encode(exe, tmp_path, text, cuts)
    want = gc.pieces(text, cuts)
    got = gc.members(gz)
    assert len(got) == len(want)
    for (member, inflated), piece in zip(got, want):
        assert inflated == piece
        assert member[:10] == gc.HEAD
        assert len(member) <= gc.stored_len(piece)
    assert gzip.decompress(gz) == text if text else gz == b""
    assert b"".join(m for m, _ in got) == gz


def test_sizes(exe, cases, tmp_path):
    """regular rows shrink well below the stored form; random bytes go as stored blocks, exactly; a match of 258 is one token and one
    of 259 is not"""
    text = cases["rows_64"][0]
    assert len(gc.encode(exe, tmp_path, text)) * 6 < len(text)
    text = cases["identical_rows"][0]
    assert len(gc.encode(exe, tmp_path, text)) * 20 < len(text)
    text = cases["random"][0]
    assert len(gc.encode(exe, tmp_path, text)) == sum(gc.stored_len(p) for p in gc.pieces(text))
    by = {m: len(gc.encode(exe, tmp_path, cases["match_of_%d" % m][0])) for m in (3, 258, 259)}
    assert by[258] <= by[3] + 1 and by[259] > by[258]


def test_no_match_reaches_in_front_of_its_piece(exe, cases, tmp_path):
    """a member made of a piece alone equals the member made of it inside a longer text"""
    text = cases["run_two_pieces_plus_1"][0]
    whole = gc.members(gc.encode(exe, tmp_path, text))
    for k, piece in enumerate(gc.pieces(text)):
        assert gc.encode(exe, tmp_path, piece, tag="p%d" % k) == whole[k][0]


def test_crc_combine_equals_zlib(exe, tmp_path):
    """slice counts 1 .. 130 over lengths that leave a ragged, an empty and a one-byte last slice"""
    rng = np.random.default_rng(9)
    n_runs = 0
    for length in (1, 2, 129, 1000, gc.PCG_PIECE):
        data = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        path = str(tmp_path / ("crc_%d" % length))
        with open(path, "wb") as f:
            f.write(data)
        want = "%08x" % zlib.crc32(data)
        for slices in (range(1, 131) if length in (129, 1000) else (1, 2, 3, 64, 130)):
            out = subprocess.run([exe, "crc", path, str(slices)], stdout=subprocess.PIPE, check=True).stdout.split()
            assert out == [want.encode(), want.encode()], (length, slices)
            n_runs += 1
    assert n_runs > 260


def test_base_gz_entry_is_declared_exported_listed_and_mirrored():
    from pecaller_amd import build, pemap, pecall
    txt = open(os.path.join(ROOT, "include", "pemap_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+pecall_dev_sites_base_gz\s*\(([^;]*)\)\s*;", txt)
    assert m, "include/pemap_hip.h does not declare pecall_dev_sites_base_gz"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["dev", "names", "name_off", "n_contigs", "contig", "pos", "ref_char", "gz", "gz_cap", "n_gz",
                                                         "hole_site", "hole_gz_at", "hole_cap", "n_holes", "n_text", "kernel_ms5"]
    assert "unsigned char *gz" in args and "uint64_t gz_cap" in args and "uint64_t * n_gz" in args and "uint64_t * hole_gz_at" in args
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "pecall_dev_sites_base_gz")
    assert "pecall_dev_sites_base_gz" in pemap.SYMBOLS
    assert callable(getattr(pecall.PecallDev, "base_gz", None))
    assert pecall.PCG_PIECE == gc.PCG_PIECE
    for dep in ("pecall_gz.hip.h", "pecall_gz_rule.h"):
        assert dep in build.DEPS and os.path.exists(os.path.join(build.CSRC, dep)), dep
