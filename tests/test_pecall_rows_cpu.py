"""The row arithmetic of the device-made <outfile>.base.gz text (pecaller_amd/csrc/pecall_row_len.h: what the kernels of
pecall_rows.hip.h and pecaller_main.c both call) on the CPU, and the C-ABI entry pecall_dev_sites_base_text as a name."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_arithmetic_equals_sprintf(tmp_path):
    """a stand-alone program (its own main, nothing loaded into Python) built with the address and undefined-behaviour sanitizers:
    digit count and digit bytes of 0, 9, 10, 99, 100, ... 999999999, 1000000000, 2147483647 and 6,000 generated positions equal
    sprintf("%d"); the length of a template row equals strlen of the row sprintf builds, for 1, 3, 64, 65 and 512 samples, contig
    names of 1 and 23 bytes and a position of every digit count; 2^22 rows of 512 samples sum beyond 32 bits"""
    exe = str(tmp_path / "row_len_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "row_len_check.c")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout[-2000:].decode(errors="replace")
    assert b"6030 positions, 110 rows, 0 disagree" in r.stdout


def test_the_header_is_plain_c():
    """no HIP types in pecall_row_len.h: it compiles as C99 on its own"""
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c",
                           os.path.join(ROOT, "pecaller_amd", "csrc", "pecall_row_len.h")])


def test_base_text_entry_is_declared_exported_listed_and_mirrored():
    from pecaller_amd import build, pemap, pecall
    txt = open(os.path.join(ROOT, "include", "pemap_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+pecall_dev_sites_base_text\s*\(([^;]*)\)\s*;", txt)
    assert m, "include/pemap_hip.h does not declare pecall_dev_sites_base_text"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["dev", "names", "name_off", "n_contigs", "contig", "pos", "ref_char", "text", "text_cap", "n_text",
                                                         "hole_site", "hole_at", "hole_cap", "n_holes", "kernel_ms3"]
    assert "uint64_t text_cap" in args and "uint64_t * n_text" in args and "uint64_t * hole_at" in args
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "pecall_dev_sites_base_text")
    assert "pecall_dev_sites_base_text" in pemap.SYMBOLS
    assert callable(getattr(pecall.PecallDev, "base_text", None))
    for dep in ("pecall_rows.hip.h", "pecall_row_len.h"):
        assert dep in build.DEPS and os.path.exists(os.path.join(build.CSRC, dep)), dep
