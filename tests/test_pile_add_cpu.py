"""The word arithmetic of pemap_dev_absorb's counter sum (pm_add_u16x2, pecaller_amd/csrc/pemap_pile_add.h: the function
pm_pile_add_kernel calls per 32-bit word) on the CPU, and the two C-ABI entries of the multi-object path as names."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pemap_dev_index_share", "pemap_dev_absorb"]


def test_add_u16x2_equals_two_u16_additions(tmp_path):
    """a stand-alone program (its own main, nothing loaded into Python) built with the address and undefined-behaviour sanitizers:
    49 x 49 edge-value word pairs and 1 M generated ones must equal two separate uint16_t additions -- each half modulo 2^16, no
    carry from the low half into the high one"""
    exe = str(tmp_path / "pile_add_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "pile_add_check.c")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout[-2000:].decode(errors="replace")
    assert b"1002401 word pairs, 0 disagree" in r.stdout


def test_the_header_is_plain_c():
    """no HIP types in pemap_pile_add.h: it compiles as C99 on its own"""
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c",
                           os.path.join(ROOT, "pecaller_amd", "csrc", "pemap_pile_add.h")])


def test_multi_object_entries_are_declared_exported_and_listed():
    from pecaller_amd import build, pemap
    txt = open(os.path.join(ROOT, "include", "pemap_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = ctypes.CDLL(build.build())
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*pemap_dev\s*\*\s*dst\s*,\s*pemap_dev\s*\*\s*src\s*\)\s*;" % name, txt), name
        assert hasattr(lib, name), name
        assert name in pemap.SYMBOLS, name
    assert hasattr(pemap.PemapDev, "index_share") and hasattr(pemap.PemapDev, "absorb")
