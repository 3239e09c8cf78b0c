"""The difference form of a pileup counter plane (pecaller_amd/csrc/pemap_pile_diff.h: the signed half-word add with its take-back,
the per-word unfold and fold steps, the combine of tile sums -- what pm_pile_kernel and the two conversions call per 32-bit word)
against plain uint16_t arithmetic on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_difference_form_equals_u16_increments(tmp_path):
    """a stand-alone program (its own main, nothing loaded into Python) built with the address and undefined-behaviour sanitizers, on
    4,099 positions with edge values planted: fold (unfold (x)) == x; 100,000 ranges (the whole genome, single positions, abutting
    ones and 70,000 over one position among them) applied as two word adds with take-back equal uint16_t increments on every half;
    the fold in tiles of 1, 2, 64 and 4,096 words equals the serial one"""
    exe = str(tmp_path / "pile_diff_check")
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "pile_diff_check.c")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout[-2000:].decode(errors="replace")
    assert b"round trip 0 words differ; 100000 ranges, 0 halves differ; tiled folds 0 words differ" in r.stdout


def test_the_header_is_plain_c():
    """no HIP types in pemap_pile_diff.h: it compiles as C99 on its own"""
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c",
                           os.path.join(ROOT, "pecaller_amd", "csrc", "pemap_pile_diff.h")])
