"""pecaller_amd/csrc/pemap_fastq_rule.h -- the rule by which reads are taken out of fastq text, shared by the host and the kernels of
pemap_fastq.hip.h -- against the Python model of tests/fastq_cases.py, on every case of its list.  tests/csrc/fastq_rule_check.c is a
stand-alone program (its own main, nothing loaded into Python) that walks a text line by line with the header; it is built plainly and
with the address and undefined-behaviour sanitizers.  No GPU is needed."""
import os
import subprocess

import pytest

import fastq_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pecaller_amd", "csrc", "pemap_fastq_rule.h")
SRC = os.path.join(ROOT, "tests", "csrc", "fastq_rule_check.c")


def _manifest(tmp_path):
    """-> (manifest path, the output the model expects)"""
    lines, want = [], []
    for i, c in enumerate(fc.CASES):
        gots = []
        for m, (text, state) in enumerate(((c["text1"], c["state1"]), (c["text2"], c["state2"]))):
            if text is None:
                continue
            p = tmp_path / ("c%d_%d.txt" % (i, m + 1))
            p.write_bytes(text)
            lines.append("mate %s %d %d %d %d %d" % (p, state, c["trim_start"], c["trim_end"], 1 if m == 0 else 0, c["max_records"]))
            r = fc.parse_mate(text, state, c["trim_start"], c["trim_end"], m == 0, c["max_records"])
            want.append("mate %d %d %d" % (r["got"], r["end"], r["bad_len"]))
            for s, nx in zip(r["records"], r["nexts"]):
                want.append(("rec", s, nx))     # (the offset the program prints is checked through the bytes that lie there)
            gots.append(r["got"])
        paired = c["text2"] is not None
        lines.append("pair %d %d %d" % (gots[0], gots[1] if paired else 0, 1 if paired else 0))
        want.append("pair %d" % fc.model_of(c)["n"])
    man = tmp_path / "manifest.txt"
    man.write_text("\n".join(lines) + "\n")
    return str(man), want


def _texts_by_mate():
    for c in fc.CASES:
        for text in (c["text1"], c["text2"]):
            if text is not None:
                yield text


def _compare(out, want):
    got = out.decode().splitlines()
    assert len(got) == len(want)
    texts = _texts_by_mate()
    text = None
    for g, w in zip(got, want):
        if isinstance(w, str):
            assert g == w
            if w.startswith("mate"):
                text = next(texts)
        else:
            _, s, nx = w
            tag, off, ln, gnx = g.split()
            assert tag == "rec" and int(gnx) == nx and int(ln) == len(s) and text[int(off):int(off) + int(ln)] == s, (g, w)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_rule_header_equals_the_model_on_every_case(tmp_path, flags):
    exe = str(tmp_path / "fastq_rule_check")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror"] + flags + ["-o", exe, SRC])
    man, want = _manifest(tmp_path)
    r = subprocess.run([exe, man], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:].decode(errors="replace"))
    _compare(r.stdout, want)


def test_the_header_is_plain_c():
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-function", "-fsyntax-only", "-x", "c", HEADER])


def test_the_case_list_covers_what_it_must():
    """the model on a few cases whose answer is plain from the rule's text, so that the model itself is pinned"""
    by = {c["name"]: fc.model_of(c) for c in fc.CASES}
    assert by["wellformed"]["n"] == 5 and by["wellformed"]["end"] == [1, 1]
    assert by["no_newline_at_all"]["n"] == 0 and by["no_newline_at_all"]["consumed"] == [0, 0]
    assert by["state0_single_line"]["got"][0] == 0 and by["state0_single_line"]["end"][0] == 1
    assert by["length_12_first"]["end"][0] == 2 and by["length_12_second"]["end"][1] == 3 and by["length_12_second"]["bad_len"][1] == 12
    assert by["length_13_first"]["end"][0] == 3 and by["length_13_first"]["bad_len"][0] == 13
    assert by["length_16_first"]["n"] == 4 and by["length_278_second"]["n"] == 4
    assert by["length_279_first"]["bad_len"][0] == 279 and by["length_279_second"]["bad_len"][1] == 279
    assert by["stop_at_max"]["end"] == [0, 0] and by["stop_at_max"]["n"] == 3
    assert by["stop_at_max_minus_1"]["end"][0] == 3 and by["stop_at_max_minus_1"]["n"] == 2
    assert by["both_stop_at_2_short_and_long"]["end"] == [2, 3] and by["both_stop_at_2_short_and_long"]["n"] == 2
    assert by["mates_differ_first_longer"]["n"] == 4 and by["mates_differ_first_longer"]["got"] == [7, 4]
    assert by["crlf"]["records"][0][0].endswith(b"\r") and len(by["crlf"]["records"][0][0]) == 31
    assert by["trim_3_2"]["records"][0][0] == fc.CASES[[c["name"] for c in fc.CASES].index("trim_3_2")]["text1"].split(b"\n")[1][3:-2]


def test_the_python_mirror_has_the_kernels_constants():
    import re
    from pecaller_amd import pemap
    src = open(os.path.join(ROOT, "pecaller_amd", "csrc", "pemap_fastq.hip.h")).read()
    block = int(re.search(r"#define PFQ_BLOCK (\d+)", src).group(1))
    assert re.search(r"#define PFQ_TILE \(PFQ_BLOCK \* 16\)", src) and pemap.FASTQ_TILE == block * 16
    assert pemap.FASTQ_TOP == int(re.search(r"#define PFQ_TOP (\d+)", src).group(1))
    per = int(re.search(r"#define PFQ_LINES_PER_LANE (\d+)", src).group(1))
    assert re.search(r"#define PFQ_LINE_TILE \(PFQ_BLOCK \* PFQ_LINES_PER_LANE\)", src) and pemap.FASTQ_LINE_TILE == block * per
    assert "pemap_dev_stage_fastq" in pemap.SYMBOLS and "pemap_dev_submit_fastq" in pemap.SYMBOLS
    assert callable(getattr(pemap.PemapDev, "stage_fastq", None)) and callable(getattr(pemap.PemapDev, "submit_fastq", None))
