"""Texts and columns for the tests of the gzip rule of the device-made <outfile>.base.gz (pecaller_amd/csrc/pecall_gz_rule.h), and the
stand-alone program that states the rule serially (tests/csrc/gz_rule_check.c)."""
import os
import re
import subprocess
import zlib
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = os.path.join(ROOT, "pecaller_amd", "csrc", "pecall_gz_rule.h")
PCG_PIECE = int(re.search(r"#define\s+PCG_PIECE\s+(\d+)u", open(RULE).read()).group(1))
HEAD = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3])
GEN = "ACGTDIMRWSYKEHN"


def build_check(tmp_dir, sanitize=False):
    exe = os.path.join(str(tmp_dir), "gz_rule_check" + ("_san" if sanitize else ""))
    if not os.path.exists(exe):
        extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "csrc", "gz_rule_check.c")])
    return exe


def encode(exe, tmp_dir, text, cuts=None, tag="t"):
    """-> the members the serial rule makes of `text`, cut into runs at `cuts`"""
    tp, op, cp = (os.path.join(str(tmp_dir), tag + e) for e in (".txt", ".gz", ".cuts"))
    with open(tp, "wb") as f:
        f.write(text)
    cmd = [exe, "encode", tp, op]
    if cuts is not None:
        with open(cp, "w") as f:
            f.write("".join("%d\n" % int(c) for c in cuts))
        cmd.append(cp)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout[-2000:].decode(errors="replace")
    with open(op, "rb") as f:
        return f.read()


def members(gz):
    """-> [(member bytes, its inflated bytes)], each inflated on its own"""
    out, rest = [], bytes(gz)
    while rest:
        d = zlib.decompressobj(31)
        text = d.decompress(rest)
        assert d.eof, "a member that does not end"
        used = len(rest) - len(d.unused_data)
        out.append((rest[:used], text))
        rest = d.unused_data
    return out


def pieces(text, cuts=None):
    """the pieces the rule cuts `text` into"""
    edges = [0] + [int(c) for c in (cuts if cuts is not None else [])] + [len(text)]
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        out += [text[k:min(b, k + PCG_PIECE)] for k in range(a, b, PCG_PIECE)]
    return out


def stored_len(piece):
    return 10 + 5 + len(piece) + 8


def row(name, pos, ref, calls):
    name = name if isinstance(name, bytes) else name.encode()
    return b"\n" + name + b"\t%d\t" % pos + ref.encode() + b"".join(b"\t" + GEN[c].encode() + b"\t1" for c in calls)


def rows(n_rows, n, name="chr7", pos0=1000, seed=0, p_n=0.03, same=False):
    """template rows of n samples at consecutive positions: random reference letters, every sample calls the reference, p_n of
    the calls 'N'; same: every row equal to the first"""
    rng = np.random.default_rng(seed + 7 * n + n_rows)
    out = []
    for r in range(n_rows):
        ref = int(rng.integers(0, 4))
        calls = np.where(rng.random(n) < p_n, 14, ref)
        out.append(row(name, pos0 + r, GEN[ref], calls))
    if same:
        out = [out[0]] * n_rows
    return b"".join(out)


def run_of(length, n=8, seed=0):
    """template rows of exactly `length` bytes in all: names of up to 1,024 bytes make up the difference"""
    base = len(row("c", 1000, "A", [0] * n))            # 4-digit positions from 1000 on
    k = length // base
    body = rows(k - 1, n, name="c", pos0=1000, seed=seed)
    left = length - len(body)
    name_len = left - (base - 1)
    assert 1 <= name_len <= 1024, (length, name_len)
    rng = np.random.default_rng(seed)
    out = body + row("x" * name_len, 1000 + k - 1, "C", np.where(rng.random(n) < 0.03, 14, 1))
    assert len(out) == length
    return out


def texts():
    """name -> (text, cuts or None)"""
    P = PCG_PIECE
    t = {}
    for n in (1, 3, 64, 65, 130, 512):
        t["rows_%d" % n] = (rows(40 if n < 512 else 12, n), None)
    t["identical_rows"] = (rows(60, 64, same=True), None)
    t["pos_9_to_10"] = (rows(4, 8, pos0=8), None)
    t["pos_999999_to_1000000"] = (rows(6, 64, pos0=999997), None)
    t["name_1_to_23"] = (rows(3, 65, name="c", pos0=5000) + rows(3, 65, name="chr12_KI270904v1_altern", pos0=5003, seed=1), None)
    for tag, length in (("piece_minus_1", P - 1), ("piece", P), ("piece_plus_1", P + 1), ("two_pieces_plus_1", 2 * P + 1)):
        t["run_" + tag] = (run_of(length), None)
    # a piece boundary inside a row and inside a match: 130 samples that all call the same letter, a row of ~530 bytes of period 4
    inside = rows(2 * P // 500, 130, p_n=0.0)
    assert inside[P - 8:P + 8].count(b"\n") == 0 and inside[P - 8:P + 8] == inside[P - 12:P + 4]
    t["cut_inside_a_match"] = (inside, None)
    for m in (3, 258, 259):
        # exactly m bytes equal to those four in front of them: "abcd", then its first m bytes of period 4, then a byte that differs
        t["match_of_%d" % m] = (b"abcd" + (b"abcd" * 70)[:m] + b"#wxyz", None)
    t["one_row"] = (rows(1, 64), None)
    t["one_byte"] = (b"\n", None)
    t["high_name"] = (rows(9, 8, name=bytes(range(144, 256)) + b"\xff\x90"), None)
    t["random"] = (np.random.default_rng(5).integers(0, 256, P + 300, dtype=np.uint8).tobytes(), None)
    t["short_rows"] = (b"\n\n\n\nab\nab\nab\n\n\nabc\nabc\nabd\n" * 20, None)
    body = rows(80, 64, seed=3)
    starts = [i for i in range(len(body)) if body[i:i + 1] == b"\n"]
    t["adjacent_cuts"] = (body, [0, 0, starts[3], starts[3], starts[3], starts[10], starts[11], starts[50] + 5, len(body), len(body)])
    t["cuts_in_long_text"] = (rows(150, 64, seed=4), [starts[1], starts[2], starts[2] + 2 * P + 17])
    return t


def low_hole_columns(n=8):
    """columns without a variant at consecutive positions, every read the reference letter: no hole.  348 rows of a one-byte name
    and one of a longer name, sized so that the text is one run of 2 * PCG_PIECE + 1 bytes: three pieces, the last of one byte.
    -> reads, dom, names, contig, pos, ref"""
    short = len(row("c", 1000, "A", [0] * n))
    total = 2 * PCG_PIECE + 1
    k = total // short - 1
    last = total - k * short
    name_len = last - (short - 1)
    assert 1 <= name_len <= 1024
    rng = np.random.default_rng(11)
    dom = rng.integers(0, 4, k + 1).astype(np.uint8)
    reads = np.zeros((k + 1, n, 6), np.uint16)
    reads[np.arange(k + 1), :, dom] = 30
    contig = np.zeros(k + 1, np.int32)
    contig[-1] = 1
    pos = (1000 + np.arange(k + 1)).astype(np.uint32)
    ref = np.frombuffer(b"ACGT", np.uint8)[dom]
    return reads, dom, ["c", "L" * name_len], contig, pos, ref
