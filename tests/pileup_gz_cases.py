"""Records and byte strings for the tests of the gzip rule of the device-made <out>.pileup.gz (pecaller_amd/csrc/pemap_gz_rule.h),
the stand-alone program that states the rule serially (tests/csrc/pemap_gz_rule_check.c), and a walk over BGZF members."""
import os
import re
import subprocess
import sys
import zlib
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULE = os.path.join(ROOT, "pecaller_amd", "csrc", "pemap_gz_rule.h")
CHECK_SRC = os.path.join(ROOT, "tests", "csrc", "pemap_gz_rule_check.c")
_rule = open(RULE).read()
PIECE_RECORDS = int(re.search(r"#define\s+PMZ_PIECE_RECORDS\s+(\d+)u", _rule).group(1))
PIECE = 16 * PIECE_RECORDS
CODES = int(re.search(r"#define\s+PMZ_CODES\s+(\d+)u", _rule).group(1))
HEAD = 18
MEMBER_MAX = HEAD + 5 + PIECE + 8
EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
PILE_DT = np.dtype([("pos", "<u4"), ("c", "<u2", (6,))])


def build_check(tmp_dir, sanitize=False):
    exe = os.path.join(str(tmp_dir), "pemap_gz_rule_check" + ("_san" if sanitize else ""))
    if not os.path.exists(exe):
        extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror"] + extra + ["-o", exe, CHECK_SRC])
    return exe


def encode(exe, tmp_dir, data, tag="t"):
    """-> (the members the serial rule makes of `data`, the pieces per form [stored, fixed, preset 0, ..])"""
    ip, op = (os.path.join(str(tmp_dir), tag + e) for e in (".bin", ".gz"))
    with open(ip, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, "encode", ip, op], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout[-2000:].decode(errors="replace")
    m = re.match(r"pieces (\d+) bytes (\d+) forms((?: \d+)+)\n$", r.stdout.decode())
    assert m, r.stdout
    with open(op, "rb") as f:
        gz = f.read()
    forms = [int(x) for x in m.group(3).split()]
    assert len(gz) == int(m.group(2)) and sum(forms) == int(m.group(1)) and len(forms) == 2 + CODES
    return gz, forms


def walk(gz):
    """the BGZF members of gz, found from the heads' lengths alone -> [(member bytes, its inflated bytes)]; every head is checked,
    every member is inflated on its own and its CRC-32 and ISIZE are compared"""
    out, at = [], 0
    while at < len(gz):
        head = gz[at:at + HEAD]
        assert len(head) == HEAD and head[:4] == b"\x1f\x8b\x08\x04" and head[4:10] == b"\0\0\0\0\0\xff", (at, head)
        assert head[10:16] == b"\x06\x00BC\x02\x00", (at, head)
        m = 1 + int.from_bytes(head[16:18], "little")
        assert HEAD + 2 + 8 <= m <= 65536 and at + m <= len(gz), (at, m)
        member = gz[at:at + m]
        d = zlib.decompressobj(-15)
        text = d.decompress(member[HEAD:m - 8])
        assert d.eof and not d.unused_data, "member at %d: the deflate block does not fill it" % at
        assert int.from_bytes(member[m - 8:m - 4], "little") == zlib.crc32(text) and int.from_bytes(member[m - 4:], "little") == len(text), at
        out.append((member, text))
        at += m
    return out


def pieces(data):
    return [data[k:k + PIECE] for k in range(0, len(data), PIECE)]


def records(n, seed=0, depth=30, pos0=1000):
    """n records as a run at about `depth` would leave them: positions ascending with a few gaps, the reference letter's column
    near the depth, errors in the others, rare deletions and insertions"""
    rng = np.random.default_rng(seed * 1000 + n + depth)
    out = np.zeros(n, PILE_DT)
    out["pos"] = pos0 + np.cumsum(1 + (rng.random(n) < 0.01) * rng.integers(1, 400, n))
    ref = rng.integers(0, 4, n)
    c = (rng.random((n, 6)) < 0.004 * depth).astype(np.uint16)
    c[np.arange(n), ref] = np.clip(rng.poisson(depth, n), 1, 65535)
    c[:, 4] *= rng.random(n) < 0.2
    c[:, 5] *= rng.random(n) < 0.1
    out["c"] = c
    return out


def flags_with_runs(runs, seed=3):
    """bytes whose equality flag (t[i] == t[i - 16]) has maximal runs of exactly the lengths in `runs`, in that order, each between
    bytes whose flag is clear: 16 random bytes, then per run one byte that differs from the byte 16 back and the run's copies"""
    rng = np.random.default_rng(seed)
    t = list(rng.integers(0, 256, 16))
    for r in runs:
        t.append((t[-16] + 1 + int(rng.integers(0, 255))) % 256)
        for _ in range(r):
            t.append(t[-16])
    t.append((t[-16] + 1) % 256)
    return bytes(int(x) for x in t)


def flag_runs(t):
    """the maximal runs of set flags of the piece t: their lengths"""
    out, r = [], 0
    for i in range(len(t)):
        if i >= 16 and t[i] == t[i - 16]:
            r += 1
        else:
            if r:
                out.append(r)
            r = 0
    return out + ([r] if r else [])


RUNS = (2, 3, 258, 259, 260, 261, 600)


def cases():
    """name -> bytes"""
    t = {}
    for n in (1, PIECE_RECORDS - 1, PIECE_RECORDS, PIECE_RECORDS + 1, 2 * PIECE_RECORDS + 1):
        t["records_%d" % n] = records(n).tobytes()
    for depth in (1, 5, 100, 300):
        t["depth_%d" % depth] = records(700, seed=1, depth=depth).tobytes()
    hi = records(600, seed=2, depth=30, pos0=0xfff00000)         # positions near the top of 32 bits, counters that passed 255
    hi["c"][:, :4] *= 300
    t["high_bytes"] = hi.tobytes()
    t["runs"] = flags_with_runs(RUNS)
    t["random"] = np.random.default_rng(5).integers(0, 256, PIECE + 304, dtype=np.uint8).tobytes()
    # the second piece's first 16 bytes repeat the first piece's last 16
    a = records(PIECE_RECORDS, seed=4)
    b = records(40, seed=5, pos0=10 ** 6)
    b[0] = a[-1]
    t["repeat_across_pieces"] = a.tobytes() + b.tobytes()
    # short and without a repeat: stored costs 5 bytes over the text, a preset header far more, the fixed code less than either
    t["short_fixed"] = bytes([0, 1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 7, 0, 0, 1, 1] * 3)
    return t


def generator_section():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pileup_gz_tables.py")], stdout=subprocess.PIPE, check=True)
    return r.stdout.decode()
