"""What the mapper's kernels cost a CU, as the compiler reports it: pemap_capi.hip is compiled for the device alone with the
library's own flags (pecaller_amd/build.py) and -Rpass-analysis=kernel-resource-usage, and the remarks -- not the assembly -- are
read.  Beside the seed stage's ten persistent waves per CU (14,976 bytes of LDS and 128 VGPRs each) 10,240 bytes of LDS and 128 to 256
registers per SIMD are what the other stream's kernels run in:
  * no scratch and no spilled VGPR in pm_gapless_kernel (both launches, both row forms), the first tier of pm_seed4_kernel,
    pm_band_kernel, pm_sw_kernel, pm_pile_kernel, pm_pile_walked_kernel and pm_walk_kernel;
  * the short-row forms of pm_gapless_kernel take at most 1,024 bytes of LDS per workgroup;
  * sizeof (PmSeed4Shared < 10, 0 >) is the constant a static_assert in pemap_seed4.hip.h pins, and no more than it was (14,976).
No GPU is needed; without hipcc the test skips.  The compilation takes most of a minute.

pm_gapless_kernel is compiled for four waves per SIMD in both row forms (109 and 115 VGPRs); pm_sw_kernel's bound is per form
(PM_SW_WAVES_PER_EU): under the bounds by width alone seven of its forms for reads outside 105..160 bases spilled (W = 13 under four
waves 22 to 33 VGPRs, < 16, 16, false > and < 19, *, true > under three 1 and 2).
"""
import functools
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pecaller_amd import build as pbuild        # noqa: E402

SEED4_SHARED_10_0_BEFORE = 14976                # bytes, before the gapless kernel's rows were shortened


def _hipcc():
    c = pbuild.hipcc()
    return c if (os.path.isabs(c) and os.path.exists(c)) or shutil.which(c) else None


@functools.lru_cache(maxsize=None)
def _remarks():
    """{demangled-enough kernel name: {field: int}} for every kernel of pemap_capi.hip"""
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc")
    flags = [f for f in pbuild.FLAGS if f != "-shared"]
    cmd = [cc] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull,
                          os.path.join(pbuild.CSRC, "pemap_capi.hip")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    text = r.stdout.decode(errors="replace")
    assert r.returncode == 0, text[-3000:]
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def _kernels(pattern):
    got = {k: v for k, v in _remarks().items() if re.search(pattern, k)}
    assert got, pattern
    return got


# (mangled names: _Z<len><name>I<template arguments>E...; Lb0E / Lb1E a bool, Li10E an int)
NO_SCRATCH = [r"^_Z17pm_gapless_kernelILb[01]ELb1EE", r"^_Z17pm_gapless_kernelILb[01]ELb0EE", r"^_Z15pm_seed4_kernelILi\d+ELi0EE", r"^_Z14pm_band_kernelILb[01]EE",
              r"^_Z12pm_sw_kernelILi10ELi16ELb[01]EE", r"^_Z12pm_sw_kernelI", r"^_Z14pm_pile_kernel", r"^_Z21pm_pile_walked_kernel", r"^_Z14pm_walk_kernel"]


@pytest.mark.parametrize("pattern", NO_SCRATCH)
def test_no_scratch_and_no_spill(pattern):
    bad = []
    for name, r in _kernels(pattern).items():
        print(name[:60], {k: r.get(k) for k in ("VGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")})
        if r["ScratchSize [bytes/lane]"] != 0 or r["VGPRs Spill"] != 0:
            bad.append((name[:40], r["VGPRs"], r["ScratchSize [bytes/lane]"], r["VGPRs Spill"]))
    assert not bad, bad


def test_both_launches_of_the_gapless_rule_have_both_row_forms():
    assert len(_kernels(r"^_Z17pm_gapless_kernelILb[01]ELb[01]EE")) == 4


def test_short_rows_fit_1024_bytes():
    short = _kernels(r"^_Z17pm_gapless_kernelILb[01]ELb1EE")
    assert len(short) == 2
    for name, r in short.items():
        assert r["LDS Size [bytes/block]"] <= 1024, (name, r)
    for name, r in _kernels(r"^_Z17pm_gapless_kernelILb[01]ELb0EE").items():
        assert r["LDS Size [bytes/block]"] > 1024, (name, r)         # (the long rows are the other form)


def test_seed4_shared_is_no_larger():
    _remarks()          # the compilation succeeded: the static_assert that ties the constant to sizeof holds
    src = open(os.path.join(pbuild.CSRC, "pemap_seed4.hip.h")).read()
    m = re.search(r"#define PM_S4_SHARED_10_0_BYTES (\d+)", src)
    assert m and re.search(r"static_assert \(sizeof \(PmSeed4Shared < 10, 0 >\) == PM_S4_SHARED_10_0_BYTES", src)
    assert int(m.group(1)) <= SEED4_SHARED_10_0_BEFORE
    # as the LDS of a launch it is what the remark of the kernel cannot show (dynamic), so the seed kernel's static LDS stays 0
    for name, r in _kernels(r"^_Z15pm_seed4_kernelILi10ELi0EE").items():
        assert r["VGPRs"] <= 128, (name, r)
