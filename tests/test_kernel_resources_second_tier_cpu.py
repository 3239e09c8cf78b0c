"""The second tier of pm_seed4_kernel as the compiler reports it (the remarks test_kernel_resources_cpu.py reads for the first tier,
from the same compilation): eight loads of tail elements and a second set of record headers in flight are registers, and the
form runs one wave a SIMD under __launch_bounds__ (64, 2) -- no scratch and no spilled VGPR in any form, and no more than the 128
VGPRs that leave a SIMD's other half to the ALU stream's kernels.  No GPU is needed; without hipcc the test skips."""
import re

import test_kernel_resources_cpu as kr

SECOND_TIER = r"^_Z15pm_seed4_kernelILi\d+ELi1EE"


def test_every_read_length_has_a_second_tier():
    forms = sorted(int(re.search(r"ILi(\d+)ELi1EE", k).group(1)) for k in kr._kernels(SECOND_TIER))
    assert forms == [7, 10, 13, 16, 19]


def test_second_tier_no_scratch_no_spill_half_a_simd():
    bad = []
    for name, r in kr._kernels(SECOND_TIER).items():
        print(name[:40], {k: r.get(k) for k in ("VGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "Occupancy [waves/SIMD]")})
        if r["ScratchSize [bytes/lane]"] != 0 or r["VGPRs Spill"] != 0 or r["VGPRs"] > 128:
            bad.append((name[:40], r["VGPRs"], r["ScratchSize [bytes/lane]"], r["VGPRs Spill"]))
    assert not bad, bad
