"""The fused seed kernel's footprint after the hit list, the per-segment counts and the read's 2-bit codes left LDS of their own
(pemap_seed4.hip.h), read from the same compiler remarks as test_kernel_resources_cpu.py:
  * PM_S4_SHARED_10_0_BYTES, which a static_assert ties to sizeof (PmSeed4Shared < 10, 0 >), is at most 12,800: twelve waves on a
    CU's 163,840 bytes of LDS, whether the allocation granule is 512 or 1,280 bytes (the work did not stop at the 11-wave size);
  * no first-tier form of pm_seed4_kernel has scratch or a spilled VGPR, < 10, 0 > holds at most 128 VGPRs;
  * sizeof (PmSeed4Shared < 19, 1 >) stays under 65,536 (the header's static_assert: the compilation succeeds).
No GPU is needed; without hipcc the tests skip."""
import os
import re

from pecaller_amd import build as pbuild
from test_kernel_resources_cpu import _kernels, _remarks

SEED4_SHARED_10_0_MOST = 12800


def _header():
    return open(os.path.join(pbuild.CSRC, "pemap_seed4.hip.h")).read()


def test_twelve_waves_of_the_first_tier_fit_a_cu():
    _remarks()          # (compiled: both static_asserts hold)
    src = _header()
    m = re.search(r"#define PM_S4_SHARED_10_0_BYTES (\d+)", src)
    assert m and re.search(r"static_assert \(sizeof \(PmSeed4Shared < 10, 0 >\) == PM_S4_SHARED_10_0_BYTES", src)
    size = int(m.group(1))
    assert size <= SEED4_SHARED_10_0_MOST
    for granule in (512, 1280):
        assert 12 * (-(-size // granule) * granule) <= 160 * 1024, granule
    assert re.search(r"static_assert \(sizeof \(PmSeed4Shared < 19, 1 >\) <= 65536", src)
    # the members that left: the byte array of the codes and a hit list of its own
    struct = src[src.index("struct __align__ (16) PmSeed4Shared"):src.index("static_assert (sizeof (PmSeed4Shared < 19, 1 >)")]
    assert not re.search(r"uint8_t seq\[", struct) and not re.search(r"hits\[PM_MAX_HITS\]", struct)


def test_first_tier_forms_have_no_scratch_and_no_spill():
    forms = _kernels(r"^_Z15pm_seed4_kernelILi\d+ELi0EE")
    assert len(forms) >= 5
    for name, r in forms.items():
        print(name[:40], r["VGPRs"], r["ScratchSize [bytes/lane]"], r["VGPRs Spill"])
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (name, r)


def test_the_form_for_reads_of_up_to_160_bases_holds_128_vgprs():
    (name, r), = _kernels(r"^_Z15pm_seed4_kernelILi10ELi0EE").items()
    assert r["VGPRs"] <= 128, (name, r)
