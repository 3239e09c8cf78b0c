"""What the fastq kernels (pecaller_amd/csrc/pemap_fastq.hip.h) cost a CU, as the compiler reports it.  They run on the copy stream
beside the seed stage's ten persistent waves per CU, where the other stream's kernels get 10,240 bytes of LDS,
so each of them uses no scratch, no spilled VGPR, at most 128 VGPRs and at most 10,240 bytes of static LDS per workgroup.  The remarks
are those of test_kernel_resources_cpu.py's compilation of pemap_capi.hip (one compilation serves both files in one session).
No GPU is needed; without hipcc the test skips."""
import pytest

from test_kernel_resources_cpu import _kernels

KERNELS = ["pfq_nl_count_kernel", "pfq_sum_top_kernel", "pfq_nl_apply_kernel", "pfq_role_sum_kernel", "pfq_role_top_kernel", "pfq_records_kernel",
           "pfq_rows_kernel"]


@pytest.mark.parametrize("name", KERNELS)
def test_footprint_beside_the_seed_stage(name):
    got = _kernels(r"^_Z%d%s" % (len(name), name))
    assert len(got) == 1, list(got)
    for k, r in got.items():
        print(k[:60], {f: r.get(f) for f in ("VGPRs", "SGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")})
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, r
        assert r["VGPRs"] <= 128, r
        assert r["LDS Size [bytes/block]"] <= 10240, r
