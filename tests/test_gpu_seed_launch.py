"""How many persistent waves of the fused seed kernel's first tier are launched per CU: the knob (PEMAP_LOOKUP_WAVES) capped by what
the runtime keeps resident for the launched form with its dynamic LDS (pemap_dev_seed_launch).  On the r150 golden set every setting
-- one wave, the old default of ten, eleven, twelve, and the register bound of sixteen -- gives the reference's coordinates and
pileup and the same counters; one device object per setting, the knobs being read when the object is made."""
import numpy as np
import pytest

import fixtures

pytestmark = pytest.mark.gpu
SETTINGS = (1, 10, 11, 12, 16)


def _run(monkeypatch, waves):
    from pecaller_amd import PemapDev
    if waves is None:
        monkeypatch.delenv("PEMAP_LOOKUP_WAVES", raising=False)
    else:
        monkeypatch.setenv("PEMAP_LOOKUP_WAVES", str(waves))
    ix = fixtures.index()
    r1, l1, r2, l2 = fixtures.reads("r150")
    dev = PemapDev(0)
    try:
        dev.build_index(ix["genome"], ix["contig_len"])
        assert dev.lookup_replicas()[0] == 8
        dev.set_params(paired=True, min_dist=0, max_dist=500, min_align=0.85)
        before = dev.seed_launch()
        m1, m2, mt = dev.map_batch(r1, l1, r2, l2)
        counts, ins = dev.fetch_pileup()
        stats, _ = dev.run_stats()
        return dict(m1=m1, m2=m2, mt=mt, counts=counts, ins=sorted(ins), summary=np.array(dev.summary()), stats=stats, launch=dev.seed_launch(),
                    before=before)
    finally:
        dev.close()


@pytest.fixture(scope="module")
def base():
    mp = pytest.MonkeyPatch()
    try:
        yield _run(mp, None)
    finally:
        mp.undo()


def test_default_launch_is_resident_and_golden(base):
    la = base["launch"]
    print(la)
    assert base["before"] == dict(asked=0, resident=0, launched=0, lds_bytes=0)
    # the first tier for reads of up to 160 bases: twelve waves of it fit a CU's 160 KB under either allocation granule
    assert la["lds_bytes"] <= 12800 and la["resident"] >= 12 and la["asked"] == 12
    assert la["resident"] >= la["launched"] == min(la["asked"], la["resident"])
    assert np.array_equal(base["m1"], fixtures.golden_m("r150", 1)) and np.array_equal(base["m2"], fixtures.golden_m("r150", 2))
    fixtures.check_pileup_against_golden("r150", base["counts"])


@pytest.mark.parametrize("waves", SETTINGS)
def test_every_wave_count_computes_the_same(base, waves, monkeypatch):
    got = _run(monkeypatch, waves)
    la = got["launch"]
    print(la)
    assert la["asked"] == waves and la["lds_bytes"] == base["launch"]["lds_bytes"] and la["resident"] == base["launch"]["resident"]
    assert la["resident"] >= la["launched"] == min(waves, la["resident"])
    for k in ("m1", "m2", "mt", "counts", "summary"):
        assert np.array_equal(got[k], base[k]), k
    assert got["ins"] == base["ins"]
    assert got["stats"] == base["stats"]
