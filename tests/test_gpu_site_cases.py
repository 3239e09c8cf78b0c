"""The per-site caller's kernels on the planted columns of site_cases.py: every family of a sample count in one array (two chunks under
PECALL_CHUNK_LOG2=8, planted and plain columns mixed in every piece of eight), against the oracle, for every knob setting, parameter
set and entry point; the reference's own rows for 8 and 129 samples; the run statistics against the hand-off rules.

The tuning knobs are read once per object by pecall_dev_create, so an object of its own is what a setting needs; each check below makes
its own objects."""
import numpy as np
import pytest

import site_cases as sc
from test_pecall_sites import _chunk_coverage

pytestmark = pytest.mark.gpu

KNOBS = (dict(), dict(PECALL_HEAVY_MIN="0", PECALL_HEAVY_MIN_WIDE="0"), dict(PECALL_HEAVY_MIN_WIDE="1"), dict(PECALL_HEAVY_WAVES="1"))


def _dev(monkeypatch, knobs):
    from pecaller_amd.pecall import PecallDev
    for k in ("PECALL_HEAVY_MIN", "PECALL_HEAVY_MIN_WIDE", "PECALL_HEAVY_WAVES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PECALL_CHUNK_LOG2", "8")
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    return PecallDev(0)


def _kw(N, run):
    kw = {k: v for k, v in sc.RUNS[run].items() if k != "chrom"}
    kw["chrom"] = sc.run_chrom(N, run)
    return kw


def _same_as_oracle(got, e, what):
    assert np.array_equal(got[0], e["call"]), what
    assert np.array_equal(got[2], e["type"]) and np.array_equal(got[3], e["ac"]) and np.array_equal(got[4], e["passes"]), what
    assert np.max(np.abs(got[1] - e["p"])) <= 1e-6, what          # north_star: genotype posteriors within 1e-6


def _dense(sparse, n, N):
    call, (site, rows), typ, ac, npass = sparse
    p = np.ones((n, N))
    p[site] = rows
    return call, p, typ, ac, npass


@pytest.mark.parametrize("N", sc.SIZES)
def test_gpu_planted_columns_every_knob_parameter_and_entry_point(N, monkeypatch):
    from pecaller_amd.pemap import PemapError
    a = sc.arrays(N)
    reads, dom = a["reads"], a["dom"]
    assert len(dom) > 256                           # two chunks
    first = {}
    for knobs in KNOBS:
        dev = _dev(monkeypatch, knobs)
        for run in sc.RUNS:
            kw = _kw(N, run)
            got = [x.copy() for x in dev.call_sites(reads, dom, **kw)]
            _same_as_oracle(got, sc.expected(N, run), (knobs, run))
            # bit for bit the same under every knob setting and through every entry point, posteriors included
            entries = [("call_sites", got)]
            if run in ("default", "weak_prior", "haploid") or not knobs:
                entries.append(("sparse", _dense(dev.call_sites_sparse(reads, dom, **kw), len(dom), N)))
                dev.sites_stage(reads, dom, chrom=kw["chrom"])
                dev.sites_run(**{k: v for k, v in kw.items() if k != "chrom"})
                entries.append(("resident", dev.sites_collect()))
            for name, res in entries:
                ref = first.setdefault(run, got)
                assert all(np.array_equal(x, y) for x, y in zip(res, ref)), (knobs, run, name)
        if not knobs:
            # theta: both ends of the accepted interval are runs above (0.5 and 1e-10); just outside is refused, and the object still works
            for theta in (np.nextafter(0.5, 1.0), np.nextafter(1e-10, 0.0)):
                with pytest.raises(PemapError):
                    dev.call_sites(reads[:8], dom[:8], theta=float(theta))
            assert all(np.array_equal(x, y) for x, y in zip(dev.call_sites(reads, dom, chrom=a["chrom"]), first["default"]))
        dev.close()


@pytest.mark.parametrize("N", [8, 129])
def test_gpu_planted_columns_match_reference_text(N, monkeypatch):
    """the rows the reference itself printed for the planted columns (%g: six significant digits), under the defaults and with the small
    beam taking the carriers' columns"""
    f = sc.reference(N)
    for knobs in KNOBS[:2]:
        dev = _dev(monkeypatch, knobs)
        for run, kw in sc.REFERENCE_RUNS.items():
            call, p, typ, ac, _ = dev.call_sites(f["reads"], f["dom"], **kw)
            bad = sc.reference_mismatches(N, run, call, p, typ, ac)
            assert not bad, (knobs, run, len(bad), bad[:2])
        dev.close()


def _too_deep(a):
    return (a["reads"].astype(np.int64).sum(2) + 601 >= 2048).any(1) & (a["dom"] < 4)


@pytest.mark.parametrize("N", sc.SIZES)
def test_gpu_small_beam_hands_off_what_the_rules_say(N, monkeypatch):
    """PECALL_HEAVY_MIN=0: no early list, every column with an unsettled sample reaches the small beam, and what it does not keep is listed
    for the beam search.  The listed count of pecall_dev_sites_stats against pcs_mini_core's hand-off rules (the comment above
    PCS_MINI_U) evaluated on the oracle's pass-1 statistics; beyond 128 samples a column too deep for the head of the ln n! table is
    listed as well, up to 128 it goes to the deep list and the second pass (whose listings the statistics add)."""
    a = sc.arrays(N)
    dev = _dev(monkeypatch, KNOBS[1])
    deep = _too_deep(a)
    for run in ("default", "weak_prior", "haploid", "chrom_turn"):
        kw = _kw(N, run)
        e = sc.expected(N, run)
        h = sc.hand_off(N, e["stats"])
        handed = h["many"] | h["early"] | h["long"] | h["no_hom"] | h["changed"]
        if N > 128:
            handed = handed | (deep & (e["passes"] >= 1))
        dev.sites_stage(a["reads"], a["dom"], chrom=kw["chrom"])
        dev.sites_run(**{k: v for k, v in kw.items() if k != "chrom"})
        st = dev.sites_stats()
        print(N, run, st, int(handed.sum()), {k: int(v.sum()) for k, v in h.items()})
        assert st["columns"] == len(a["dom"]) and st["early"] == [0, 0, 0, 0]
        assert st["deep"] == (int(deep.sum()) if N <= 128 else 0)
        assert sum(st["listed"]) == int(handed.sum()), (run, st, int(handed.sum()))
        _same_as_oracle(dev.sites_collect(), e, run)
    # the planted small-beam columns the rules keep were kept (weak_prior: lists of two to four configurations in one pass)
    assert (h["live"] & ~handed & a["planted"]).sum() >= 10
    dev.close()


@pytest.mark.parametrize("N", sc.SIZES)
def test_gpu_early_list_is_the_variant_read_rule(N, monkeypatch):
    """the defaults: the columns started ahead of the shortcut kernels are those with PECALL_HEAVY_MIN (1; beyond 128 samples 3) or more
    samples of three or more reads off the reference base that are an eighth of their depth (_chunk_coverage's rule)"""
    a = sc.arrays(N)
    e = sc.expected(N)
    for knobs, thr in ((KNOBS[0], 1 if N <= 128 else 3), (KNOBS[2], 1)):
        dev = _dev(monkeypatch, knobs)
        early = _chunk_coverage(a["reads"], a["dom"], e["p"], 256, thr)[3]
        dev.sites_stage(a["reads"], a["dom"], chrom=a["chrom"])
        dev.sites_run()
        st = dev.sites_stats()
        print(N, knobs, st, int(early.sum()))
        assert sum(st["early"]) == int(early.sum()) and early.sum() >= 10          # (an early list worth counting: 19 columns at the wide threshold)
        # an early-listed column is in no other list; the deep list holds the others that are too deep for the table's head
        r = a["reads"].astype(np.int64)
        tot = r.sum(2)
        ref = r[np.arange(len(tot))[:, None], np.arange(N)[None, :], np.minimum(a["dom"], 3)[:, None]]
        is_early = (((tot - ref >= 3) & (8 * (tot - ref) >= tot)).sum(1) >= thr) & (a["dom"] < 4)
        assert st["deep"] == (int((_too_deep(a) & ~is_early).sum()) if N <= 128 else 0)
        dev.close()
    # sites_stats is for a finished run
    from pecaller_amd.pemap import PemapError
    dev = _dev(monkeypatch, KNOBS[0])
    with pytest.raises(PemapError):
        dev.sites_stats()
    dev.sites_stage(a["reads"], a["dom"])
    with pytest.raises(PemapError):
        dev.sites_stats()
    dev.close()
